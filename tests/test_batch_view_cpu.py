"""record_of (bbmap_amd/csrc/batch_view.h) on the host: the two tier rules on a hand-made view of four reads.

The expected lines are worked out from the rules as batch_view.h states them, not from a run: ByList takes the tier's record where the
main list's count is BBMAP_NSITES_IN_TIER (-3), ByRecord where the main final record's nsites is; both need a tier record
(tierIdx >= 0) and a batch with tier reads (tierIdx not null).  n is the count of the list taken, clamped to [0, cap]; flag is the
main list's raw count.  Read 2 is the one on which the rules disagree."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# read, rule, t(ier) / m(ain), n, flag, match length
EXPECTED = """\
0 list m 2 5 7
1 list t 3 -3 9
2 list t 1 -3 4
3 list m 0 -3 0
0 record m 2 5 7
1 record t 3 -3 9
2 record m 0 -3 0
3 record m 0 -3 0
0 list-notier m 2 5 7
1 list-notier m 0 -3 0
2 list-notier m 0 -3 0
3 list-notier m 0 -3 0
"""


def test_tier_rules_on_a_hand_made_view(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "batch_view_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "bbmap_amd", "csrc"), os.path.join(ROOT, "tests", "batch_view_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert out == EXPECTED
    # the rules differ on read 2 and nowhere else
    by_list, by_record = out.splitlines()[0:4], out.splitlines()[4:8]
    assert [a.split()[2:] != b.split()[2:] for a, b in zip(by_list, by_record)] == [False, False, True, False]
