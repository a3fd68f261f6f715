"""plan_route (bbmap_amd/csrc/msa_route.h) on the host: which kernels a DP launch runs, from the context's switches and its size.

The expected lines are worked out from the rule as DESIGN 3.7 states it, not from a run.  9PacBio: nothing but `indirect` and
`pipelined` = a host count, pipeJobsMax > 0 and n <= pipeJobsMax.  11ts: band = the band kernel is present and not switched off;
wide = the wide pass is present; sorted = sortByWidth, a host count, n >= 256, n > latencyJobs, and no band kernel unless
sortWithBand; latency = wide, a host count, no band kernel, n <= latencyJobs; unlList = sorted and unlimitedLoop; wideBoth =
wideUnlimited in a context without a band.  Each line lists the fields that are true ("-": none); "dev" marks a job count read on the
device.  Every 11ts case but 10 has a wide pass; cases 1-8 have the band kernel (7: switched off, as in 9 and 10)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
1 n=5200: band wide
2 n=5200: band wide
3 n=5200: band sorted wide unlList
4 n=5200: band sorted wide
5 n=255: band wide
5 n=256: band sorted wide unlList
6 n=5200 dev: band indirect wide
7 n=4096: latency wide
7 n=4097: sorted wide unlList
7 n=4096 dev: indirect wide
8 n=300: band wide
9 n=1: wide
10 n=10: -
11-plain n=5200: wide wideBoth
11-banded n=5200: wide
12 n=512: pipelined
12 n=513: -
12 n=10 dev: indirect
12-nopipe n=10: -
cross product: 24576 routes, 0 broken
"""


def test_route_rule_on_hand_picked_switches(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "msa_route_check")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "bbmap_amd", "csrc"), os.path.join(ROOT, "tests", "msa_route_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    # the last line: sorted and latency never together; a device count rules out sorted, latency and pipelined; unlList implies
    # sorted; latency implies no band kernel and a wide pass -- over 2^11 switch settings x host / device count x six launch sizes
    assert out == EXPECTED
