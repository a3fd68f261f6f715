"""The merge stage without a device: the host forms bbmerge_overlap_batch and bbmerge_join_batch against the oracle's restatement of
BBMerge's natives (tests/merge_problems.py) and against the restatement of Read.joinRead (tests/merge_check.py), the answers worked
out by hand in tests/test_jni_shim.py through the batch form, joins written out by hand, the records' layout, from_flags, and every
rejected argument.  Everything is compared exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bbmap_amd import _lib, build
from bbmap_amd import merge as M
from tests import merge_check as K
from tests import merge_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build()


# ------------------------------------------------------------------------------------------------ the inputs themselves
@pytest.mark.parametrize("name", ["defaults", "quality-only"])
def test_problem_set_holds_every_class(name):
    """A condition on the inputs, judged on the oracle's answers alone: merged / not merged, each unambiguous and ambiguous, for the
    flat form (defaults) and for the quality form (quality-only)."""
    exp = P.expected_for(name)
    assert set(exp["info"]) == {M.INFO_FLAT if name == "defaults" else M.INFO_QUALITY}
    counts = P.classes(exp)
    print(name, counts)
    assert all(c > 0 for c in counts), counts


# ------------------------------------------------------------------------------------------------ overlap: host form against the oracle
@pytest.mark.parametrize("name", sorted(P.CONFIGS))
def test_host_overlap_equals_the_oracle(name):
    pairs, (r1, r2, bases, quality) = P.problem_set()
    got = M.overlap_batch(r1, r2, bases, quality, P.config(P.CONFIGS[name]))
    exp = P.expected_for(name)
    diff = np.flatnonzero(got != exp)
    assert diff.size == 0, (diff[:5], got[diff[:5]], exp[diff[:5]])
    if name == "quality-then-flat":
        assert {M.INFO_QUALITY, M.INFO_QUALITY | M.INFO_FLAT} == set(exp["info"])       # both outcomes of the composition occur


def test_host_overlap_without_qualities_runs_the_flat_form_whatever_the_flags():
    pairs, (r1, r2, bases, quality) = P.problem_set()
    got = M.overlap_batch(r1[:300], r2[:300], bases, None, P.config(P.CONFIGS["quality-only"]))
    assert (got == P.expected_for("defaults")[:300]).all()


HAND = (4, 4, 10, 10, 0.4, 2.0, 0.5, 1.0, 1.0)


@pytest.mark.parametrize("use_quality", [0, 1])
def test_known_answers_derived_by_hand_through_the_batch_form(use_quality):
    """tests/test_jni_shim.py::test_bbmerge_known_answers_derived_by_hand, whose docstring holds the traces: a = AAAACGGCAC against
    b = CGGCACTTTT, CGTCACTTTT, TTTTTTTTTT under (4, 4, 10, 10, .4, 2, .5, 1, 1) gives (14, 0, 0), (14, 1, 0), (-1, 10, 0), flat and
    with every quality 40 (probCorrect[40] = 1, the same traces)."""
    a = b"AAAACGGCAC"
    bs = [b"CGGCACTTTT", b"CGTCACTTTT", b"TTTTTTTTTT"]
    q40 = np.full(10, 40, np.uint8)
    r1, r2, bases, quality = M.pack_pairs([a] * 3, [P.revcomp(b) for b in bs], [q40] * 3, [q40] * 3)
    got = M.overlap_batch(r1, r2, bases, quality, P.config(HAND + (use_quality, 0)))
    info = M.INFO_QUALITY if use_quality else M.INFO_FLAT
    assert got.tolist() == [(14, 0, 0, info), (14, 1, 0, info), (-1, 10, 0, info)]


def test_a_pair_outside_the_limits_is_reported_and_its_neighbours_are_not_disturbed():
    pairs = P.make_pairs(4, 3)
    s1, s2, q1, q2 = P.hand_over(pairs)
    long_ = b"ACGT" * 128 + b"A"                                        # 513 bases
    s1b, q1b = [s1[0], long_, s1[1], s1[2], s1[3]], [q1[0], np.full(513, 30, np.uint8), q1[1], q1[2].copy(), q1[3]]
    s2b, q2b = [s2[0], s2[0], s2[1], s2[2], s2[3]], [q2[0], q2[0], q2[1], q2[2], q2[3]]
    q1b[3][5] = 71                                                      # outside probCorrect
    cfg = P.config(P.CONFIGS["quality-then-flat"])
    got = M.overlap_batch(*M.pack_pairs(s1b, s2b, q1b, q2b), cfg)
    exp = P.expected_records(pairs, P.CONFIGS["quality-then-flat"])
    assert got[[0, 2, 4]].tolist() == exp[[0, 1, 3]].tolist()
    assert got[[1, 3]].tolist() == [(-1, 0, 0, M.INFO_SKIPPED)] * 2
    # where the quality form does not run no quality is read, and a quality of 71 is no obstacle
    flat = M.overlap_batch(*M.pack_pairs(s1b, s2b, q1b, q2b), P.config(P.CONFIGS["defaults"]))
    assert flat[3].tolist() == P.expected_records(pairs, P.CONFIGS["defaults"])[2].tolist() and flat[1]["info"] == M.INFO_SKIPPED


# ------------------------------------------------------------------------------------------------ join
# (a, b in overlap orientation, qa, qb, insert, expected bases, expected qualities), maxMergeQuality 41
HAND_JOINS = [
    (b"ACGT", b"ACGT", [40, 40, 10, 3], [40, 20, 30, 2], 4, b"ACGT", [41, 41, 32, 3]),
    (b"ACGT", b"TCAA", [30, 10, 20, 20], [10, 10, 35, 20], 4, b"ACAN", [20, 12, 15, 0]),
    (b"NCNT", b"ANNT", [2, 30, 2, 30], [25, 7, 9, 30], 4, b"ACNT", [25, 30, 9, 37]),
    (b"ACGTGG", b"TTACGT", [10] * 6, [20] * 6, 4, b"ACGT", [22] * 4),
    (b"ACG", b"GTT", [30, 30, 12], [20, 5, 6], 5, b"ACGTT", [30, 30, 23, 5, 6]),
]
# (a, b, insert, expected bases) for reads without qualities
HAND_JOINS_NOQ = [(b"ACNT", b"AGTN", 4, b"AGTT"), (b"ACG", b"GTT", 5, b"ACGTT"), (b"AC", b"NC", 2, b"NC"), (b"ACGTGG", b"TTACGT", 4, b"ACGT")]


def hand_join_inputs():
    s1, s2, q1, q2 = P.hand_over([(a, b, np.array(qa, np.uint8), np.array(qb, np.uint8)) for a, b, qa, qb, _, _, _ in HAND_JOINS])
    return M.pack_pairs(s1, s2, q1, q2), np.array([j[4] for j in HAND_JOINS], np.int32)


def hand_join_inputs_noq():
    return M.pack_pairs([j[0] for j in HAND_JOINS_NOQ], [P.revcomp(j[1]) for j in HAND_JOINS_NOQ]), np.array([j[2] for j in HAND_JOINS_NOQ], np.int32)


def slot(merged, buf, i):
    off, ln = int(merged["bases_off"][i]), int(merged["len"][i])
    return buf[off:off + ln]


def test_host_join_of_pairs_written_out_by_hand():
    """Read.joinRead(a, b, insert) with MAX_MERGE_QUALITY 41; b is aligned to the right end of the insert, a to the left.
      ACGT q 40 40 10 3 + ACGT q 40 20 30 2, insert 4: equal bases, max + min / 4 = 50, 45, 32, 3 -> 41, 41 (saturated), 32, 3.
      ACGT q 30 10 20 20 + TCAA q 10 10 35 20, insert 4: A(30) beats T(10) with 30 - 10 = 20; C = C: 10 + 10 / 4 = 12; A(35) beats G(20)
        with 15; T(20) against A(20) is a tie: N with quality 0.
      NCNT q 2 30 2 30 + ANNT q 25 7 9 30, insert 4: N in a takes b's A and 25; N in b leaves C and 30; N against N takes b's N and 9;
        T = T: 30 + 30 / 4 = 37.
      ACGTGG + TTACGT, insert 4 < alen: the result is a's first four bases against b's last four, ACGT = ACGT, 20 + 10 / 4 = 22 each.
      ACG q 30 30 12 + GTT q 20 5 6, insert 5 = alen + blen - 1: one column overlaps, G = G: 20 + 12 / 4 = 23; b's TT fill the rest.
    Without qualities (:2806-2818): ACNT + AGTN, insert 4: A = A; C against G keeps the larger byte G; N takes T; T against N keeps
      the larger byte T.  AC + NC, insert 2: A against N keeps the larger byte N.  The other two as above."""
    (r1, r2, bases, quality), ins = hand_join_inputs()
    merged, ob, oq = M.join_batch(r1, r2, bases, quality, ins)
    for i, (a, b, qa, qb, insert, eb, eq) in enumerate(HAND_JOINS):
        assert slot(merged, ob, i).tobytes() == eb and slot(merged, oq, i).tolist() == eq, i
        kb, kq = K.join_read(a, b, insert, qa, qb)                      # the checker agrees with the hand
        assert kb == eb and kq.tolist() == eq, i
    (r1, r2, bases, _), ins = hand_join_inputs_noq()
    merged, ob, oq = M.join_batch(r1, r2, bases, None, ins)
    assert oq is None
    for i, (a, b, insert, eb) in enumerate(HAND_JOINS_NOQ):
        assert slot(merged, ob, i).tobytes() == eb, i
        assert K.join_read(a, b, insert) == (eb, None)


def expected_joins(pairs, inserts, with_quality, maxq=41):
    return [K.join_read(a, b, int(ins), qa if with_quality else None, qb if with_quality else None, maxq) for (a, b, qa, qb), ins in zip(pairs, inserts)]


def check_joins(pairs, inserts, with_quality, merged, ob, oq, maxq=41):
    for i, e in enumerate(expected_joins(pairs, inserts, with_quality, maxq)):
        if e is None:
            assert merged["len"][i] == 0, i
            continue
        assert slot(merged, ob, i).tobytes() == e[0], i
        if with_quality:
            assert (slot(merged, oq, i) == e[1]).all(), i


def join_inserts(n):
    """the oracle's inserts by the usual rule, and a few inserts no search would give: <= 0, below either length, alen + blen - 1 and
    the no-overlap sizes alen + blen and beyond"""
    pairs = P.problem_set()[0][:n]
    ins = M.usual_inserts(P.expected_for("defaults")[:n])
    for i, (a, b, _, _) in enumerate(pairs):
        if i % 10 == 3:
            ins[i] = (-1, 0, 1, 7, len(a) + len(b) - 1, len(a) + len(b), len(a) + len(b) + 5, min(len(a), len(b)) - 1)[(i // 10) % 8]
    return pairs, ins


@pytest.mark.parametrize("with_quality, maxq", [(True, 41), (True, 30), (False, 41)])
def test_host_join_equals_the_restatement_of_joinread(with_quality, maxq):
    pairs, ins = join_inserts(1200)
    r1, r2, bases, quality = P.problem_set()[1]
    merged, ob, oq = M.join_batch(r1[:1200], r2[:1200], bases, quality if with_quality else None, ins, cfg=M.default_config(maxMergeQuality=maxq))
    assert (merged["len"] > 0).sum() > 300 and (merged["len"] == 0).sum() > 300
    check_joins(pairs, ins, with_quality, merged, ob, oq, maxq)


def test_host_join_writes_nothing_outside_the_joined_bytes():
    pairs, ins = join_inserts(200)
    r1, r2, bases, quality = P.problem_set()[1]
    merged, total = M.slots_for(r1[:200], r2[:200])
    ob, oq = np.full(total, 0xA5, np.uint8), np.full(total, 0xA5, np.uint8)
    M.join_batch(r1[:200], r2[:200], bases, quality, ins, merged, ob, oq)
    written = np.zeros(total, bool)
    for off, ln in zip(merged["bases_off"], merged["len"]):
        written[off:off + ln] = True
    assert (ob[~written] == 0xA5).all() and (oq[~written] == 0xA5).all() and written.sum() == merged["len"].sum()
    assert (merged["keys_off"] == 0).all() and (merged["nkeys"] == 0).all()


# ------------------------------------------------------------------------------------------------ layout, flags, refusals
def test_the_two_records_have_the_compiler_s_layout(tmp_path):
    """sizeof and offsetof as the host C compiler lays the header's structs out (the method of
    tests/test_abi.py::test_every_mirrored_record_has_the_compiler_s_layout)"""
    mirrors = [("bbmerge_config", M.bbmerge_config), ("bbmerge_rec", M.REC_DTYPE)]
    layout = lambda m: ((m.itemsize, {n: m.fields[n][1] for n in m.names}) if isinstance(m, np.dtype) else      # noqa: E731
                        (C.sizeof(m), {n: getattr(m, n).offset for n, *_ in m._fields_}))
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "bbmap_amd.h"', "int main(void) {"]
    for i, (name, mirror) in enumerate(mirrors):
        src.append('    printf("%d sizeof %%zu\\n", sizeof(%s));' % (i, name))
        for f in layout(mirror)[1]:
            src.append('    printf("%d %s %%zu\\n", offsetof(%s, %s));' % (i, f, name, f))
    src += ['    printf("9 max %d\\n", BBMERGE_MAX_READ_LEN);', "    return 0;", "}", ""]
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", exe], check=True)
    got = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        i, f, v = line.split()
        got.setdefault(int(i), {})[f] = int(v)
    for i, (name, mirror) in enumerate(mirrors):
        size, offsets = layout(mirror)
        assert dict(offsets, sizeof=size) == got[i], name
    assert got[0]["sizeof"] == 48 and got[1]["sizeof"] == 16 and got[9]["max"] == M.MAX_READ_LEN


def fields(cfg):
    return tuple(getattr(cfg, n) for n, _ in M.bbmerge_config._fields_)


def test_default_config_and_from_flags():
    """BBMerge.java:605-611 by hand, with MIN_OVERLAPPING_BASES 11, MIN_OVERLAPPING_BASES_0 8, the ratio reduction 3, minInsert 35,
    minInsert0 -1:
      no flag: minInsert = max(35, 11) = 35; minInsert0 = min(35, max((int)26.25, 5, 8)) = 26; overlaps 8 - 3, 11 - 3.
      mininsert=50: minInsert0 = min(35, max(37, 5, 8)) = 35.                mininsert=20: minInsert0 = max(15, 5, 8) = 15.
      minoverlap=30 mininsert=12: minInsert = max(12, 30) = 30, minInsert0 = max(22, 5, 8) = 22, minOverlap 27.
      minoverlap0=25 mininsert=20: minInsert0 = min(35, max(15, 5, 25)) = 25, then min(20, 25) = 20; minOverlap0 22.
      mininsert0=40: given (>= 1), so only the last line applies: min(35, 40) = 35.      mininsert0=10: 10.
      ratiominoverlapreduction=0: overlaps 8, 11."""
    f32 = lambda x: float(np.float32(x))        # noqa: E731
    tail = (f32(0.09), 5.5, f32(0.55), f32(0.95), f32(0.95), 0, 1, 41)
    assert fields(M.default_config()) == (5, 8, 26, 35) + tail
    assert fields(M.from_flags()) == (5, 8, 26, 35) + tail
    assert fields(M.from_flags(mininsert=50))[:4] == (5, 8, 35, 50)
    assert fields(M.from_flags(mininsert=20))[:4] == (5, 8, 15, 20)
    assert fields(M.from_flags(minoverlap=30, mininsert=12))[:4] == (5, 27, 22, 30)
    assert fields(M.from_flags(minoverlap0=25, mininsert=20))[:4] == (22, 8, 20, 20)
    assert fields(M.from_flags(mininsert0=40))[:4] == (5, 8, 35, 35)
    assert fields(M.from_flags(mininsert0=10))[:4] == (5, 8, 10, 35)
    assert fields(M.from_flags(ratiominoverlapreduction=0))[:4] == (8, 11, 26, 35)
    got = M.from_flags(maxratio="0.075", ratiomargin=2, ratiooffset=0.5, maxq=30, usequality="t", overlapwithoutquality="f")
    assert fields(got)[4:] == (f32(0.075), 2.0, 0.5, f32(0.95), f32(0.95), 1, 0, 30)
    assert M.from_flags(overlapusingquality=True).useQuality == 1
    with pytest.raises(ValueError):
        M.from_flags(usequality=True, overlapusingquality=True)


VP, I64 = C.c_void_p, C.c_int64
BAD_CONFIG = b": bad config (no NaN, ratioMargin >= 1, gIncr and bIncr >= 0, minInsert0 and minInsert >= 0, maxMergeQuality 0..127)"
OVERLAPS = ("bbmerge_overlap_batch", "bbmerge_overlap_batch_device")
JOINS = ("bbmerge_join_batch", "bbmerge_join_batch_device")


def _call(name, cfg, n, nulls=()):
    """the entry point with every buffer a valid host address except those named in `nulls`: each refusal below comes before the
    first HIP call and before any buffer is read, so the device forms can be asked without a device"""
    L = _lib.load()
    buf = np.zeros(64, np.uint8)
    device = name.endswith("_device")
    names = ["reads1", "reads2", "bases", "quality"] + (["recs"] if "overlap" in name else ["insert", "merged", "out_bases", "out_quality"])
    args = [None if cfg is None else C.byref(cfg)] + ([None] if device else []) + [n] + [None if k in nulls else buf.ctypes.data for k in names]
    rc = getattr(L, name)(*args)
    return rc, L.bbmap_last_error()


@pytest.mark.parametrize("name", OVERLAPS + JOINS)
def test_rejected_arguments_keep_their_code_and_message(name):
    who = name.encode()
    good = M.default_config()
    assert _call(name, None, 1) == (-2, who + b": null config")
    assert _call(name, good, -1) == (-2, who + b": bad pair count")
    for bad in (dict(maxRatio=float("nan")), dict(ratioOffset=float("nan")), dict(gIncr=float("nan")), dict(ratioMargin=0.99), dict(gIncr=-0.5),
                dict(bIncr=-1.0), dict(minInsert=-1), dict(minInsert0=-1), dict(maxMergeQuality=128), dict(maxMergeQuality=-1)):
        assert _call(name, M.default_config(**bad), 1) == (-2, who + BAD_CONFIG), bad
    for k in ("reads1", "reads2", "bases", "recs") if name in OVERLAPS else ("reads1", "reads2", "bases", "insert", "merged", "out_bases"):
        assert _call(name, good, 1, nulls={k}) == (-2, who + b": null buffer"), k
    if name in JOINS:
        assert _call(name, good, 1, nulls={"out_quality"}) == (-2, who + b": null buffer")      # qualities in, nowhere to put them
    assert _call(name, good, 0, nulls={"reads1", "reads2", "bases", "quality", "recs", "insert", "merged", "out_bases", "out_quality"})[0] == 0


def test_default_config_refuses_null():
    L = _lib.load()
    assert L.bbmerge_default_config(None) == -2 and L.bbmap_last_error() == b"bbmerge_default_config: null argument"


def test_min_overlap0_above_min_overlap_is_clamped_not_refused():
    pairs, (r1, r2, bases, quality) = P.problem_set()
    values = (20, 8, 26, 35, 0.09, 5.5, 0.55, 0.95, 0.95, 1, 1)
    got = M.overlap_batch(r1[:400], r2[:400], bases, quality, P.config(values))
    assert (got == P.expected_records(pairs[:400], values)).all()


# ------------------------------------------------------------------------------------------------ what the GPU property test relies on
def fragments(n, seed):
    """[(frag, r1, r2 as sequenced)] for fragments of 40..280 bases cut from a random sequence, reads of 100 and of 150"""
    rng = np.random.default_rng(seed)
    genome = P.ACGT[rng.integers(0, 4, 20000)].tobytes()
    out = []
    for i in range(n):
        ln = int(rng.integers(40, 281))
        at = int(rng.integers(0, len(genome) - ln))
        frag = genome[at:at + ln]
        L = (100, 150)[i % 2]
        out.append((frag, frag[:L], P.revcomp(frag)[:L]))
    return out


def check_fragments(frs, recs, merged_bases):
    """What an error-free pair must give.  The mates of a fragment of F bases read to L overlap in len(m1) + len(m2) - F columns (2L - F, and
    all F of both for F <= L).  The flat form accepts an insert unambiguously only with good = 0.95 * columns >= minOverlap = 8, that is from 9 columns
    on; with 6..8 columns it returns ambiguous (bad == 0, good between minOverlap0 and minOverlap), and with fewer, or with no overlap
    at all (L = 100 and F > 200), the true insert is not among those it tests.  So: an unambiguous pair with at least 9 overlapping
    columns comes back as its fragment, and an unambiguous pair with fewer comes back unmerged, not as something else.
    merged_bases[i]: bytes or None."""
    for i, (frag, m1, m2) in enumerate(frs):
        if recs["ambig"][i]:
            continue
        if len(m1) + len(m2) - len(frag) >= 9:
            assert merged_bases[i] == frag, i
        else:
            assert merged_bases[i] is None, i


def test_error_free_fragments_merge_unambiguously_on_the_host():
    """The share the GPU property test relies on, from records that equal the oracle's: of 500 error-free pairs at least 95 % are
    unambiguous (here: all 500), and check_fragments holds for them."""
    frs = fragments(500, 8)
    q = [np.full(len(f[1]), 35, np.uint8) for f in frs]
    r1, r2, bases, quality = M.pack_pairs([f[1] for f in frs], [f[2] for f in frs], q, q)
    recs = M.overlap_batch(r1, r2, bases, quality)
    exp = P.expected_records([(f[1], P.revcomp(f[2]), None, None) for f in frs], P.CONFIGS["defaults"], with_quality=False)
    assert (recs == exp).all()
    ok = recs["ambig"] == 0
    print("unambiguous: %d of %d" % (ok.sum(), len(frs)))
    assert ok.mean() >= 0.95
    assert sum(len(f[1]) + len(f[2]) - len(f[0]) < 9 for f in frs) > 20 and sum(len(f[0]) < 100 for f in frs) > 50      # both kinds occur
    merged, ob, oq = M.join_batch(r1, r2, bases, quality, M.usual_inserts(recs))
    check_fragments(frs, recs, [slot(merged, ob, i).tobytes() if merged["len"][i] else None for i in range(len(frs))])
