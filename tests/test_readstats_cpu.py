"""The read histograms without a device: the sequential restatement of align2.ReadStats (tests/readstats_check.py) against answers
worked out by hand, bbmap_amd.readstats' formatters against the restatement's writers, and the entry points' refusals.

The hand-worked records (qualities in brackets, rpos = index into the read):

A  bases ACGTTANCGA, q 30 31 32 33 34 35 2 37 38 39, plus strand, string  m S m I I m D D D N m m m
   walk: m r0, S r1, m r2, I r3, I r4, m r5, D D D at r6 (the read's N: the deletion counts once, at r6), N r6, m r7 r8 r9
   match {0,2,5,7,8,9}  sub {1}  ins {3,4}  del {6}  N {6}  other {}
   accuracy: match q 30 32 35 37 38 39; sub q 31; ins q 33 34 (T, T are defined); del: x = r6 is N (nothing), y = r5 is A -> q 35
   errors 1;  identity: good 6, N 1, bad 1 + 2 + 3 = 6 -> n = 1, good 7, bad 9, 7/16 = 0.4375 -> bin 43, 10 bases
   indel (no reversal, the first min(len, MAXLEN) = 10 symbols  m S m I I m D D D N): ins[2], del[3], del2[0]
   bases by position: A C G T T A N C G A;  length 10;  gc: A T T A A = 5, C G C G = 4 -> 4/9 = 0.444.. * 101 = 44.9 -> bin 44
B  the same read and string on the minus strand: the string is walked from its far end  m m m N D D D m I I m S m
   walk: m r0 r1 r2, N r3 (base T is defined: other), D D D at r4 (once), m r4, I r5, I r6 (base N: N, not ins), m r7, S r8, m r9
   match {0,1,2,4,7,9}  other {3}  del {4}  ins {5}  N {6}  sub {8}
   accuracy: match q 30 31 32 34 37 39; del: x = r4 (T) -> q 34, y = r3 (T) -> q 33; ins q 35 (r5 = A; r6 = N is not defined); sub q 38
   errors, identity and indel as A (none of them reverses the string)
C  bases ACNT, q 10 11 12 13, plus, string  m m D D m m: the read's N sits under the deletion
   match {0,1,3}  del {2}  N {2} (the m at r2 lies under a read N)
   accuracy: match q 10 11 12 13 (the m at r2 counts: only I and D look at the base); del: x = r2 is N, y = r1 is C -> q 11
   indel: the first 4 symbols  m m D D: the run is cut at the limit -> del[2], del2[0];  identity 4/6 -> bin 66;  errors 0
D  bases G, q 40, plus, string m: match {0}; accuracy match q 40; identity 1/1 -> bin 100, 1 base; gc 1/1 * 101 = 101 -> bin 100
P  the pair GGCA / ATGCAT: gc1 = 3/4, gc2 = 2/6 = 0.33333334f; 0.75 * 4 = 3, 0.33333334f * 6 = 2 (float32), 5 / 10 = 0.5,
   0.5 * 101 = 50.5 -> bin 50, gcMaxReadLen 10.  Single-ended the two reads fall in bins (int)(75.75) = 75 and (int)(33.67) = 33.
   An all-AT read has gc 0 -> bin 0."""
import ctypes as C

import numpy as np
import pytest

from bbmap_amd import _lib, build
from bbmap_amd import readstats as R
from tests import readstats_check as K

A_BASES, A_QUAL, A_MATCH = b"ACGTTANCGA", bytes([30, 31, 32, 33, 34, 35, 2, 37, 38, 39]), b"mSmIImDDDNmmm"


def _nz(a):
    """the non-zero entries of an array as {index tuple: value}"""
    return {tuple(int(x) for x in i) if len(i) > 1 else int(i[0]): int(a[tuple(i)]) for i in np.argwhere(a)}


def _one(bases, qual, strand, match, pairnum=0):
    rs = K.ReadStats()
    rs.add_read(bases, qual, True, strand, match, pairnum)
    rs.add_gc(bases, None)
    return rs


def _rows(rs, mate=0):
    names = ("match", "sub", "del", "ins", "N", "clip", "other")
    return {n: sorted(int(i) for i in np.flatnonzero(rs.match[k][mate])) for k, n in enumerate(names) if rs.match[k][mate].any()}


def test_record_a_plus_strand():
    rs = _one(A_BASES, A_QUAL, 0, A_MATCH)
    assert _rows(rs) == {"match": [0, 2, 5, 7, 8, 9], "sub": [1], "ins": [3, 4], "del": [6], "N": [6]}
    assert int(rs.match.sum()) == 11 and not rs.match[:, 1].any()
    assert _nz(rs.accuracy) == {(0, 30): 1, (0, 32): 1, (0, 35): 1, (0, 37): 1, (0, 38): 1, (0, 39): 1, (1, 31): 1, (2, 33): 1, (2, 34): 1, (3, 35): 1}
    assert _nz(rs.errorHist) == {1: 1} and _nz(rs.idHist) == {43: 1} and _nz(rs.idBaseHist) == {43: 10} and rs.idMaxReadLen == 10
    assert _nz(rs.insHist) == {2: 1} and _nz(rs.delHist) == {3: 1} and _nz(rs.delHist2) == {0: 1}
    slots = {"A": 1, "C": 2, "G": 3, "T": 4, "N": 0}
    assert _nz(rs.baseHist) == {(0, slots[chr(b)], i): 1 for i, b in enumerate(A_BASES)}
    assert _nz(rs.lengthHist) == {10: 1} and _nz(rs.gcHist) == {44: 1} and rs.gcMaxReadLen == 10
    assert _nz(rs.qualLength) == {(0, 9): 1} and _nz(rs.bqualHist) == {(0, i, q): 1 for i, q in enumerate(A_QUAL)}
    assert _nz(rs.qcountHist) == {(0, q): 1 for q in A_QUAL} and [int(x) for x in rs.qualSum[0][:10]] == list(A_QUAL)


def test_record_b_minus_strand():
    rs = _one(A_BASES, A_QUAL, 1, A_MATCH)
    assert _rows(rs) == {"match": [0, 1, 2, 4, 7, 9], "other": [3], "del": [4], "ins": [5], "N": [6], "sub": [8]}
    assert _nz(rs.accuracy) == {(0, 30): 1, (0, 31): 1, (0, 32): 1, (0, 34): 1, (0, 37): 1, (0, 39): 1, (1, 38): 1, (2, 35): 1, (3, 33): 1, (3, 34): 1}
    assert _nz(rs.errorHist) == {1: 1} and _nz(rs.idHist) == {43: 1} and _nz(rs.idBaseHist) == {43: 10}
    assert _nz(rs.insHist) == {2: 1} and _nz(rs.delHist) == {3: 1} and _nz(rs.delHist2) == {0: 1}


def test_record_c_n_under_a_deletion_and_the_cut_run():
    rs = _one(b"ACNT", bytes([10, 11, 12, 13]), 0, b"mmDDmm", pairnum=1)
    assert _rows(rs, 1) == {"match": [0, 1, 3], "del": [2], "N": [2]} and not rs.match[:, 0].any()
    assert _nz(rs.accuracy) == {(0, 10): 1, (0, 11): 1, (0, 12): 1, (0, 13): 1, (3, 11): 1}
    assert _nz(rs.delHist) == {2: 1} and _nz(rs.delHist2) == {0: 1} and not rs.insHist.any()
    assert _nz(rs.idHist) == {66: 1} and _nz(rs.idBaseHist) == {66: 4} and _nz(rs.errorHist) == {0: 1}
    assert _nz(rs.qualLength) == {(1, 3): 1}


def test_record_d_length_one():
    rs = _one(b"G", bytes([40]), 0, b"m")
    assert _rows(rs) == {"match": [0]} and _nz(rs.accuracy) == {(0, 40): 1}
    assert _nz(rs.idHist) == {100: 1} and _nz(rs.idBaseHist) == {100: 1} and _nz(rs.gcHist) == {100: 1}
    assert _nz(rs.lengthHist) == {1: 1} and _nz(rs.baseHist) == {(0, 3, 0): 1} and _nz(rs.qualLength) == {(0, 0): 1}


def test_gc_of_a_pair_and_of_its_reads():
    rs = K.ReadStats()
    rs.add_gc(b"GGCA", b"ATGCAT")
    assert _nz(rs.gcHist) == {50: 1} and rs.gcMaxReadLen == 10
    rs = K.ReadStats()
    for b in (b"GGCA", b"ATGCAT", b"ATTAnNAT"):
        rs.add_gc(b, None)
    assert _nz(rs.gcHist) == {75: 1, 33: 1, 0: 1} and rs.gcMaxReadLen == 8


def test_gates_and_deviations():
    rs = K.ReadStats()
    rs.add_read(b"ACGT", None, True, 0, b"mmmm", 0)              # no qualities: the quality-dependent histograms do not move
    assert not rs.qualLength.any() and not rs.accuracy.any() and int(rs.match.sum()) == 4
    rs = K.ReadStats()
    rs.add_read(b"ACGT", bytes([99, 126, 200, 98]), False, 0, None, 0)     # unmapped: quality, base and length histograms only
    assert not rs.match.any() and not rs.idHist.any() and not rs.errorHist.any() and int(rs.baseHist.sum()) == 4
    assert _nz(rs.qcountHist) == {(0, 99): 1, (0, 126): 2, (0, 98): 1}
    rs = K.ReadStats()
    rs.add_read(b"ACGT", bytes([99, 126, 200, 98]), True, 0, b"", 0)        # mapped without a string: as unmapped
    assert not rs.match.any() and not rs.idHist.any() and not rs.insHist.any()
    rs = K.ReadStats()
    rs.add_read(b"ACGT", bytes([99, 126, 200, 98]), True, 0, b"mmmmmm", 0)  # a string that overruns its read; q > 98 in bin 98
    assert int(rs.match.sum()) == 4 and _nz(rs.accuracy) == {(0, 98): 4}


# ------------------------------------------------------------------------------------------------ formatters against the writers
SYMS = np.frombuffer(b"mmmmmmmmmmmmmmmmSSDIXYNC", np.uint8)
BASES = np.frombuffer(b"ACGTACGTACGTACGTNacgtnU", np.uint8)


def random_batch(rng, n, max_len=90):
    reads, quals, fin, matches = [], [], np.zeros(n, [("mapped", "i4"), ("strand", "i4")]), []
    for r in range(n):
        ln = int(rng.integers(1, max_len))
        reads.append(BASES[rng.integers(0, len(BASES), ln)].tobytes())
        quals.append(rng.integers(0, 45, ln).astype(np.uint8).tobytes())
        fin[r] = (rng.random() < 0.9, int(rng.integers(0, 2)))
        matches.append(SYMS[rng.integers(0, len(SYMS), int(rng.integers(1, max_len + 10)))].tobytes() if rng.random() < 0.9 else None)
    return reads, quals, fin, matches


def hist_of(rs):
    """the restatement's arrays laid out as the library lays out its state"""
    h = R.ReadHist(rs.flags, np.zeros(R.state_words(rs.flags), np.int64))
    for name, a in rs.arrays().items():
        h.arrays[name][...] = np.asarray(a).reshape(h.arrays[name].shape)
    return h


def assert_qhist(h, rs, paired):
    """qhist: the log column as numbers to 1e-9 relative (the host's weighted sum against Java's running double sum), every other
    column as text"""
    got, want = h.qhist_lines(paired), rs.write_quality(paired)
    rows, wrows = h.qhist_rows(paired), rs.quality_rows(paired)
    assert len(got) == len(want) == len(rows) + 1 == len(wrows) + 1 and got[0] == want[0]
    per = 3 if "measured" in want[0] else 2
    for g, w, row, wrow in zip(got[1:], want[1:], rows, wrows):
        g, w = g.split("\t"), w.split("\t")
        assert len(g) == len(w) == 1 + per * len(row)
        assert [x for k, x in enumerate(g) if (k - 1) % per != 1 or k == 0] == [x for k, x in enumerate(w) if (k - 1) % per != 1 or k == 0], (g, w)
        for (_, log, _), (_, wlog, _) in zip(row, wrow):
            assert abs(log - wlog) <= 1e-9 * max(abs(log), abs(wlog)), (log, wlog)


def assert_text(h, rs, paired):
    f = rs.flags
    if f & R.RH_MATCH:
        assert h.mhist_lines(paired) == rs.write_match(paired)
    if f & R.RH_QUALITY:
        assert_qhist(h, rs, paired)
        assert h.bqhist_lines(paired) == rs.write_bquality(paired) and h.bqhist_overall_lines() == rs.write_bquality_overall()
        assert h.qchist_lines(paired) == rs.write_qcount(paired)
    if f & R.RH_BASE:
        assert h.bhist_lines(paired) == rs.write_base_content(paired)
    if f & R.RH_ACCURACY:
        assert h.qahist_lines() == rs.write_quality_accuracy()
    if f & R.RH_INDEL:
        assert h.indelhist_lines() == rs.write_indel()
    if f & R.RH_ERROR:
        assert h.ehist_lines() == rs.write_error()
    if f & R.RH_LENGTH:
        assert h.lhist_lines() == rs.write_length()
    if f & R.RH_GC:
        assert h.gchist_lines() == rs.write_gc() and h.gchist_lines(False) == rs.write_gc(False)
    if f & R.RH_IDENTITY:
        assert h.idhist_lines() == rs.write_identity() and h.idhist_lines(False) == rs.write_identity(False)


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("flags", [R.RH_ALL, R.RH_ALL & ~R.RH_MATCH])
def test_formatters_reproduce_the_writers(paired, flags):
    build.build()
    rs = K.ReadStats(flags)
    rs.add_batch(*random_batch(np.random.default_rng(7 + paired), 400), paired)
    h = hist_of(rs)
    assert_text(h, rs, paired)
    lines = h.qhist_lines(paired)
    assert lines[0].count("measured") == ((2 if paired else 1) if flags & R.RH_MATCH else 0) and len(lines) > 50
    assert h.gc_max_read_len == rs.gcMaxReadLen and h.id_max_read_len == rs.idMaxReadLen


def test_formatters_on_an_empty_state_and_on_hand_text():
    build.build()
    rs = K.ReadStats()
    assert_text(hist_of(rs), rs, True)
    assert rs.write_quality_accuracy()[:2] == ["#Deviation\tNaN", "#DeviationSub\tNaN"] and rs.write_match(True) == [rs.write_match(True)[0]]
    rs = _one(A_BASES, A_QUAL, 0, A_MATCH)
    h = hist_of(rs)
    assert_text(h, rs, False)
    assert h.mhist_lines(False)[1] == "1\t1.00000\t0.00000\t0.00000\t0.00000\t0.00000\t0.00000"
    assert h.mhist_lines(False)[7] == "7\t0.00000\t0.00000\t1.00000\t0.00000\t1.00000\t0.00000"         # the deletion column is not in the sum
    assert h.indelhist_lines() == ["#Length\tDeletions\tInsertions", "2\t0\t1", "3\t1\t0"]
    assert h.ehist_lines() == ["#Errors\tCount", "1\t1"] and h.lhist_lines() == ["#Length\tCount", "10\t1"]
    assert h.idhist_lines(False)[-1] == "43.0\t1\t10" and h.gchist_lines(False)[-1] == "44.0\t1"
    assert h.qhist_lines(False)[1] == "1\t30.000\t30.000\t60.000" and h.bhist_lines(False)[7] == "6\t0.00000\t0.00000\t0.00000\t0.00000\t1.00000"
    assert K.jfmt(0.03125, 4) == R.jfmt(0.03125, 4) == "0.0313"        # HALF_UP on the exact value, where Python's % gives 0.0312
    assert [float(x) for x in R.PROB_ERROR] == [float(x) for x in K.PROB_ERROR] and float(R.PROB_ERROR[0]) == float(np.float32(0.8))


# ------------------------------------------------------------------------------------------------ sizes and refusals (no device)
def _raw():
    build.build()
    L = C.CDLL(_lib.SO_PATH)
    L.bbmap_last_error.restype = C.c_char_p
    L.bbpipe_read_hist_bytes.restype = C.c_int64
    return L


def test_state_sizes():
    L = _raw()
    size = {g: 0 for g in R.RH_GROUPS}
    group = {"match": R.RH_MATCH, "qual_length": R.RH_QUALITY, "bqual": R.RH_QUALITY, "qcount": R.RH_QUALITY, "base": R.RH_BASE,
             "accuracy": R.RH_ACCURACY, "ins": R.RH_INDEL, "del": R.RH_INDEL, "del2": R.RH_INDEL, "error": R.RH_ERROR, "length": R.RH_LENGTH,
             "gc": R.RH_GC, "identity": R.RH_IDENTITY}
    for name, shape in R.SHAPES:
        size[group[name]] += 8 * int(np.prod(shape))
    assert size[R.RH_MATCH] == 8 * 7 * 2 * 6000 and size[R.RH_GC] == 8 * 102 and size[R.RH_IDENTITY] == 8 * 203
    for flags in list(R.RH_GROUPS) + [R.RH_ALL, R.RH_MATCH | R.RH_GC, 0]:
        assert L.bbpipe_read_hist_bytes(C.c_int32(flags)) == sum(v for g, v in size.items() if flags & g)
    assert L.bbpipe_read_hist_bytes(C.c_int32(512)) == -2 and L.bbmap_last_error() == b"bbpipe_read_hist_bytes: unknown flag bits"
    # the arrays lie in the order of the view's pointers, the selected ones back to back
    h = R.ReadHist(R.RH_MATCH | R.RH_GC | R.RH_IDENTITY, np.arange(7 * 2 * 6000 + 102 + 203, dtype=np.int64))
    assert int(h.match[0][0][0]) == 0 and int(h.gc[0]) == 84000 and int(h.identity[0]) == 84102 and h.bqual is None and h.del_ is None


NULL, I32, I64 = None, C.c_int32, C.c_int64
REJECTED = [
    ("bbpipe_read_hist_add_device", (NULL, I64(-1), I32(0), I32(1), NULL, NULL, NULL, NULL, NULL, NULL), b"bbpipe_read_hist_add_device: bad argument"),
    ("bbpipe_read_hist_add_device", (NULL, I64(3), I32(1), I32(1), NULL, NULL, NULL, NULL, NULL, NULL), b"bbpipe_read_hist_add_device: bad argument"),
    ("bbpipe_read_hist_add_device", (NULL, I64(2), I32(1), I32(1024), NULL, NULL, NULL, NULL, NULL, NULL), b"bbpipe_read_hist_add_device: unknown flag bits"),
    ("bbpipe_read_hist_add_device", (NULL, I64(2), I32(1), I32(511), NULL, NULL, NULL, NULL, NULL, NULL), b"bbpipe_read_hist_add_device: null buffer"),
    ("bbpipe_read_hist_view", (I32(1), NULL, NULL), b"bbpipe_read_hist_view: null argument"),
    ("bbpipe_read_hist_view", (I32(-1), NULL, C.byref(R.bbmap_readhist_view())), b"bbpipe_read_hist_view: unknown flag bits"),
    ("bbmap_hist_enable", (NULL, I32(1)), b"bbmap_hist_enable: null context"),
    ("bbmap_add_read_hist", (NULL, NULL, NULL), b"bbmap_add_read_hist: null context"),
    ("bbmap_get_read_hist_view", (NULL, NULL), b"bbmap_get_read_hist_view: null argument"),
    ("bbmap_get_read_hist", (NULL, NULL, I64(0), NULL), b"bbmap_get_read_hist: null context"),
    ("bbmap_reset_read_hist", (NULL,), b"bbmap_reset_read_hist: null context"),
]


@pytest.mark.parametrize("case", range(len(REJECTED)), ids=["%02d-%s" % (i, c[0]) for i, c in enumerate(REJECTED)])
def test_rejected_arguments(case):
    name, args, msg = REJECTED[case]
    L = _raw()
    assert getattr(L, name)(*args) == -2
    assert L.bbmap_last_error() == msg
