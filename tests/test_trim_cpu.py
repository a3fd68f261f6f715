"""The trim stage's host form (bbtrim_batch) against the restatement of align2.TrimRead (tests/trim_check.py), and both against
(left, right) pairs derived by hand from TrimRead.java.  Exact integers throughout.  The restatement and the library come from the
same reading of the Java source, so the hand-derived cases below are literals: a mistake shared by both would still miss them.

How each literal follows (trimq = 10, so avgErrorRate = PROB_ERROR[10] = 0.1; PROB_ERROR[2] = 0.631, PROB_ERROR[30] = 0.001):
  1  quals 2 2 30 30 30 2: the score is reset at bases 0, 1, climbs .099 / .198 / .297 over bases 2..4 (maxLoc 4, maxCount 3) and is
     reset at base 5: left 4 - 3 + 1 = 2, right 6 - 4 - 1 = 1.  minLength 4: maxTrim 2, the excess 1 comes off the left -> (1, 1);
     minLength 6: maxTrim 0 -> (0, 0); minLength 9: maxTrim -3 -> (0, 0).
  2  five bases of quality 2: nothing scores -> left 0, right 5; minLength 2 leaves maxTrim 3 -> right 3.  Left only: a = 0, b = 0 -> null.
  3  ANAA, quality 30: the N costs max(min(.11, 1), .75) = .75 and resets the score; bases 2, 3 reach .198 > .099 -> left 2, right 0.
  4  30 30 2 30 30: both runs reach the same float .198 with count 2; `count > maxCount` is false for the later one -> maxLoc 1.
  5  window 4, thresh 40: the window sums are 80, 62, 44, 26: the fourth (j = 2) is below -> 8 - 2 - 1 = 5.
  6  interval 2: from the left the last bad base before two good ones is base 2 -> 3; from the right it is base 6 -> 8 - 6 = 2."""
import ctypes as C
import itertools

import numpy as np
import pytest

from bbmap_amd import _lib
from bbmap_amd import keys as K
from bbmap_amd import trim as T
from bbmap_amd.index import READ_DTYPE
from tests import trim_check as TC

OPT, WIN, INT = T.MODE_OPTIMAL, T.MODE_WINDOW, T.MODE_INTERVAL
LENGTHS = [1, 2, 3, 63, 64, 65, 150, 151, 600]
TRIMQS = [0, 1, 6, 10, 20, 41]
SIDES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def cfg(mode=OPT, left=1, right=1, trimq=10, minLength=0, **kw):
    return T.default_config(mode=mode, trimLeft=left, trimRight=right, trimq=trimq, minLength=minLength, **kw)


def pack(reads, quals=None):
    """reads laid out back to back: (READ_DTYPE records, bases blob, quality blob or None)"""
    recs = np.zeros(len(reads), READ_DTYPE)
    lens = np.array([len(r) for r in reads], np.int64)
    recs["len"] = lens
    recs["bases_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(reads) else 0
    blob = np.concatenate([np.frombuffer(bytes(r), np.uint8) for r in reads] + [np.zeros(1, np.uint8)])
    qblob = None if quals is None else np.concatenate([np.frombuffer(bytes(q), np.uint8) for q in quals] + [np.zeros(1, np.uint8)])
    return recs, blob, qblob


def expected(reads, quals, c):
    cc = TC.Config.of(c)
    return [TC.trim(r, None if quals is None else quals[i], cc) for i, r in enumerate(reads)]


def check_batch(reads, quals, c):
    """bbtrim_batch == the restatement, and the output records are the input's, moved"""
    recs, blob, qblob = pack(reads, quals)
    out, trims = T.trim_batch(recs, blob, qblob, c)
    want = expected(reads, quals, c)
    got = [(int(t["left"]), int(t["right"])) for t in trims]
    assert got == want, [(i, got[i], want[i]) for i in range(len(got)) if got[i] != want[i]][:5]
    assert np.array_equal(out["bases_off"], recs["bases_off"] + trims["left"]) and np.array_equal(out["len"], recs["len"] - trims["left"] - trims["right"])
    assert not out["keys_off"].any() and not out["nkeys"].any()
    return got


def case_reads(seed=5):
    """[(bases, quality)]: every length x 0 % / 5 % / 100 % N x qualities over 0..41 and over 0..126; an N has quality 0 in the first
    set (as stream.Read leaves it) and any quality in the second"""
    rng = np.random.default_rng(seed)
    out = []
    for n, pn, qmax in itertools.product(LENGTHS, (0.0, 0.05, 1.0), (41, 126)):
        b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
        b[rng.random(n) < pn] = ord("N")
        # runs of good and bad qualities, so that every mode finds something to trim and something to keep
        q = np.where(rng.random(n) < 0.5, rng.integers(0, 12, n), rng.integers(0, qmax + 1, n)).astype(np.uint8)
        edge = int(rng.integers(0, n // 3 + 1))
        q[:edge] = rng.integers(0, 8, edge)
        q[n - edge:] = rng.integers(0, 8, edge)
        if qmax == 41:
            q[b == ord("N")] = 0
        out.append((b.tobytes(), q.tobytes()))
    return out


# ------------------------------------------------------------------------------------------------ hand-derived literals
LITERALS = [
    ("1 minLength 0", cfg(minLength=0), b"ACGTAC", [2, 2, 30, 30, 30, 2], (2, 1)),
    ("1 minLength 4: excess off the left first", cfg(minLength=4), b"ACGTAC", [2, 2, 30, 30, 30, 2], (1, 1)),
    ("1 minLength 6", cfg(minLength=6), b"ACGTAC", [2, 2, 30, 30, 30, 2], (0, 0)),
    ("1 minLength 9 > len", cfg(minLength=9), b"ACGTAC", [2, 2, 30, 30, 30, 2], (0, 0)),
    ("2 both", cfg(minLength=2), b"ACGTA", [2] * 5, (0, 3)),
    ("2 right only", cfg(left=0, minLength=2), b"ACGTA", [2] * 5, (0, 3)),
    ("2 left only", cfg(right=0, minLength=2), b"ACGTA", [2] * 5, (0, 0)),
    ("3 N costs .75", cfg(), b"ANAA", [30] * 4, (2, 0)),
    ("4 tie keeps the earlier run", cfg(), b"ACGTA", [30, 30, 2, 30, 30], (0, 3)),
    ("5 window", cfg(WIN, left=0), b"ACGTACGT", [20, 20, 20, 20, 2, 2, 2, 2], (0, 5)),
    ("5 window, trimLeft set", cfg(WIN, left=1), b"ACGTACGT", [20, 20, 20, 20, 2, 2, 2, 2], (0, 5)),
    ("6 interval", cfg(INT), b"ACGTACGT", [2, 30, 2, 30, 30, 30, 2, 30], (3, 2)),
    # the window mode's own fallback for a read shorter than the window (:351): testRightN for trimq 0, nothing for trimq > 0
    ("window fallback trimq 0", cfg(WIN, trimq=0), b"ANN", [30, 30, 30], (0, 2)),
    ("window fallback trimq 1", cfg(WIN, trimq=1), b"ANN", [30, 30, 30], (0, 0)),
]


@pytest.mark.parametrize("case", LITERALS, ids=[c[0] for c in LITERALS])
def test_hand_derived_cases(case):
    _, c, bases, quals, want = case
    assert TC.trim(bases, bytes(quals), TC.Config.of(c)) == want
    assert check_batch([bases], [bytes(quals)], c) == [want]


def test_default_config_is_bbmaps():
    c = T.default_config()
    assert (c.mode, c.trimLeft, c.trimRight, c.trimq, c.minLength, c.windowLength, c.minGoodInterval, c.optimalBias) == (0, 0, 0, 6, 60, 4, 2, -1.0)
    L = _lib.load()
    trim_exports = ["bbtrim_default_config", "bbtrim_batch", "bbtrim_batch_device"]
    assert [s for s in _lib.EXPORTS if s.startswith("bbtrim_")] == sorted(trim_exports)
    assert all(hasattr(L, s) for s in trim_exports) and hasattr(L, "bbmap_untrim_batch_device")


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("mode", [OPT, WIN, INT])
def test_every_side_trimq_and_min_length(mode):
    cases = case_reads()
    reads, quals = [c[0] for c in cases], [c[1] for c in cases]
    by_len = {n: [i for i, r in enumerate(reads) if len(r) == n] for n in LENGTHS}
    trimmed = 0
    for (left, right), trimq in itertools.product(SIDES, TRIMQS):
        for ml in (0, 1, 60):
            got = check_batch(reads, quals, cfg(mode, left, right, trimq, ml))
            trimmed += sum(1 for g in got if g != (0, 0))
        for n, idx in by_len.items():                       # minLength = len and len + 1: nothing may be trimmed
            for ml in (n, n + 1):
                got = check_batch([reads[i] for i in idx], [quals[i] for i in idx], cfg(mode, left, right, trimq, ml))
                assert all(g == (0, 0) for g in got)
    assert trimmed > 200


@pytest.mark.parametrize("mode", [OPT, WIN, INT])
def test_without_a_quality_array(mode):
    reads = [c[0] for c in case_reads()] + [b"NNACGTNACGTAANN", b"NANACGTACGTANAN", b"N" * 20, b"ACGT" * 5]
    seen = set()
    for (left, right), trimq, ml in itertools.product(SIDES, (0, 1, 10), (0, 5)):
        seen.update(check_batch(reads, None, cfg(mode, left, right, trimq, ml)))
    assert len(seen) > 3
    if mode == OPT:                                         # an average error rate of 1 switches the N-only scan off (:268)
        assert set(check_batch(reads, None, cfg(OPT, optimalBias=1.0))) == {(0, 0)}


def test_optimal_bias():
    cases = case_reads()
    reads, quals = [c[0] for c in cases], [c[1] for c in cases]
    a = check_batch(reads, quals, cfg(OPT, trimq=10, optimalBias=0.05))
    b = check_batch(reads, quals, cfg(OPT, trimq=41, optimalBias=0.05))       # the bias replaces PROB_ERROR[trimq]
    assert a == b and a != check_batch(reads, quals, cfg(OPT, trimq=10))
    check_batch(reads, quals, cfg(OPT, trimq=10, optimalBias=0.0))


def test_window_lengths_and_good_intervals():
    cases = case_reads()
    reads, quals = [c[0] for c in cases], [c[1] for c in cases]
    for w in (1, 2, 4, 7, 64):
        check_batch(reads, quals, cfg(WIN, trimq=10, windowLength=w))
    for g in (1, 2, 3, 5):
        check_batch(reads, quals, cfg(INT, trimq=10, minGoodInterval=g))
        check_batch(reads, None, cfg(INT, trimq=10, minGoodInterval=g))


def lowered_phix(mode):
    """the PhiX fixture's reads with their qualities lowered to 2 on the last 0..40 and the first 0..10 bases of each read, so that
    qtrim=rl trims both ends by amounts that differ from read to read (mates end up with different lengths).  Every fifth read
    keeps its qualities; reads 3, 13, 23, ... are lowered at the left end only.  Reads 8, 9 and 21 get random bases: they map
    nowhere, and are trimmed like the others."""
    from tests.golden_phix import fixture_inputs
    reads, quals, paired = fixture_inputs(mode, True)
    rng = np.random.default_rng(77)
    reads = [np.asarray(r, np.uint8).copy() for r in reads]
    for i in (8, 9, 21):
        reads[i] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(reads[i]))].copy()
    out = []
    for i, q in enumerate(quals):
        q = np.asarray(q, np.uint8).copy()
        tail, head = int(rng.integers(0, 41)), int(rng.integers(0, 11))
        if i % 5 != 0:
            if i % 10 != 3:
                q[len(q) - tail:] = 2
            q[:head if i % 10 != 3 else max(head, 4)] = 2
        out.append(q)
    return reads, out, paired


def test_phix_qualities():
    from tests.golden_phix import sample_qualities, sample_reads
    for which in (1, 2):
        reads = [bytes(r) for r in sample_reads(which)[0]]
        quals = [bytes(q) for q in sample_qualities(which)]
        for mode in (OPT, WIN, INT):
            for trimq in (6, 10, 20):
                check_batch(reads, quals, cfg(mode, trimq=trimq, minLength=30))
    reads, quals, _ = lowered_phix("pe")
    got = check_batch([bytes(r) for r in reads], [bytes(q) for q in quals], T.from_flags(qtrim="rl", trimq=10, minlength=30))
    assert sum(1 for g in got if g[0] > 0) > 50 and sum(1 for g in got if g[1] > 0) > 50 and sum(1 for g in got if g == (0, 0)) >= 20
    assert sum(1 for g in got if g[0] > 0 and g[1] == 0) >= 10


FLAGS = [
    (dict(), (OPT, 0, 0, 6, 60, 4)),
    (dict(qtrim="l"), (OPT, 1, 0, 6, 60, 4)), (dict(qtrim="left"), (OPT, 1, 0, 6, 60, 4)), (dict(qtrim="L"), (OPT, 1, 0, 6, 60, 4)),
    (dict(qtrim="r"), (OPT, 0, 1, 6, 60, 4)), (dict(qtrim="right"), (OPT, 0, 1, 6, 60, 4)),
    (dict(qtrim="rl"), (OPT, 1, 1, 6, 60, 4)), (dict(qtrim="lr"), (OPT, 1, 1, 6, 60, 4)), (dict(qtrim="both"), (OPT, 1, 1, 6, 60, 4)),
    (dict(qtrim=""), (OPT, 1, 1, 6, 60, 4)),
    (dict(qtrim="w"), (WIN, 0, 1, 6, 60, 4)), (dict(qtrim="window"), (WIN, 0, 1, 6, 60, 4)),
    (dict(qtrim="window,8"), (WIN, 0, 1, 6, 60, 8)), (dict(qtrim="w,3"), (WIN, 0, 1, 6, 60, 3)),
    (dict(qtrim="15"), (OPT, 0, 1, 15, 60, 4)),             # a leading digit: trimq and the right side
    (dict(qtrim="t"), (OPT, 1, 1, 6, 60, 4)), (dict(qtrim="true"), (OPT, 1, 1, 6, 60, 4)), (dict(qtrim=True), (OPT, 1, 1, 6, 60, 4)),
    (dict(qtrim="f"), (OPT, 0, 0, 6, 60, 4)), (dict(qtrim=False), (OPT, 0, 0, 6, 60, 4)),
    (dict(qtrim="r", trimq=10), (OPT, 0, 1, 10, 60, 4)), (dict(qtrim="rl", trimq=10, minlength=30), (OPT, 1, 1, 10, 30, 4)),
    (dict(qtrim="r", optitrim="f"), (INT, 0, 1, 6, 60, 4)), (dict(qtrim="w", optitrim="t"), (OPT, 0, 1, 6, 60, 4)),
    (dict(qtrim="rl", optitrim=False, trimgoodinterval=3), (INT, 1, 1, 6, 60, 4)),
]


@pytest.mark.parametrize("case", FLAGS, ids=[repr(c[0]) for c in FLAGS])
def test_from_flags(case):
    kw, want = case
    c = T.from_flags(**kw)
    assert (c.mode, c.trimLeft, c.trimRight, c.trimq, c.minLength, c.windowLength) == want
    assert c.minGoodInterval == kw.get("trimgoodinterval", 2) and c.optimalBias == -1.0


def test_from_flags_bias():
    c = T.from_flags(qtrim="r", optitrim=".05")
    assert c.mode == OPT and abs(c.optimalBias - 0.05) < 1e-7
    with pytest.raises(ValueError):
        T.from_flags(qtrim="r", optitrim="1.5")
    with pytest.raises(ValueError):
        T.from_flags(qtrim="sideways")


def test_refusals():
    L = _lib.load()
    recs, blob, _ = pack([b"ACGT"])
    out, trims = np.zeros(1, READ_DTYPE), np.zeros(1, T.TRIM_DTYPE)
    args = lambda c, n=1, o=out: (None if c is None else C.byref(c), n, recs.ctypes.data, blob.ctypes.data, None, o.ctypes.data, trims.ctypes.data)  # noqa: E731
    assert L.bbtrim_batch(*args(None)) == -2 and L.bbmap_last_error() == b"bbtrim_batch: null config"
    assert L.bbtrim_batch(*args(cfg(), n=-1)) == -2 and L.bbmap_last_error() == b"bbtrim_batch: bad read count"
    assert L.bbtrim_batch(*args(cfg(), o=recs)) == -2 and L.bbmap_last_error() == b"bbtrim_batch: reads_out must not alias reads_in"
    for bad in (cfg(trimq=127), cfg(trimq=-1), cfg(mode=3), cfg(mode=-1), cfg(windowLength=0), cfg(minGoodInterval=0), cfg(optimalBias=1.5)):
        assert L.bbtrim_batch(*args(bad)) == -2 and L.bbmap_last_error().startswith(b"bbtrim_batch: bad config")
    assert L.bbtrim_default_config(None) == -2
    assert L.bbtrim_batch(C.byref(cfg()), 0, None, None, None, None, None) == 0          # nothing to do
    # the device form refuses the same before it touches a device
    assert L.bbtrim_batch_device(None, None, 1, None, None, None, None, None) == -2 and L.bbmap_last_error() == b"bbtrim_batch_device: null config"
    assert L.bbtrim_batch_device(C.byref(cfg(trimq=127)), None, 1, None, None, None, None, None) == -2
    assert L.bbtrim_batch_device(C.byref(cfg()), None, 0, None, None, None, None, None) == 0
    assert L.bbmap_untrim_batch_device(None, None, None, None) == -2 and L.bbmap_last_error() == b"bbmap_untrim_batch_device: null argument"


def test_trimmed_records_give_the_keys_of_the_trimmed_reads():
    """the key stage addresses a read through (bases_off, len) alone: the moved records over the full blob give what the trimmed
    reads packed back to back give"""
    reads, quals, _ = lowered_phix("pe")
    recs, blob, qblob = pack([bytes(r) for r in reads], [bytes(q) for q in quals])
    out, trims = T.trim_batch(recs, blob, qblob, T.from_flags(qtrim="rl", trimq=10, minlength=30))
    assert int(trims["left"].max()) > 0 and int(trims["right"].max()) > 0
    tr = [r[int(t["left"]): len(r) - int(t["right"])] for r, t in zip(reads, trims)]
    tq = [q[int(t["left"]): len(q) - int(t["right"])] for q, t in zip(quals, trims)]
    wrecs, wblob, wbs, wki = K.make_batch(tr, tq)
    L = _lib.load()
    kc = K.default_config()
    n = len(out)
    offs, lens = np.ascontiguousarray(out["bases_off"], np.int64), np.ascontiguousarray(out["len"], np.int32)
    grecs, gki, gbs, used = np.zeros(n, READ_DTYPE), np.zeros(2 * int(lens.sum()) + 2, np.int32), np.zeros(len(blob), np.int8), C.c_int64(0)
    _lib.check(L.bbkeys_make_batch(C.byref(kc), n, offs.ctypes.data, lens.ctypes.data, blob.ctypes.data, qblob.ctypes.data, grecs.ctypes.data,
                                   gki.ctypes.data, gki.size, gbs.ctypes.data, C.byref(used)), "bbkeys_make_batch")
    assert np.array_equal(grecs["nkeys"], wrecs["nkeys"]) and np.array_equal(grecs["keys_off"], wrecs["keys_off"]) and int(wrecs["nkeys"].sum()) > n
    assert np.array_equal(grecs["len"], wrecs["len"]) and np.array_equal(grecs["bases_off"], out["bases_off"])
    assert np.array_equal(gki[:used.value], wki[:used.value])
    for g, w in zip(grecs, wrecs):
        assert np.array_equal(gbs[int(g["bases_off"]): int(g["bases_off"]) + int(g["len"])], wbs[int(w["bases_off"]): int(w["bases_off"]) + int(w["len"])])
