"""Read histograms on the device (bbmap_hist_* / bbpipe_read_hist_*) against the sequential restatement of align2.ReadStats
(tests/readstats_check.py): every array the device returns equals the restatement's exactly (all state is 64-bit integers, so the
order of the adds does not matter).  Raw form over planted records first, then the context form over the PhiX fixture's pairs with
their qualities, then the text.

The restatement's groups do not read one another's state, so its arrays under all flags are also the expected arrays of every
subset of the flags; and accumulation is a sum, so the expectation for k distinct records repeated n_i times is the sum of n_i times
each record's own arrays (the two maxima apart).  Both are used below to keep the restatement's Python loops short."""
import ctypes as C

import numpy as np
import pytest
import torch

from bbmap_amd import _lib
from bbmap_amd import readstats as R
from bbmap_amd.index import DeviceIndex, READ_DTYPE
from bbmap_amd.mapper import FINAL_DTYPE, Mapper
from tests import readstats_check as K
from tests.test_readstats_cpu import assert_text

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, QT = R.RH_POS_TILE, R.RH_QUAL_TILE
READ_SYMS = np.frombuffer(b"ACGTACGTACGTACGTNacgtnU", np.uint8)
SYMS = np.frombuffer(b"mmmmmmmmmmmmmmmmSSDIXYNC", np.uint8)
QUALS = np.array([0, 2, 41, 93, 98, 99, 126, 200, QT - 1, QT, 30, 30, 30, 37, 37, 12], np.uint8)     # 200: above the last bin

STRINGS = [b"m", b"m" * 63, b"m" * 64, b"m" * 65, b"m" * 129,
           b"m" * 70,                                       # an m run across a 64-symbol step
           b"m" * 60 + b"D" * 10 + b"m" * 10,               # a D run across one
           b"m" * 60 + b"I" * 10 + b"m" * 10,               # an I run across one
           # (the indel walk looks at the first min(len, MAXLEN) SYMBOLS: a read has to be as long as the run's end lies deep)
           b"m" * 5 + b"D" * 256 + b"m" * 270,              # 2 x 128 D: an expanded gap
           b"m" * 3 + b"D" * 999 + b"m" * 1010, b"m" * 3 + b"D" * 1000 + b"m" * 1010, b"m" * 3 + b"D" * 1001 + b"m" * 1010,
           b"m" * 3 + b"I" * 1000 + b"m" * 3, b"m" * 3 + b"I" * 1001 + b"m" * 3,
           b"C" * 3 + b"m" * 20, b"X" * 2 + b"m" * 20 + b"Y" * 2, b"N" * 2 + b"m" * 20, b"I" * 64 + b"m" * 3, b"D" * 3 + b"m" * 70,
           b"mD" * 40, b"m" * 63 + b"D" + b"m" * 63 + b"I" * 64 + b"S" * 3 + b"N" * 2, b"m" * 64 + b"D" * 64 + b"I" * 64 + b"m" * 64,
           b"m" * 29 + b"S" * 71, b"m" * 57 + b"S" * 43, b"S" * 71 + b"m" * 29,      # identity on a bin edge: 29/100, 57/100 (and 1/1 above)
           b"m" * 29 + b"D" * 71, b"mR" * 8 + b"N" * 5 + b"C" * 9 + b"?" * 2]
LENGTHS = [1, 63, 64, 65, T - 1, T, T + 1, 5999, 6000, 6001, 6016]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _read(rng, n, syms=READ_SYMS):
    return syms[rng.integers(0, len(syms), n)].tobytes()


def _qual(rng, n):
    return QUALS[rng.integers(0, len(QUALS), n)].tobytes()


def _planted(rng, long_reads=True, extra=60):
    """[(mapped, strand, bases, quality, match)]: the issue's list; every string on both strands, with a read that fits it, one
    that is longer and one that is shorter"""
    out = []

    def put(mapped, strand, n, match, syms=READ_SYMS):
        out.append((mapped, strand, _read(rng, n, syms), _qual(rng, n), match))

    put(0, 0, 50, None)                                                          # unmapped
    put(0, 1, 50, b"m" * 50)                                                     # unmapped with a stale string: not counted
    put(1, 1, 40, b"m" * 40, np.frombuffer(b"ATatTAUu", np.uint8))               # all AT: gc 0
    put(1, 0, 40, b"m" * 40, np.frombuffer(b"Nn", np.uint8))                     # no defined base at all (as a pair: gc 0 as well)
    put(1, 0, 50, None)                                                          # mapped, match_len = 0
    for s in STRINGS:
        fits = sum(1 for c in s if c != ord("D"))
        for strand in (0, 1):
            put(1, strand, fits, s)
            put(1, strand, fits + 7, s)                                          # the string ends before the read does
            put(1, strand, max(1, fits - 5), s)                                  # the string overruns its read
    for n in LENGTHS if long_reads else LENGTHS[:7]:
        for strand in (0, 1):
            put(1, strand, n, b"m" * n)
            put(1, strand, n, b"m" * (n // 2) + b"D" * 3 + b"S" + b"m" * (n - n // 2 - 1))
        put(1, 0, n, b"m" * max(0, n - 3) + b"D" * 10 + b"m" * 3)               # the indel walk's len limit cuts the D run
        put(0, 0, n, None)
    for _ in range(extra):
        put(1, int(rng.integers(0, 2)), int(rng.integers(1, 200)), _read(rng, int(rng.integers(1, 260)), SYMS) if rng.random() < 0.9 else None)
    if len(out) & 1:
        put(1, 0, 10, b"m" * 10)                                                 # (an even number: the same list serves as pairs)
    return out


def _upload(records, with_quality=True):
    n = len(records)
    fin, reads = np.zeros(n, FINAL_DTYPE), np.zeros(n, READ_DTYPE)
    pool, bases, quals = [np.zeros(3, np.uint8)], [], []
    poff, boff = 3, 0
    for r, (mapped, strand, b, q, m) in enumerate(records):
        f = fin[r]
        f["mapped"], f["strand"], f["chrom"], f["start"], f["stop"] = mapped, strand, 1, 1000, 1000 + len(b)
        if m:
            f["match_len"], f["match_off"] = len(m), poff
            pool.append(np.frombuffer(m, np.uint8)); poff += len(m)
        reads[r]["len"], reads[r]["bases_off"] = len(b), boff
        bases.append(np.frombuffer(b, np.uint8)); quals.append(np.frombuffer(q, np.uint8)); boff += len(b)
    pad = [np.zeros(1, np.uint8)]
    return (_dev(reads), _dev(np.concatenate(bases + pad)), _dev(np.concatenate(quals + pad)) if with_quality else None, _dev(fin),
            _dev(np.concatenate(pool)))


def _restatement(records, paired, with_quality=True, rs=None):
    rs = rs or K.ReadStats()
    reads = [b for _, _, b, _, _ in records]
    fin = np.zeros(len(records), [("mapped", "i4"), ("strand", "i4")])
    fin["mapped"], fin["strand"] = [x[0] for x in records], [x[1] for x in records]
    rs.add_batch(reads, [q for _, _, _, q, _ in records] if with_quality else None, fin, [m for _, _, _, _, m in records], paired)
    return rs


def _compare(h, rs, flags=R.RH_ALL):
    want = {k: v for k, v in rs.arrays().items()}
    got = {k: v for k, v in h.arrays.items() if v is not None}
    group = {"match": R.RH_MATCH, "qual_length": R.RH_QUALITY, "bqual": R.RH_QUALITY, "qcount": R.RH_QUALITY, "base": R.RH_BASE,
             "accuracy": R.RH_ACCURACY, "ins": R.RH_INDEL, "del": R.RH_INDEL, "del2": R.RH_INDEL, "error": R.RH_ERROR, "length": R.RH_LENGTH,
             "gc": R.RH_GC, "identity": R.RH_IDENTITY}
    assert sorted(got) == sorted(k for k in want if group[k] & flags)
    for name, a in got.items():
        w = np.asarray(want[name]).reshape(a.shape)
        if name in ("gc", "identity"):                      # the last word is the maximum: 0 on the device until something counts
            assert max(1, int(a[-1])) == int(w[-1]), name
            a, w = a[:-1], w[:-1]
        assert np.array_equal(a, w), (name, np.argwhere(a != w)[:8], a[a != w][:8], w[a != w][:8])


_CACHE = {}


def _set(name):
    """(records, restatement single-ended, restatement paired): built once and left unchanged"""
    if name not in _CACHE:
        recs = _planted(np.random.default_rng(11), long_reads=name == "full", extra=60 if name == "full" else 30)
        _CACHE[name] = (recs, _restatement(recs, False), _restatement(recs, True))
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ the raw form, planted records
@pytest.mark.parametrize("paired", [False, True])
def test_planted_records_every_array(paired):
    recs, single, pair = _set("full")
    rs = pair if paired else single
    state = R.DeviceState(R.RH_ALL)
    state.add(*_upload(recs), paired=paired)
    h = state.read()
    _compare(h, rs)
    # the planted list reaches what it is meant to reach
    assert rs.match[:, :, T:].any() and rs.match[2].any() and rs.match[4].any() and rs.match[5].any() and rs.match[6].any()
    assert rs.baseHist[:, :, R.RH_MAXLEN:].any() and rs.lengthHist[6016] and rs.qualLength[0][5999] >= 3
    assert rs.bqualHist[:, :T, QT:].any() and rs.bqualHist[:, T:, :].any() and rs.bqualHist[0, :, 126].any() and rs.accuracy[:, 98].any()
    assert rs.delHist[999] and rs.delHist2[10] >= 2 and rs.insHist[1000] >= 2 and rs.delHist[256] and rs.delHist[10]
    assert rs.idHist[29] and rs.idHist[57] and rs.idHist[100] and rs.gcHist[0] and rs.errorHist[71]
    assert paired == bool(rs.match[:, 1].any())


def test_no_quality_array():
    recs, _, _ = _set("small")
    rs = _restatement(recs, True, with_quality=False)
    state = R.DeviceState(R.RH_ALL)
    state.add(*_upload(recs, with_quality=False), paired=True)
    h = state.read()
    _compare(h, rs)
    assert not h.bqual.any() and not h.qcount.any() and not h.qual_length.any() and not h.accuracy.any() and h.match.any()


def test_every_group_alone_and_every_group_left_out():
    """the walks are shared between the groups: each must count the same whichever others are selected"""
    recs, _, rs = _set("small")
    up = _upload(recs)
    for flags in list(R.RH_GROUPS) + [R.RH_ALL & ~g for g in R.RH_GROUPS] + [R.RH_MATCH | R.RH_INDEL, R.RH_ACCURACY | R.RH_GC | R.RH_LENGTH]:
        state = R.DeviceState(flags)
        state.add(*up, paired=True)
        _compare(state.read(), rs, flags)


def test_two_batches_into_one_state_then_a_reset():
    recs, _, rs1 = _set("small")
    more = _planted(np.random.default_rng(12), long_reads=False, extra=40)
    state = R.DeviceState(R.RH_ALL)
    state.add(*_upload(recs), paired=True)
    _compare(state.read(), rs1)
    state.add(*_upload(more), paired=True)
    both = _restatement(more, True, rs=_restatement(recs, True))
    _compare(state.read(), both)
    state.reset()
    assert not state.read().block.any()


def test_many_identical_reads_several_workgroups_several_chunks():
    """more 150-base reads than the grid's workgroups take in one chunk each: every workgroup flushes into the same counters, and
    the first ones count a second chunk after their flush"""
    rng = np.random.default_rng(3)
    kinds = [(1, 0, _read(rng, 150), bytes([37] * 150), b"m" * 150), (1, 1, _read(rng, 150), bytes([2] * 75 + [41] * 75), b"m" * 70 + b"S" + b"m" * 79),
             (1, 0, _read(rng, 150), bytes([12] * 150), b"m" * 50 + b"D" * 4 + b"m" * 98 + b"I" * 2), (0, 0, _read(rng, 150), bytes([30] * 150), None)]
    n = (R.RH_MAX_BLOCKS + 3) * R.RH_CHUNK_UNITS + 17
    kind = np.arange(n) % 4
    fin, reads = np.zeros(n, FINAL_DTYPE), np.zeros(n, READ_DTYPE)
    pool, poff = [np.zeros(3, np.uint8)], []
    at = 3
    for _, _, _, _, m in kinds:
        poff.append(at)
        if m:
            pool.append(np.frombuffer(m, np.uint8)); at += len(m)
    fin["mapped"], fin["strand"] = np.array([k[0] for k in kinds])[kind], np.array([k[1] for k in kinds])[kind]
    fin["match_len"], fin["match_off"] = np.array([len(k[4] or b"") for k in kinds])[kind], np.array(poff)[kind]
    reads["len"], reads["bases_off"] = 150, 150 * kind
    bases = np.concatenate([np.frombuffer(k[2], np.uint8) for k in kinds])
    quals = np.concatenate([np.frombuffer(k[3], np.uint8) for k in kinds])
    state = R.DeviceState(R.RH_ALL)
    state.add(_dev(reads), _dev(bases), _dev(quals), _dev(fin), _dev(np.concatenate(pool)), paired=False)
    h = state.read()
    sums = None
    for i, k in enumerate(kinds):
        one = _restatement([k], False).arrays()
        count = int(np.count_nonzero(kind == i))
        sums = {name: a * count for name, a in one.items()} if sums is None else {name: sums[name] + a * count for name, a in one.items()}
    for name, a in h.arrays.items():
        w = sums[name].reshape(a.shape)
        if name in ("gc", "identity"):
            assert int(a[-1]) == 150
            a, w = a[:-1], w[:-1]
        assert np.array_equal(a, w), name
    assert int(h.length[150]) == n and int(h.base.sum()) == 150 * n


def test_raw_call_on_nothing():
    L = _lib.load()
    assert L.bbpipe_read_hist_add_device(None, 0, 0, R.RH_ALL, *([None] * 6)) == 0
    state = R.DeviceState(R.RH_GC)
    assert state.words == R.RH_GC_BINS + 2


# ------------------------------------------------------------------------------------------------ the context form, PhiX pairs
def _phix(mode, hist=True, **kw):
    from tests.golden_phix import fixture_inputs, phix_reference
    reads, quals, paired = fixture_inputs(mode, True)
    di = DeviceIndex.build([phix_reference()], k=13)
    mp = Mapper.from_reads(di, [len(r) for r in reads], np.concatenate(reads), np.concatenate(quals), paired=paired, **kw)
    if hist:
        mp.enable_read_hist()
    return di, mp, [bytes(r) for r in reads], [bytes(q) for q in quals], paired


def _restate_context(mp, reads, quals, paired, rs=None):
    fin, blob = mp.final()
    matches = [blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None for f in fin]
    rs = rs or K.ReadStats()
    rs.add_batch(reads, quals, fin, matches, paired)
    return rs, fin, blob


@pytest.mark.parametrize("mode", ["pe", "se1"])
def test_phix_reads_with_their_qualities(mode):
    di, mp, reads, quals, paired = _phix(mode, max_sites=32)
    try:
        mp.enable_read_hist(R.RH_ALL)                       # the same flags again: nothing changes
        assert mp.L.bbmap_add_read_hist(mp.h, None, None) == -2 and mp.L.bbmap_last_error() == b"bbmap_add_read_hist: no batch has been mapped yet"
        mp.step()
        mp.add_read_hist()
        assert mp.L.bbmap_add_read_hist(mp.h, None, None) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_add_read_hist: the last batch has been counted already"
        assert mp.L.bbmap_hist_enable(mp.h, R.RH_MATCH) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_hist_enable: the histograms are enabled already with other flags"
        h = mp.read_hist()
        rs, fin, blob = _restate_context(mp, reads, quals, paired)
        _compare(h, rs)
        assert_text(h, rs, paired)
        assert int(h.length[100]) == len(reads) and int(np.count_nonzero(fin["mapped"])) > 0.9 * len(reads) and h.accuracy.any()
        assert int(h.id_hist.sum()) == int(np.count_nonzero((fin["mapped"] != 0) & (fin["match_len"] > 0)))
        assert int(h.gc_hist.sum()) == (len(reads) // 2 if paired else len(reads))
        # the view's pointers are the device's, in the order of the host copy
        w = R.bbmap_readhist_view()
        assert mp.L.bbmap_get_read_hist_view(mp.h, C.byref(w)) == 0 and w.flags == R.RH_ALL and w.words == h.block.size and w.match == w.state
        # the feature only reads: the batch's records and strings are what a run without histograms gives
        di0, mp0, _, _, _ = _phix(mode, hist=False, max_sites=32)
        try:
            mp0.step()
            fin0, blob0 = mp0.final()
            assert fin0.tobytes() == fin.tobytes() and blob0.tobytes() == blob.tobytes()
        finally:
            mp0.close()
            di0.close()
        # a second step adds to the first; a reset zeroes; the batch the context holds may then be added again
        mp.step()
        mp.add_read_hist()
        rs, _, _ = _restate_context(mp, reads, quals, paired, rs=rs)
        _compare(mp.read_hist(), rs)
        mp.reset_read_hist()
        assert not mp.read_hist().block.any()
        mp.add_read_hist()
        assert int(mp.read_hist().length[100]) == len(reads)
    finally:
        mp.close()
        di.close()


def test_phix_overflow_tier_records_are_counted():
    """max_sites = 1: most pairs are mapped by the overflow tier.  Their records and strings are read from the tier's own output, as
    the run-statistics and coverage tests read them (tests/test_runstats_gpu.py::_restate): the main context's final stage runs
    before the tier's reads are marked in the main list, so bbmap_get_final alone does not show which records the tier replaced."""
    from tests.test_runstats_gpu import _restate
    di, mp, reads, quals, paired = _phix("pe", max_sites=1, reserved=(C.c_int32 * 4)(0, 4096, 256, 0))
    try:
        mp.step()
        assert mp.stats()["reads_reprobed"] > 0
        mp.add_read_hist()
        fin, matches, _, _ = _restate(mp, [np.frombuffer(r, np.uint8) for r in reads], paired, None)
        rs = K.ReadStats()
        rs.add_batch(reads, quals, fin, matches, paired)
        _compare(mp.read_hist(), rs)
        assert int(np.count_nonzero(fin["mapped"])) > 0.9 * len(reads)
    finally:
        mp.close()
        di.close()


def test_refusals():
    di, mp, _, _, _ = _phix("pe", hist=False, max_sites=32, finalStage=0)
    try:
        assert mp.L.bbmap_hist_enable(mp.h, R.RH_ALL) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_hist_enable: the context runs without the final stage (bbmap_config.finalStage)"
    finally:
        mp.close()
        di.close()
    di, mp, _, _, _ = _phix("pe", hist=False, max_sites=32)
    try:
        assert mp.L.bbmap_add_read_hist(mp.h, None, None) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_add_read_hist: the histograms are not enabled (bbmap_hist_enable)"
        assert mp.L.bbmap_hist_enable(mp.h, 512) == -2 and mp.L.bbmap_last_error() == b"bbmap_hist_enable: unknown flag bits"
        assert mp.L.bbmap_hist_enable(mp.h, 0) == -2 and mp.L.bbmap_last_error() == b"bbmap_hist_enable: no histogram group selected"
        assert mp.L.bbmap_get_read_hist(mp.h, None, 0, None) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_get_read_hist: the histograms are not enabled (bbmap_hist_enable)"
        assert mp.L.bbmap_reset_read_hist(mp.h) == 0            # nothing to reset
        mp.enable_read_hist(R.RH_MATCH | R.RH_IDENTITY)
        mp.step()
        mp.add_read_hist()
        h = mp.read_hist()
        assert h.flags == R.RH_MATCH | R.RH_IDENTITY and h.bqual is None and h.match.any() and h.id_hist.any()
    finally:
        mp.close()
        di.close()


# ------------------------------------------------------------------------------------------------ text
@pytest.mark.parametrize("paired", [True, False])
def test_text_from_the_device_state(paired):
    recs, single, pair = _set("small")
    rs = pair if paired else single
    state = R.DeviceState(R.RH_ALL)
    state.add(*_upload(recs), paired=paired)
    h = state.read()
    assert_text(h, rs, paired)                              # mhist qhist bqhist qchist bhist qahist indelhist ehist lhist gchist idhist
    assert len(h.mhist_lines(paired)) > T and len(h.qahist_lines()) > 90 and len(h.indelhist_lines()) > 5
    state = R.DeviceState(R.RH_QUALITY)                     # without the match histogram qhist has no "measured" column
    state.add(*_upload(recs), paired=paired)
    h = state.read()
    rq = K.ReadStats(R.RH_QUALITY)
    rq.qualLength, rq.qualSum, rq.qualSumDouble, rq.bqualHist, rq.qcountHist = rs.qualLength, rs.qualSum, rs.qualSumDouble, rs.bqualHist, rs.qcountHist
    rq.bqualHistOverall = rs.bqualHistOverall
    assert_text(h, rq, paired)
    assert "measured" not in h.qhist_lines(paired)[0]
