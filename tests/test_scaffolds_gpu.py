"""Multi-scaffold references on the device mapper: bbidx_set_scaffolds (the quickMap-tail filter of removeOutOfBounds,
Data.isSingleScaffold) and bbmap_get_scaffold_records (SamLine's coordinate block).

The CPU oracle has no scaffold table, so parity is pinned three ways: reads the filter does not touch equal oracle.map_reads exactly;
reads it touches are checked against the test-local restatement in tests/scaffold_check.py; and the final stage is checked downstream
of the filter (the device's post-rescue lists through oracle.final_reads equal the device's final records)."""
import ctypes as C
import functools

import numpy as np
import pytest

from bbmap_amd import keys as K
from bbmap_amd import reference as R
from bbmap_amd.index import DeviceIndex, PROFILE_PACBIO
from bbmap_amd.mapper import Mapper
from oracle import oracle as O
from tests import scaffold_check as SC
from tests.mapper_check import FINAL_FIELDS, SITE_FIELDS, compare, compare_final, gpu_fills

pytestmark = pytest.mark.gpu
L, KL = 150, 12
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b


def _rc(a):
    return COMP[np.asarray(a, np.uint8)[::-1]]


@functools.lru_cache(maxsize=None)
def genome():
    """About 40 seeded scaffolds (some shorter than a read) packed into three chromosomes."""
    rng = np.random.default_rng(11)
    lens = np.exp(rng.uniform(np.log(200), np.log(50000), 40)).astype(int)
    lens[[5, 17, 29]] = [90, 120, 140]                        # shorter than a read
    recs = [("scaf%d desc" % i, ACGT[rng.integers(0, 4, int(n))]) for i, n in enumerate(lens)]
    body = sum(len(b) for _, b in recs) + 300 * len(recs)
    for ml in range(body // 3 + 16300, body + 40000, 2000):
        p = R.pack(recs, max_length=ml)
        if p.nchroms == 3:
            return p
    raise AssertionError("no max_length gives three chromosomes")


def _mutate(rng, a, n):
    a = a.copy()
    for i in rng.choice(len(a), n, replace=False):
        a[i] = ACGT[(int(np.searchsorted(ACGT, a[i])) + 1 + int(rng.integers(0, 3))) % 4] if a[i] != ord("N") else a[i]
    return a


def _read_sets(paired, seed):
    """(reads uint8[n, L], kind per read: 0 ordinary / 1 chimeric / 2 hangs into a pad, truth (global scaffold, 1-based pos) or None)"""
    p = genome()
    rng = np.random.default_rng(seed)
    sb = p.scaffold_bases()
    nexts = [g for g in range(len(sb) - 1) if sb[g + 1][0] == sb[g][0]]          # scaffolds followed by one on the same chromosome
    big = [g for g in range(len(sb)) if sb[g][2] >= 500]
    reads, kinds, truth = [], [], []

    def ordinary():
        g = int(rng.choice(big))
        c, a, n = sb[g]
        o = int(rng.integers(0, n - 400))
        return g, c, a + o, o

    def chimeric():
        g = int(rng.choice(nexts))
        (c, a, n), (_, b, m) = sb[g], sb[g + 1]
        h = int(rng.integers(30, 120))
        h = min(h, n)
        t = min(L - h, m)
        seg = np.concatenate([p.chroms[c - 1][a + n - h: a + n], p.chroms[c - 1][b: b + t]])
        if len(seg) < L:
            seg = np.concatenate([seg, p.chroms[c - 1][b + t: b + t + L - len(seg)]])
        return seg, g, c, b

    def hanging():
        g = int(rng.choice(big))
        c, a, n = sb[g]
        out = int(rng.integers(10, 60))
        if rng.random() < 0.5:
            return p.chroms[c - 1][a + n - (L - out): a + n + out], c, a + n + out
        return p.chroms[c - 1][a - out: a - out + L], c, a - out + L

    units = 260 if paired else 520
    for u in range(units):
        kind = 0 if u % 4 < 2 else (1 if u % 4 == 2 else 2)
        if kind == 0:
            g, c, s, o = ordinary()
            seg = p.chroms[c - 1][s: s + L]
            mates = [(_mutate(rng, seg, 3), 0, (g, o + 1))]
            if paired:
                mates.append((_rc(_mutate(rng, p.chroms[c - 1][s + 250: s + 250 + L], 2)), 0, (g, o + 251)))
        elif kind == 1:
            seg, g, c, b = chimeric()
            mates = [(_mutate(rng, seg, 2), 1, None)]
            if paired:                                        # the mate lies in scaffold B, pointing back
                mates.append((_rc(p.chroms[c - 1][b + 150: b + 150 + L]), 1, None))
        else:
            seg, c, e = hanging()
            mates = [(np.asarray(seg, np.uint8), 2, None)]
            if paired:
                mates.append((_rc(p.chroms[c - 1][max(0, e + 100): max(0, e + 100) + L]), 2, None))
        if not paired:
            mates = mates[:1]
        if rng.random() < 0.5 and not paired:
            mates = [(_rc(mates[0][0]), mates[0][1], mates[0][2])]
        for b, k, t in mates:
            assert len(b) == L
            reads.append(np.asarray(b, np.uint8)); kinds.append(k); truth.append(t)
    return np.stack(reads), np.array(kinds), truth


def _offs():
    offs = O.make_offsets(L, KL, 1.9)
    return offs, [100 * KL] * len(offs)


@functools.lru_cache(maxsize=None)
def device_index():
    return DeviceIndex.build(genome().chroms, k=KL)


def _map(reads, paired, table, max_sites=64, **kw):
    """One Mapper step with the index's table set to `table` ("packed", None, or a Packed) -> (fetch, stats, scaffold records)"""
    di = device_index()
    table = genome() if table == "packed" else table
    di.set_scaffolds(table)
    offs, ks = _offs()
    mp = Mapper(di, len(reads), L, offs, ks, paired=paired, max_sites=max_sites, **kw)
    mp.load_reads(reads)
    mp.step()
    out, st = mp.fetch(), mp.stats()
    recs = None
    if mp.cfg.finalStage and table is not None:
        recs, names = mp.scaffold_records()
        assert names == table.scaffold_names()
    mp.close()
    di.set_scaffolds(None)
    return out, st, recs


def _spanning(sites, n, table):
    locs, _, pad, _ = table
    return sum(1 for s in sites[:max(n, 0)] if not SC.is_single_scaffold(locs, pad, int(s["chrom"]), int(s["start"]), int(s["stop"])))


def _probe(reads, paired, max_sites=256):
    """find_batch over the same reads (after a Mapper has set quitAfterTwoPerfects as the mapper does): per read, the spanning
    sites that removeOutOfBounds would drop"""
    di = device_index()
    offs, ks = _offs()
    lists, ns = di.find_batch([(r, np.zeros(L, np.int8), ks, offs) for r in reads], max_sites=max_sites, codes=True)
    assert (ns >= 0).all(), "size max_sites so that nothing overflows"
    tab = SC.table_of(genome())
    lens = [len(c) for c in genome().chroms]
    per = []
    for lst in lists:
        k = 0
        for s in lst:
            if s["start"] < 0 or s["stop"] > lens[s["chrom"] - 1] - 1:
                continue
            if not SC.is_single_scaffold(tab[0], tab[2], s["chrom"], s["start"], s["stop"]):
                k += 1
        per.append(k)
    return np.array(per)


def _units_touched(per, paired):
    t = per > 0
    if paired:
        t = np.repeat(t[0::2] | t[1::2], 2)
    return t


def _recs_of(n):
    recs = np.zeros(n, O.READ_DTYPE)
    recs["bases_off"] = np.arange(n, dtype=np.int64) * L
    recs["len"] = L
    return recs


def _final_strings(out):
    fin, blob = out["final"], out["final_match"]
    return [blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None
            for f in fin]


def _assert_no_spanning(out, tab):
    for r in range(len(out["nsites"])):
        assert _spanning(out["sites"][r], int(out["nsites"][r]), tab) == 0, r
    if "overflow" in out:
        t = out["overflow"]
        for i in range(len(t["nsites"])):
            assert _spanning(t["sites"][i], int(t["nsites"][i]), tab) == 0
    if "final" in out:
        for f in out["final"]:
            if int(f["mapped"]):
                assert SC.is_single_scaffold(tab[0], tab[2], int(f["chrom"]), int(f["start"]), int(f["stop"]))


def _same_outputs(a, b):
    """Two runs' outputs are the same: site lists, final records and match strings, and every fill keyed by (read, seq).  Where a
    fill or a string lands in its log or pool follows the order in which threads claim slots, so log positions and pool offsets
    (match_job, reserved, match_off) are compared through what they point at, not as numbers."""
    assert np.array_equal(a["nsites"], b["nsites"])
    for r in range(len(a["nsites"])):
        n = max(int(a["nsites"][r]), 0)
        for f in SITE_FIELDS + ("gaps",):
            assert np.array_equal(a["sites"][r, :n][f], b["sites"][r, :n][f]), (r, f)
    fa, fb = gpu_fills(a), gpu_fills(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        assert {x: v for x, v in fa[k].items() if x != "index"} == {x: v for x, v in fb[k].items() if x != "index"}, k
    if "final" in a or "final" in b:
        for f in FINAL_FIELDS:
            assert np.array_equal(a["final"][f], b["final"][f]), f
        assert _final_strings(a) == _final_strings(b)


@pytest.mark.parametrize("paired", [False, True])
def test_scaffold_filter_coordinates_and_parity(paired):
    reads, kinds, truth = _read_sets(paired, 3 + paired)
    n = len(reads)
    tab = SC.table_of(genome())
    base, st0, _ = _map(reads, paired, None)                  # no table: what the mapper did before the feature
    fs1, st1, recs = _map(reads, paired, "packed")
    fs0, st_0, _ = _map(reads, paired, "packed", finalStage=0)
    per = _probe(reads, paired)
    for st in (st0, st1, st_0):
        assert st["reads_overflowed"] == 0 and st["reads_reprobed"] == 0
    # (1) the case is real without the table, and gone with it: lists after rescue, lists after the final stage, final records
    spans_before = sum(_spanning(base["sites"][r], int(base["nsites"][r]), tab) for r in range(n))
    assert spans_before > 0
    _assert_no_spanning(fs1, tab)
    _assert_no_spanning(fs0, tab)
    # (2) the counter is what removeOutOfBounds would drop from the probe's lists
    assert st1["sites_cross_scaffold"] == st_0["sites_cross_scaffold"] == int(per.sum()) > 0
    assert st0["sites_cross_scaffold"] == 0
    touched = _units_touched(per, paired)
    assert touched.any() and not touched.all()
    # (3) untouched reads equal the oracle (no table there), field by field, fill logs and match strings included
    chroms = genome().chroms
    oi = O.OracleIndex(chroms, k=KL)
    if paired:
        oi.s.p.quitAfterTwoPerfects = 0
    offs, ks = _offs()
    recs_o = _recs_of(n)
    recs_o["nkeys"] = len(offs)
    keyinfo = np.concatenate([np.asarray(offs, np.int32), np.asarray(ks, np.int32)])
    orc = O.map_reads(oi, recs_o, reads.reshape(-1), keyinfo, None, paired, cap=64, threads=8, match_stride=4200)
    untouched = [r for r in range(n) if not touched[r]]
    bad = compare(fs1, orc, n, paired, reads_range=untouched)
    assert not bad, "\n".join(bad[:10])
    # (4) downstream of the filter: the device's post-rescue lists through the oracle's final stage = the device's final records
    s = fs0["sites"].copy()
    s["match_job"] = -1
    orc_f = O.final_reads(oi, recs_o, reads.reshape(-1), s, fs0["nsites"], paired=paired)
    bad = compare_final(fs1, orc_f, range(n), paired)
    assert not bad, "\n".join(bad[:10])
    # (5) SamLine's block on the device's own records and strings
    want = SC.scaffold_records(tab, fs1["final"], _final_strings(fs1), paired)
    assert np.array_equal(recs, want), [(r, recs[r], want[r]) for r in range(n) if recs[r] != want[r]][:5]
    # ordinary reads land on their scaffold and position at least as often as the oracle's records say (less the reads the filter
    # touched, which alone may differ)
    want_o = SC.scaffold_records(tab, orc["final"], [orc["fmatch"][r][:int(orc["final"][r]["match_len"])].tobytes() or None for r in range(n)],
                                 paired)
    ordi = [r for r in range(n) if kinds[r] == 0]
    hit = lambda rr: np.mean([rr[r]["scaffold"] == truth[r][0] and rr[r]["pos"] == truth[r][1] for r in ordi])
    floor = hit(want_o) - np.mean([touched[r] for r in ordi])
    assert floor > 0.8 and hit(recs) >= floor
    # (6) a table of one scaffold per chromosome, and a cleared table, map as no table does
    one = R.Packed(genome().chroms, [np.array([8000], np.int32)] * 3, [np.array([len(c) - 16001], np.int32) for c in chroms],
                   [["c%d" % i] for i in range(3)], 300)
    out1, st_one, _ = _map(reads, paired, one)
    assert st_one["sites_cross_scaffold"] == 0
    _same_outputs(out1, base)
    di = device_index()
    di.set_scaffolds(genome())
    di.set_scaffolds(None)
    outc, _, _ = _map(reads, paired, None)
    _same_outputs(outc, base)


def test_overflow_tier_applies_the_filter():
    """max_sites too small for many reads: the tier (reserved[1..2]) maps them again from the probe on, with the same table"""
    reads, _, _ = _read_sets(False, 7)
    tab = SC.table_of(genome())
    out, st, recs = _map(reads, False, "packed", max_sites=1, reserved=(C.c_int32 * 4)(0, 4096, 256, 0))
    assert st["reads_reprobed"] > 0 and st["reads_overflowed"] == 0
    _assert_no_spanning(out, tab)
    per = _probe(reads, False)
    assert st["sites_cross_scaffold"] == int(per.sum()) > 0
    want = SC.scaffold_records(tab, out["final"], _final_strings(out), False)
    assert np.array_equal(recs, want)


def test_pacbio_pieces_straddling_scaffolds():
    p = genome()
    rng = np.random.default_rng(5)
    sb = p.scaffold_bases()
    nexts = [g for g in range(len(sb) - 1) if sb[g + 1][0] == sb[g][0] and sb[g][2] >= 600 and sb[g + 1][2] >= 600]
    pieces = []
    for i in range(60):
        g = int(rng.choice(nexts))
        (c, a, n), (_, b, m) = sb[g], sb[g + 1]
        h, t = int(rng.integers(200, 600)), int(rng.integers(200, 600))
        if i % 3 == 0:                                        # a piece that simply lies inside scaffold A
            pieces.append(np.asarray(p.chroms[c - 1][a: a + h + t], np.uint8))
        else:
            pieces.append(np.concatenate([p.chroms[c - 1][a + n - h: a + n], p.chroms[c - 1][b: b + t]]))
    di = DeviceIndex.build(p.chroms, profile=PROFILE_PACBIO)
    try:
        recs, blob, bs, ki = K.make_batch(pieces, None, K.default_config(K.PROFILE_PACBIO))
        di.set_scaffolds(p)
        mp = Mapper.from_records(di, recs, blob, bs, ki, max_sites=256, profile=PROFILE_PACBIO, finalStage=1)
        mp.step()
        out, st = mp.fetch(), mp.stats()
        srecs, _ = mp.scaffold_records()
        mp.close()
        tab = SC.table_of(p)
        assert st["reads_overflowed"] == 0 and st["reads_reprobed"] == 0
        _assert_no_spanning(out, tab)
        reads = []
        for r in recs:
            o, ln, ko, nk = int(r["bases_off"]), int(r["len"]), int(r["keys_off"]), int(r["nkeys"])
            reads.append((blob[o: o + ln], bs[o: o + ln], ki[ko + nk: ko + 2 * nk], ki[ko: ko + nk]))
        lists, ns = di.find_batch(reads, max_sites=256, codes=True)
        assert (ns >= 0).all()
        lens = [len(c) for c in p.chroms]
        span = sum(1 for lst in lists for s in lst if s["start"] >= 0 and s["stop"] <= lens[s["chrom"] - 1] - 1
                   and not SC.is_single_scaffold(tab[0], tab[2], s["chrom"], s["start"], s["stop"]))
        assert st["sites_cross_scaffold"] == span > 0
        want = SC.scaffold_records(tab, out["final"], _final_strings(out), False)
        assert np.array_equal(srecs, want)
    finally:
        di.close()


def test_malformed_tables_are_rejected_and_the_old_one_stays():
    di = device_index()
    p = genome()
    reads, _, _ = _read_sets(False, 9)
    offs, ks = _offs()
    di.set_scaffolds(p)
    mp = Mapper(di, len(reads), L, offs, ks, paired=False, max_sites=64)
    mp.load_reads(reads)
    mp.step()
    st_a, rec_a = mp.stats()["sites_cross_scaffold"], mp.scaffold_records()[0]
    assert st_a > 0
    Lb = di.L
    nc = p.nchroms

    def call(locs, lens, counts=None, pad=300, nchroms=nc):
        la = [np.ascontiguousarray(a, np.int32) for a in locs]
        lb = [np.ascontiguousarray(a, np.int32) for a in lens]
        cnt = np.array([0] + ([len(a) for a in la] if counts is None else counts), np.int32)
        lp = (C.c_void_p * (len(la) + 1))(*([0] + [a.ctypes.data if len(a) else 0 for a in la]))
        ln = (C.c_void_p * (len(lb) + 1))(*([0] + [a.ctypes.data if len(a) else 0 for a in lb]))
        return Lb.bbidx_set_scaffolds(di.h, nchroms, cnt.ctypes.data, lp, ln, pad)

    good_l, good_n = [a.copy() for a in p.locs], [a.copy() for a in p.lengths]
    bad = []
    l = [a.copy() for a in good_l]; l[1][2] = l[1][1]; bad.append((l, good_n))                 # not strictly ascending
    l = [a.copy() for a in good_l]; l[0][1], l[0][2] = l[0][2], l[0][1]; bad.append((l, good_n))   # descending
    n_ = [a.copy() for a in good_n]; n_[2][-1] = len(p.chroms[2]); bad.append((good_l, n_))   # past chromArrLen
    l = [a.copy() for a in good_l]; l[0][0] = -1; bad.append((l, good_n))                     # negative start
    for l, n_ in bad:
        assert call(l, n_) == -2
    assert call(good_l, good_n, pad=0) == -2                  # padding <= 0 with multi-scaffold chromosomes
    assert call(good_l, good_n, pad=-5) == -2
    assert call(good_l, good_n, nchroms=nc + 1) == -2         # not the index's chromosome count
    assert call(good_l, good_n, counts=[len(good_l[0]), 0, len(good_l[2])]) == -2
    mp.step()                                                 # the table in force is still the good one
    st_b, rec_b = mp.stats()["sites_cross_scaffold"], mp.scaffold_records()[0]
    assert st_b == st_a and np.array_equal(rec_a, rec_b)
    di.set_scaffolds(None)
    p0 = C.c_void_p()
    assert mp.L.bbmap_get_scaffold_records(mp.h, None, C.byref(p0)) == -2        # no table
    mp.step()
    assert mp.stats()["sites_cross_scaffold"] == 0
    mp.close()
    di.set_scaffolds(p)
    m0 = Mapper(di, len(reads), L, offs, ks, paired=False, max_sites=64, finalStage=0)
    m0.load_reads(reads)
    m0.step()
    assert m0.L.bbmap_get_scaffold_records(m0.h, None, C.byref(p0)) == -2        # no final stage
    m0.close()
    di.set_scaffolds(None)
