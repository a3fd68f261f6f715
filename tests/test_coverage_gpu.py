"""Coverage on the device (bbmap_cov_* / bbpipe_coverage_*) against the sequential restatement of jgi.CoveragePileup
(tests/coverage_check.py): every integer the device returns equals the restatement's; the floats bbmap_amd.coverage derives from
them equal the restatement's float64 loops to 1e-9 relative (the device's moments are exact integers, so this only allows for the
order of the host's sums).  Raw form over planted records first, then the context form over mapped reads."""
import ctypes as C

import numpy as np
import pytest
import torch

from bbmap_amd import _lib
from bbmap_amd import coverage as V
from bbmap_amd.index import DeviceIndex, READ_DTYPE
from bbmap_amd.mapper import FINAL_DTYPE, Mapper
from tests import coverage_check as K
from tests import scaffold_check as SC
from tests.test_runstats_gpu import _load, _mapper, _pairs, _restate, genome

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 300
SYMS = np.frombuffer(b"mmmmmmmmmmmmSSDIXYNC", np.uint8)
READ_SYMS = np.frombuffer(b"ACGTACGTACGTNacgtnU", np.uint8)
ALL_FLAGS = [0, V.COV_START_ONLY, V.COV_EXCLUDE_DELETIONS, V.COV_START_ONLY | V.COV_EXCLUDE_DELETIONS, V.COV_STRANDED,
             V.COV_STRANDED | V.COV_START_ONLY, V.COV_STRANDED | V.COV_EXCLUDE_DELETIONS, V.COV_32BIT,
             V.COV_32BIT | V.COV_STRANDED | V.COV_EXCLUDE_DELETIONS]
T, M = V.COV_SCAN_TILE, V.COV_MEDIAN_SHORT
# three scaffolds on chromosome 1, 300 apart, and a single-scaffold chromosome: lengths 1 / 63 / 64 / 65; one each side of the scan's
# tile and one spanning three tiles; one each side of the median's one-workgroup limit
# "chunk": a short scaffold and a long one each lying across a boundary of the statistics pass's 65,536-slot chunks on purpose
CH = V.COV_STATS_CHUNK
GEOMETRIES = {"tiny": ([1, 63, 64], [65]), "tiles": ([T - 2, T, 2 * T + 10], [65]), "median": ([M, 65, M + 1], [64]),
              "chunk": ([CH - 10, 30, CH + 5], [64])}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _table(chrom_lengths, first=1000):
    """(locs, lengths, pad, base): every chromosome's scaffolds PAD apart, the first one at `first`"""
    locs, lengths, base, acc = [None], [None], [0], 0
    for ls in chrom_lengths:
        at, lo = first, []
        for n in ls:
            lo.append(at)
            at += n + PAD
        locs.append(lo); lengths.append(list(ls)); base.append(acc)
        acc += len(ls)
    return locs, lengths, PAD, base


STRINGS = [b"m", b"m" * 63, b"m" * 64, b"m" * 65, b"m" * 129,
           b"m" * 70,                                       # an m run across a 64-symbol step
           b"m" * 60 + b"D" * 10 + b"m" * 10,               # a D run across one
           b"m" * 5 + b"D" * 256 + b"m" * 5,                # 2 x 128 D: an expanded gap
           b"C" * 3 + b"m" * 20, b"X" * 2 + b"m" * 20, b"I" * 2 + b"m" * 20,
           b"mD" * 40, b"m" * 63 + b"D" + b"m" * 63 + b"I" * 64 + b"S" * 3 + b"N" * 2,
           b"I" * 64 + b"m" * 3, b"m" * 64 + b"D" * 64 + b"I" * 64 + b"m" * 64, None]


def _planted(table, rng, extra=120):
    """[(mapped, chrom, start, stop, strand, bases, match)]: every edge of the issue's list on every scaffold, each with a string of
    STRINGS in turn, then random records"""
    locs, lengths, _, _ = table
    out, k = [], 0

    def put(mapped, chrom, start, stop, match="next"):
        nonlocal k
        if match == "next":
            match = STRINGS[k % len(STRINGS)]
            k += 1
        n = int(rng.integers(1, 200))
        out.append((mapped, chrom, int(start), int(stop), int(rng.integers(0, 2)), READ_SYMS[rng.integers(0, len(READ_SYMS), n)].tobytes(), match))

    put(0, -1, -1, -1, None)                                                    # unmapped
    for c in range(1, len(locs)):
        for i, (a, n) in enumerate(zip(locs[c], lengths[c])):
            if i + 1 < len(locs[c]):
                put(1, c, a + n - 1, locs[c][i + 1] + 1)                        # spans two scaffolds: readsProcessed only
            put(1, c, a - 5, a + min(n, 10) - 1)                                # starts in the pad: clamped to 0
            put(1, c, a - 2, a + min(n, 150) - 1, b"m" * 152)                   # the clamped-start quirk with a string that fits the span
            put(1, c, a + max(0, n - 3), a + n + 5)                             # ends past the scaffold: clamped
            put(1, c, a - 8, a - 5)                                             # wholly in the left pad: negative basehits, no depth
            put(1, c, a + n // 2, a + n // 2)                                   # start == stop
            put(1, c, a, a + n - 1)                                             # the whole scaffold: the -1 lands in the extra slot
            put(1, c, a, a + n - 1, b"m" * n if n < 5000 else None)
            put(1, c, a, a + min(n, 200) - 1, b"m" * 20)                        # the string ends before stop
            put(1, c, a + n // 3, a + n // 3 + min(n, 30) - 1, b"m" * 300)      # cut by rpos > stop
            put(1, c, a + n + 2, a + n + 6)                                     # wholly right of the scaffold
            for _ in range(len(STRINGS)):
                s = a + int(rng.integers(0, n))
                put(1, c, s, s + int(rng.integers(0, 140)))
            for _ in range(extra):
                s = a + int(rng.integers(-20, n + 10))
                ml = int(rng.integers(1, 260))
                put(1, c, s, s + int(rng.integers(0, 200)), SYMS[rng.integers(0, len(SYMS), ml)].tobytes() if rng.random() < 0.9 else None)
    return out


def _upload(records):
    n = len(records)
    fin, reads = np.zeros(n, FINAL_DTYPE), np.zeros(n, READ_DTYPE)
    pool, bases = [np.zeros(3, np.uint8)], []
    poff, boff = 3, 0
    for r, (mapped, chrom, start, stop, strand, b, m) in enumerate(records):
        f = fin[r]
        f["mapped"], f["chrom"], f["strand"], f["start"], f["stop"] = mapped, chrom, strand, start, stop
        if m:
            f["match_len"], f["match_off"] = len(m), poff
            pool.append(np.frombuffer(m, np.uint8)); poff += len(m)
        reads[r]["len"], reads[r]["bases_off"] = len(b), boff
        bases.append(np.frombuffer(b, np.uint8)); boff += len(b)
    return _dev(reads), _dev(np.concatenate(bases + [np.zeros(1, np.uint8)])), _dev(fin), _dev(np.concatenate(pool))


def _restatement(table, flags, records, paired=False, p=None):
    p = p or K.Pileup(table, flags)
    for mapped, chrom, start, stop, strand, b, m in records:
        p.process_read(bool(mapped), chrom, start, stop, strand, b, m, 1 if paired else 0)
    return p


def _close(a, b):
    return a == b or abs(a - b) <= 1e-9 * max(abs(a), abs(b))


def _sumsq(d):
    return sum(int(x) * int(x) for x in d)


def _compare(cov, p, binsize=0, floats=True):
    """every integer of the view against the restatement; then the derived floats"""
    t = cov.totals
    assert (int(t["readsProcessed"]), int(t["mappedReads"]), int(t["mappedBases"]), int(t["refBases"])) == \
        (p.readsProcessed, p.mappedReads, p.mappedBases, p.refBases)
    assert len(cov.recs) == len(p.list) and cov.strands == (2 if p.flags & K.STRANDED else 1)
    for g, s in enumerate(p.list):
        r = cov.recs[g]
        got = (int(r["length"]), int(r["basehits"]), int(r["readhits"]), int(r["readhitsMinus"]), int(r["fraghits"]), [int(x) for x in r["readBases"]])
        assert got == (s.length, s.basehits, s.readhits, s.readhitsMinus, s.fraghits, s.basecount[:4]), (g, got)
        for st in range(cov.strands):
            want = p.depth(s, st)
            a = int(cov.covoff[g])
            have = cov.depth[st][a:a + s.length + 1].astype(np.int64)
            assert np.array_equal(have, want), (g, st, np.flatnonzero(have != want)[:8])
            assert want[s.length] == 0                       # the extra slot
            d = want[:s.length]
            rs = r["strand"][st]
            assert (int(rs["covered"]), int(rs["median"]), int(rs["max"]), int(rs["sumDepth"])) == \
                (int(np.count_nonzero(d)), p.median(s, st), int(d.max()), int(d.sum())), (g, st)
            assert (int(rs["sumSqHi"]) << 64) | int(rs["sumSqLo"]) == _sumsq(d)
            if floats and s.obj[st] is not None:
                assert _close(V.scaffold_stdev(r, st), K.standard_deviation(want))
    for st in range(cov.strands):
        assert np.array_equal(cov.hist[st], p.device_hist(st))
        if binsize:
            assert np.array_equal(cov.bins[st], p.bin_sums(binsize, st))
            if floats:
                assert all(_close(x, y) for x, y in zip(V.binned_mean_stdev(cov, st), p.standard_deviation_binned(binsize, st)))
        if floats:
            assert all(_close(x, y) for x, y in zip(V.global_stdev(cov, st), p.standard_deviation(st)))


# ------------------------------------------------------------------------------------------------ the raw form, planted records
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_planted_records_every_flag_and_geometry(geo, flags):
    table = _table(GEOMETRIES[geo])
    records = _planted(table, np.random.default_rng(len(geo) * 100 + flags))
    p = _restatement(table, flags, records)
    state = V.DeviceState(table, flags)
    state.add(*_upload(records))
    big = geo != "tiny"
    # binsize 1, one that leaves a short last bin of 1 (65 = 64 + 1, T + ... ), and one larger than every scaffold
    for binsize in ([1, 64, 100000] if not big else [T - 3 if geo == "tiles" else M if geo == "median" else CH + 4]):
        cov = state.finalize(binsize)                        # (every finalize is a snapshot of the same state)
        _compare(cov, p, binsize, floats=not big or flags in (0, V.COV_32BIT))
    if not big:                                             # the text, character for character
        for st in range(cov.strands):
            lines, hist = p.write_stats(st)
            assert V.covstats_lines(cov, st) == lines and V.covhist_lines(cov, st) == p.write_hist(hist)
            assert V.bincov_lines(cov, st) == p.write_binned(100000, st) and V.basecov_lines(cov, st) == p.write_coverage_per_base(st)
        p.write_stats(0)
        assert V.summary_lines(cov) == p.summary()
    s = sum(x.readhits for x in p.list)
    assert s > 100 and any(x.basehits < 0 or x.readhits for x in p.list) and p.readsProcessed > p.mappedReads > 0


def test_more_scaffolds_than_the_lds_counters_hold():
    """above COV_LDS_SCAFFOLDS the accumulate kernel adds to the records in HBM directly"""
    rng = np.random.default_rng(5)
    table = _table([list(rng.integers(1, 40, V.COV_LDS_SCAFFOLDS + 30)), [50]])
    for flags in (0, V.COV_STRANDED | V.COV_EXCLUDE_DELETIONS):
        records = _planted(table, rng, extra=2)
        state = V.DeviceState(table, flags)
        state.add(*_upload(records))
        _compare(state.finalize(7), _restatement(table, flags, records), 7, floats=False)


def test_midpoint_rule_truncates_toward_zero():
    """scaffoldIndex(chrom, (start + stop) / 2) with Java's division: -3 / 2 = -1, so -4..1 has key -1 + 150 = 149, scaffold 1's start
    exactly (floor division would give 148 and scaffold 0); 240..259 has mid 499 / 2 = 249, key 399: scaffold 1, not scaffold 2 at 400"""
    table = ([None, [0, 149, 400]], [None, [5, 20, 30]], PAD, [0, 0])
    records = [(1, 1, -4, 1, 0, b"ACGT", b"mmmm"), (1, 1, 240, 259, 1, b"ACGTA", None)]
    for flags in (0, V.COV_EXCLUDE_DELETIONS):
        p = _restatement(table, flags, records)
        assert [s.readhits for s in p.list] == [0, 2, 0] and p.list[1].basehits == (-147 - 71 if flags == 0 else 0)
        state = V.DeviceState(table, flags)
        state.add(*_upload(records))
        _compare(state.finalize(4), p, 4)


@pytest.mark.parametrize("flags", [0, V.COV_32BIT])
def test_saturation(flags):
    """66,000 identical records on a 65-base scaffold: 65,535 in 16-bit mode, 66,000 in 32-bit mode; basehits does not saturate.
    The second scaffold stays shallow: LDS sub-histogram and HBM histogram bins in one run."""
    table = _table([[65, 40], [3]])
    n = 66000
    records = [(1, 1, 1000, 1064, 0, b"AC", None)] * n + [(1, 1, 1000 + 65 + PAD + 3, 1000 + 65 + PAD + 9, 1, b"G", None)] * 5
    p = _restatement(table, flags, records)
    depth = 66000 if flags else 65535
    assert int(p.depth(p.list[0]).max()) == depth and p.list[0].basehits == 65 * n
    state = V.DeviceState(table, flags)
    state.add(*_upload(records))
    cov = state.finalize(64)
    _compare(cov, p, 64, floats=False)
    assert int(cov.hist[0][depth]) == 65 and int(cov.hist[0][5]) == 7 and depth > V.COV_HIST_LDS_BINS
    assert int(cov.recs[0]["strand"][0]["sumDepth"]) == 65 * depth and int(cov.recs[0]["basehits"]) == 65 * n
    assert V.covstats_lines(cov)[1].split("\t")[1] == K.jfmt(n, 4)                   # Avg_fold comes from basehits, as in Java


@pytest.mark.parametrize("n,paired", [(1, False), (2, True), (2 * V.COV_MAX_WAVES + 1, False), (2 * V.COV_MAX_WAVES + 2, True)])
def test_read_counts_and_the_persistent_loop(n, paired):
    table = _table(GEOMETRIES["tiny"])
    rng = np.random.default_rng(n)
    records = (_planted(table, rng, extra=4200) * 2)[:n] if n > 2 else [(1, 1, 1301, 1320, 1, b"ACGTN", b"mmDm")] * n
    assert len(records) == n
    flags = V.COV_EXCLUDE_DELETIONS | V.COV_STRANDED
    p = _restatement(table, flags, records, paired)
    state = V.DeviceState(table, flags)
    state.add(*_upload(records), paired=paired)
    _compare(state.finalize(16), p, 16, floats=False)
    assert sum(s.fraghits for s in p.list) == p.mappedReads * (1 if paired else 2) and p.readsProcessed == n


def test_accumulation_goes_on_after_a_finalize():
    table = _table(GEOMETRIES["tiles"])
    rng = np.random.default_rng(8)
    one, two = _planted(table, rng, extra=10), _planted(table, rng, extra=10)
    state = V.DeviceState(table, 0)
    state.add(*_upload(one))
    p = _restatement(table, 0, one)
    _compare(state.finalize(100), p, 100, floats=False)
    state.add(*_upload(two))
    _compare(state.finalize(100), _restatement(table, 0, two, p=p), 100, floats=False)


def test_raw_calls_reject_bad_arguments():
    L = _lib.load()
    assert L.bbpipe_coverage_add_device(None, -1, 0, 0, *([None] * 4), 1, 1, None, None, None, 0, *([None] * 5)) == -2
    assert L.bbpipe_coverage_add_device(None, 1, 0, 16, *([None] * 4), 1, 1, None, None, None, 0, *([None] * 5)) == -2
    assert L.bbmap_last_error() == b"bbpipe_coverage_add_device: unknown flag bits"
    assert L.bbpipe_coverage_add_device(None, 1, 0, 0, *([None] * 4), 1, 1, None, None, None, 0, *([None] * 5)) == -2
    assert L.bbmap_last_error() == b"bbpipe_coverage_add_device: null buffer"
    assert L.bbpipe_coverage_finalize_device(None, 0, 0, 0, *([None] * 10), 0, None, 0, *([None] * 4), 0) == -2
    assert L.bbpipe_coverage_workspace_bytes(-1, 0) == -2
    lens = np.array([3, 0], np.int32)
    assert L.bbpipe_coverage_layout(2, lens.ctypes.data, 0, None, None) == -2
    covoff, binoff = V.layout([1, 63, 64, 65], 64)
    assert list(covoff) == [0, 2, 66, 131, 197] and list(binoff) == [0, 1, 2, 3, 5]


# ------------------------------------------------------------------------------------------------ the context form, mapped reads
def _refcounts(packed):
    out = []
    for c, a, n in packed.scaffold_bases():
        seg = packed.chroms[c - 1][a:a + n]
        out.append(tuple(int(np.count_nonzero((seg == ord(x)) | (seg == ord(x.lower())))) for x in "ACGT"))
    return out


def _pileup_of(mp, reads, paired, packed, flags=0, p=None):
    fin, matches, _, _ = _restate(mp, reads, paired, None)
    p = p or K.Pileup(SC.table_of(packed), flags, packed.scaffold_names(), _refcounts(packed))
    p.add_batch(fin, matches, [bytes(r) if isinstance(r, (bytes, bytearray)) else np.asarray(r, np.uint8).tobytes() for r in reads], paired)
    return p, fin


def _compare_context(cov, p, binsize):
    _compare(cov, p, binsize)
    for g, s in enumerate(p.list):
        assert [int(x) for x in cov.recs[g]["refBases"]] == s.refcount
    lines, hist = p.write_stats(0)
    assert V.covstats_lines(cov) == lines and V.covhist_lines(cov) == p.write_hist(hist)
    assert V.bincov_lines(cov) == p.write_binned(binsize) and V.summary_lines(cov) == p.summary()


@pytest.mark.parametrize("paired", [True, False])
def test_mapped_reads_default_flags(paired):
    reads, _ = _pairs(300, 1 if paired else 2)
    di, mp = _mapper(reads, paired, max_sites=64)
    try:
        mp.enable_coverage(V.COV_32BIT)
        mp.enable_coverage(V.COV_32BIT)                      # the same flags over the same table: nothing changes
        assert mp.L.bbmap_add_coverage(mp.h, None) == -2     # no batch has been mapped yet
        mp.step()
        mp.add_coverage()
        cov = mp.coverage(1000)
        p, fin = _pileup_of(mp, reads, paired, genome(), V.COV_32BIT)
        _compare_context(cov, p, 1000)
        # ---- independent of the restatement (32-bit mode: nothing saturates)
        recs = cov.recs
        assert int(recs["strand"]["sumDepth"][:, 0].sum()) == int(recs["basehits"].sum()) > 0
        assert int(cov.hist[0].sum()) == int(recs["length"].sum()) == int(cov.totals["refBases"])
        assert int(recs["strand"]["covered"][:, 0].sum()) == sum(int(np.count_nonzero(cov.scaffold_depth(s))) for s in range(len(recs)))
        assert int(recs["readhits"].sum()) == int(cov.totals["mappedReads"]) > 300
        assert int(recs["fraghits"].sum()) == int(cov.totals["mappedReads"]) * (1 if paired else 2)
        assert int(cov.totals["readsProcessed"]) == len(reads)
        host = mp.coverage_host(1000)                       # bbmap_get_coverage gives the same snapshot
        assert host.recs.tobytes() == cov.recs.tobytes() and host.totals.tobytes() == cov.totals.tobytes()
        assert all(np.array_equal(a, b) for a, b in zip(host.depth + host.hist + host.bins, cov.depth + cov.hist + cov.bins))
    finally:
        mp.close()
        di.close()


def test_two_steps_finalize_between_and_reset():
    reads, _ = _pairs(200, 3)
    di, mp = _mapper(reads, True, max_sites=64)
    try:
        mp.enable_coverage(0)
        mp.step()
        mp.add_coverage()
        p, _ = _pileup_of(mp, reads, True, genome())
        _compare(mp.coverage(500), p, 500, floats=False)     # a finalize between the two steps changes nothing
        assert mp.L.bbmap_add_coverage(mp.h, None) == -2     # a second count of one step
        assert mp.L.bbmap_last_error() == b"bbmap_add_coverage: the last batch has been counted already"
        reads2, _ = _pairs(200, 13)
        _load(mp, reads2)
        mp.step()
        mp.add_coverage()
        p, _ = _pileup_of(mp, reads2, True, genome(), p=p)
        _compare_context(mp.coverage(500), p, 500)
        mp.reset_coverage()
        zero = mp.coverage(500)
        assert not any(int(zero.totals[k]) for k in ("readsProcessed", "mappedReads", "mappedBases"))
        assert not zero.depth[0].any() and not zero.bins[0].any() and int(zero.hist[0][0]) == int(zero.totals["refBases"])
        assert not any(int(zero.recs[k].sum()) for k in ("basehits", "readhits", "readhitsMinus", "fraghits", "readBases"))
        assert int(zero.recs["refBases"].sum()) > 0          # the reference's own counts stay
        mp.add_coverage()                                   # after a reset the batch the context holds may be added again
        again = mp.coverage(500)
        assert int(again.totals["readsProcessed"]) == len(reads2) and int(again.recs["readhits"].sum()) == int(again.totals["mappedReads"]) > 0
    finally:
        mp.close()
        di.close()


def test_overflow_tier_records_are_counted():
    reads, _ = _pairs(300, 3)
    di, mp = _mapper(reads, True, max_sites=1, reserved=(C.c_int32 * 4)(0, 4096, 256, 0))
    try:
        mp.enable_coverage(V.COV_EXCLUDE_DELETIONS | V.COV_STRANDED)
        mp.step()
        assert mp.stats()["reads_reprobed"] > 0
        mp.add_coverage()
        p, _ = _pileup_of(mp, reads, True, genome(), V.COV_EXCLUDE_DELETIONS | V.COV_STRANDED)
        _compare(mp.coverage(1000), p, 1000)
    finally:
        mp.close()
        di.close()


def test_phix_pairs():
    from tests.golden_phix import fixture_inputs, fixture_runs, phix_reference
    ref = phix_reference()
    body = int(len(ref)) - 16000

    class OneScaffold:
        chroms, locs, lengths, names, inter_scaffold_padding = [ref], [[8000]], [[body]], [["phix"]], PAD
        nchroms = 1
        scaffold_names = staticmethod(lambda: ["phix"])
        scaffold_bases = staticmethod(lambda: [(1, 8000, body)])

    di = DeviceIndex.build([ref], k=13)
    di.set_scaffolds(OneScaffold)
    try:
        name, r = next((k, v) for k, v in fixture_runs().items() if v["inputs"][4])
        recs, blob, bs, ki, paired = r["inputs"]
        reads, _, _ = fixture_inputs(name.split("_")[0], name.endswith("_qual"))
        mp = Mapper.from_records(di, recs, blob, bs, ki, paired=True, max_sites=32)
        try:
            mp.enable_coverage(0)
            mp.step()
            mp.add_coverage()
            cov = mp.coverage(1000)
            p, fin = _pileup_of(mp, reads, True, OneScaffold)
            _compare_context(cov, p, 1000)
            lines = V.covstats_lines(cov)
            assert len(lines) == 2
            f = lines[1].split("\t")
            assert f[0] == "phix" and int(f[6]) + int(f[7]) == int(np.count_nonzero(fin["mapped"])) > 0
        finally:
            mp.close()
    finally:
        di.close()


def test_refusals():
    reads, _ = _pairs(20, 5)
    di, mp = _mapper(reads, True, max_sites=64, finalStage=0)
    try:
        assert mp.L.bbmap_cov_enable(mp.h, 0) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_cov_enable: the context runs without the final stage (bbmap_config.finalStage)"
    finally:
        mp.close()
        di.close()
    di, mp = _mapper(reads, True, max_sites=64)
    try:
        assert mp.L.bbmap_cov_enable(mp.h, 16) == -2 and mp.L.bbmap_last_error() == b"bbmap_cov_enable: unknown flag bits"
        assert mp.L.bbmap_add_coverage(mp.h, None) == -2 and mp.L.bbmap_last_error() == b"bbmap_add_coverage: coverage is not enabled (bbmap_cov_enable)"
        di.set_scaffolds(None)
        assert mp.L.bbmap_cov_enable(mp.h, 0) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_cov_enable: the index has no scaffold table (bbidx_set_scaffolds)"
        p = genome()
        di.set_scaffolds(p)
        mp.enable_coverage(0)
        assert mp.L.bbmap_cov_enable(mp.h, V.COV_STRANDED) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_cov_enable: coverage is enabled already with other flags"

        class FirstOnly:                                    # a table of another size: every chromosome's first scaffold alone
            locs, lengths, names = [a[:1] for a in p.locs], [a[:1] for a in p.lengths], None
            inter_scaffold_padding = p.inter_scaffold_padding

        di.set_scaffolds(FirstOnly)
        assert mp.L.bbmap_cov_enable(mp.h, 0) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_cov_enable: the scaffold table has been replaced since coverage was enabled"
        mp.step()
        assert mp.L.bbmap_add_coverage(mp.h, None) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_add_coverage: the scaffold table has been replaced since coverage was enabled"
        view = V.bbmap_cov_view()
        assert mp.L.bbmap_cov_finalize(mp.h, None, C.c_int32(0), C.byref(view)) == -2
        assert mp.L.bbmap_last_error() == b"bbmap_cov_finalize: the scaffold table has been replaced since coverage was enabled"
    finally:
        mp.close()
        di.close()
