"""GPU tests of the BBMap-profile mapper on pairs whose mates differ in length and on mixed-length single-ended batches, against the
CPU restatement (oracle/mapper_oracle.c, which carries len1 and len2 apart as BBMapThread.processReadPair does): site lists, every
fill's window / minScore / scores / iterations / traceback string, final records and match strings (tests/mapper_check.py: compare).
The inputs and the coverage conditions are tests/pair_problems.py's; tests/test_oracle_pairs.py pins the oracle's side of them, and
its table holds the counts both sides reach.

What writing these tests found (by reading the code the (150,11) class runs): the probe leaves a read without keys alone, its
reverse complement included, and the mapper never wrote it -- rescue searched a mate shorter than k on the minus strand in whatever
the buffer held.  revcomp_unprobed_kernel writes those strands now; with it the device rescues the oracle's 58 of 110."""
import numpy as np
import pytest

from bbmap_amd import reference as R
from bbmap_amd import runstats as RS
from bbmap_amd import workload as W
from bbmap_amd.index import DeviceIndex
from bbmap_amd.mapper import Mapper
from tests import pair_problems as PP
from tests import runstats_check as RC
from tests.mapper_check import DP_ROUTES, compare, set_route

pytestmark = pytest.mark.gpu


def _device_coverage(out, b):
    return PP.coverage(RC.merged_site_lists(out), PP.device_rescue_reads(out), b["truth"]["len"], b["cls"])


@pytest.mark.parametrize("route", sorted(DP_ROUTES))
def test_unequal_mates_match_oracle(monkeypatch, route):
    set_route(monkeypatch, route)
    b, orc = PP.pair_batch(), PP.pair_oracle()
    n = len(b["reads"])
    di = DeviceIndex.build([b["ref"]], k=PP.K_TEST)
    mp = Mapper.from_records(di, *b["records"], paired=True, max_sites=32)
    try:
        mp.step()
        out, st = mp.fetch(), mp.stats()
    finally:
        mp.close()
        di.close()
    assert st["reads_overflowed"] == 0 and "overflow" not in out
    bad = compare(out, orc, n, paired=True)
    assert not bad, "%d differences\n" % len(bad) + "\n".join(bad[:20])
    # the coverage conditions, on what the DEVICE returned
    cov = _device_coverage(out, b)
    print({k: v for k, v in cov.items() if k != "classes"}, {k: st[k] for k in ("rescue_scans", "rescue_fills", "fills", "gapped_fills", "rounds")})
    for c, d in cov["classes"].items():
        print(c, d)
    assert not PP.check_coverage(cov), PP.check_coverage(cov)
    assert st["rescue_scans"] == orc["stats"][2] and st["rescue_scans"] > 200
    assert st["rescue_fills"] == cov["fills_anchor_longer"] + cov["fills_anchor_shorter"] + cov["fills_equal"] == len(PP.oracle_rescue_reads(orc))
    assert cov["rescued_anchor_longer"] >= 20 and cov["rescued_anchor_shorter"] >= 20
    if route == "throughput":
        assert st["dp_narrow_launches"] > 0, st                      # the route really ran
    else:
        assert st["dp_narrow_launches"] == 0 and st["dp_sorted_launches"] == 0, st


def test_unequal_mates_on_one_context_after_equal_ones():
    """Per-context state sized or cached by the first batch's length: an all-150 batch, then the trimmed one (up to 151 bases), on ONE
    context; each equals its oracle run."""
    b = PP.pair_batch()
    eq_reads, eq_records = PP.equal_batch()
    di = DeviceIndex.build([b["ref"]], k=PP.K_TEST)
    mp = Mapper.from_records(di, *eq_records, paired=True, max_sites=32, max_reads=len(b["reads"]), max_read_len=PP.DRAW_LEN)
    try:
        for name, records, n, orc in (("equal", eq_records, len(eq_reads), PP.oracle_map(b["ref"], *eq_records, paired=True)),
                                      ("trimmed", b["records"], len(b["reads"]), PP.pair_oracle())):
            mp.load_records(*records)
            mp.step()
            out, st = mp.fetch(), mp.stats()
            assert st["reads_overflowed"] == 0 and st["reads"] == n and len(out["nsites"]) == n
            bad = compare(out, orc, n, paired=True)
            assert not bad, "%s batch: %d differences\n" % (name, len(bad)) + "\n".join(bad[:20])
            assert st["rescue_fills"] > 10
    finally:
        mp.close()
        di.close()


def test_unequal_mates_through_the_overflow_tier():
    """max_sites = 4 on a repeat-rich reference: pairs whose lists do not fit are mapped again by the overflow tier, as pairs, with each
    mate's own length."""
    ref = W.make_reference(200000, seed=11, pad=2000, repeat_frac=0.6, families=3)
    reads, cls, truth = PP.trimmed_pairs(ref, 700, seed=2, classes=((150, 100), (100, 150), (150, 36)))
    records = PP.make_records(reads)
    n = len(reads)
    orc = PP.oracle_map(ref, *records, paired=True, cap=1024)
    di = DeviceIndex.build([ref], k=PP.K_TEST)
    mp = Mapper.from_records(di, *records, paired=True, max_sites=4)
    try:
        mp.step()
        out, st = mp.fetch(), mp.stats()
    finally:
        mp.close()
        di.close()
    moved = out["nsites"] == -3
    assert st["reads_overflowed"] == 0 and (out["nsites"] >= -3).all() and not (out["nsites"] == -1).any()
    assert moved.sum() == st["reads_reprobed"] > 20
    t = out["overflow"]
    assert sorted(t["read_ids"].tolist()) == np.nonzero(moved)[0].tolist()
    assert (t["read_ids"][0::2] % 2 == 0).all() and (t["read_ids"][1::2] == t["read_ids"][0::2] + 1).all()       # mates travel together
    assert int(t["nsites"].max()) > 4
    moved_classes = {cls[int(r) // 2] for r in t["read_ids"]}
    assert len(moved_classes) == 3, moved_classes
    bad = compare(out, orc, n, paired=True)
    assert not bad, "%d differences\n" % len(bad) + "\n".join(bad[:20])


@pytest.mark.parametrize("route", sorted(DP_ROUTES))
def test_mixed_single_ended_batch_matches_oracle(monkeypatch, route):
    set_route(monkeypatch, route)
    ref = W.make_reference(300000, seed=5, pad=2000, repeat_frac=0.15)
    reads, truth = PP.mixed_single(ref, 3000, seed=9)
    records = PP.make_records(reads)
    n = len(reads)
    orc = PP.oracle_map(ref, *records, paired=False)
    di = DeviceIndex.build([ref], k=PP.K_TEST)
    mp = Mapper.from_records(di, *records, paired=False, max_sites=32)
    try:
        mp.step()
        out, st = mp.fetch(), mp.stats()
    finally:
        mp.close()
        di.close()
    assert st["reads_overflowed"] == 0
    bad = compare(out, orc, n, paired=False)
    assert not bad, "%d differences\n" % len(bad) + "\n".join(bad[:20])
    mapped = {int(ln): int(((truth["len"] == ln) & (out["final"]["mapped"] > 0)).sum()) for ln in PP.MIXED_LENS}
    present = {int(ln): int((truth["len"] == ln).sum()) for ln in PP.MIXED_LENS}
    print(mapped, {k: st[k] for k in ("fills", "gapped_fills", "rounds", "dp_narrow_launches", "dp_sorted_launches")})
    assert all(present[ln] == n // len(PP.MIXED_LENS) for ln in PP.MIXED_LENS)
    assert all(mapped[ln] > 0 for ln in PP.MIXED_LENS if ln > 14), mapped
    top = out["sites"][:, 0]
    at_truth = (out["nsites"] > 0) & (np.abs(top["start"] - truth["start"]) <= 40) & (top["strand"] == 0)
    assert at_truth[truth["len"] >= 35].mean() > 0.9                  # (a sanity floor; the comparison above is the test)
    assert st["fills"] > 0.1 * n and st["gapped_fills"] > 0 and st["rounds"] >= 2
    if route == "throughput":
        assert st["dp_narrow_launches"] > 0, st


def test_sam_and_run_stats_on_unequal_mates():
    """SamLine's fields and the run statistics of the unequal-mates batch, on an index with a one-scaffold table, against their
    sequential restatements given every read's own length."""
    from bbmap_amd.mapper import SAM_MD
    from tests.test_runstats_gpu import _check_mapped
    from tests.test_sam_gpu import _counts, check_run
    b = PP.pair_batch()
    ref, reads, truth = b["ref"], b["reads"], b["truth"]
    packed = R.Packed([ref], [np.array([2000], np.int32)], [np.array([len(ref) - 4000], np.int32)], [["ref"]], 300)
    di = DeviceIndex.build([ref], k=PP.K_TEST)
    mp = None
    try:
        di.set_scaffolds(packed)
        mp = Mapper.from_records(di, *b["records"], paired=True, max_sites=32)
        mp.step()
        counts = _counts()
        got = check_run(mp, packed, reads, True, counts)
        recs, _, _ = got[SAM_MD]
        print(counts)
        flag = recs["flag"]
        assert (flag & 0x40).any() and (flag & 0x80).any() and ((flag & 0x40) != 0).sum() == ((flag & 0x80) != 0).sum() == len(reads) // 2
        assert counts["tlen_pos"] > 500 and counts["tlen_neg"] > 500
        assert counts["only_self"] >= 100 and counts["only_mate"] >= 100          # the (9,150) class: 110 unmappable mates
        mate_unmapped = [r for r in range(len(reads)) if flag[r] & 8 and not flag[r] & 4]
        assert {b["cls"][r // 2] for r in mate_unmapped} >= {(9, 150), (150, 11)}
        t = np.zeros(len(reads), RS.TRUTH_DTYPE)
        t["chrom"], t["strand"], t["start"], t["stop"] = 1, truth["strand"], truth["start"], truth["start"] + truth["len"] - 1
        stats, want = _check_mapped(mp, reads, True, t)
        assert int(stats["numMated"]) > 1000 and int(stats["numMatedBases"]) != int(stats["insertSizeSum"]) - int(stats["innerLengthSum"])
    finally:
        if mp is not None:
            mp.close()
        di.close()


def test_host_buffer_entry_with_unequal_mates():
    """bbmap_map_batch (host buffers in, packed lists out) on 300 of the pairs: the same lists as the device-resident call."""
    b = PP.pair_batch()
    reads = b["reads"][:600]
    recs, blob, bs, ki = PP.make_records(reads)
    n = len(reads)
    di = DeviceIndex.build([b["ref"]], k=PP.K_TEST)
    mp = Mapper.from_records(di, recs, blob, bs, ki, paired=True, max_sites=32)
    try:
        mp.step()
        out = mp.fetch(with_match=False)
        assert "overflow" not in out
        ns, po, sites, total = mp.map_batch_host(recs, blob, bs, ki, 64 * n)
    finally:
        mp.close()
        di.close()
    assert total == len(sites) == int(np.maximum(out["nsites"], 0).sum()) and np.array_equal(ns, out["nsites"])
    assert np.array_equal(po, np.concatenate([[0], np.cumsum(ns)]))
    for r in range(n):
        want, got = out["sites"][r][:ns[r]], sites[po[r]:po[r] + ns[r]]
        for f in want.dtype.names:
            if f not in ("match_job", "reserved"):
                assert (got[f] == want[f]).all(), (r, f)
    lens = b["truth"]["len"][:n]
    short_rescued = [r for r in range(n) if lens[r] < PP.K_TEST and ns[r] > 0]
    assert short_rescued and all(sites[po[r]]["rescued"] for r in short_rescued)      # the host entry's minus strands are written too
