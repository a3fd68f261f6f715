"""The mapper with its first DP context's launches width-sorted in front of the band kernel (BBMAP_SORT_PLAIN) and the 64-lane
launches' unlimited fills in the prune-free loop (BBMAP_WIDE_UNLIMITED), against the oracle's mapper and against itself with both
switched off: the "throughput" route settings of tests/mapper_check.py (band kernel and sort on every launch) on 2,000 pairs."""
import numpy as np
import pytest

from bbmap_amd import workload as W
from bbmap_amd.index import DeviceIndex
from bbmap_amd.mapper import Mapper
from oracle import oracle as O
from tests.mapper_check import FINAL_FIELDS, SITE_FIELDS, compare, set_route

pytestmark = pytest.mark.gpu


def test_sorted_plain_context_and_wide_unlimited_on_and_off(monkeypatch):
    set_route(monkeypatch, "throughput")
    L, k = 150, 12
    ref = W.make_reference(300000, seed=16, pad=2000, repeat_frac=0.15)
    reads, _ = W.make_pairs(ref, 2000, read_len=L, seed=14, pad=2000, hard_frac=0.08)
    offs = O.make_offsets(L, k, 1.9)
    ks = [100 * k] * len(offs)
    n = reads.size // L
    oi = O.OracleIndex([ref], k=k)
    oi.s.p.quitAfterTwoPerfects = 0
    r = reads.reshape(-1, L)
    orc = O.map_batch(oi, r[0::2].copy(), r[1::2].copy(), L, offs, ks, params=O.map_default_params(finalStage=1), cap=64, match_stride=4200)
    outs, stats = {}, {}
    for switch in ("1", "0"):
        monkeypatch.setenv("BBMAP_SORT_PLAIN", switch)
        monkeypatch.setenv("BBMAP_WIDE_UNLIMITED", switch)
        di = DeviceIndex.build([ref], k=k)
        mp = Mapper(di, n, L, offs, ks, paired=True, max_sites=32, finalStage=1)
        mp.load_reads(reads)
        mp.step()
        outs[switch], stats[switch] = mp.fetch(), mp.stats()
        mp.close()
        di.close()
        bad = compare(outs[switch], orc, n, paired=True)
        assert not bad, "switches %s:\n%s" % (switch, "\n".join(bad[:20]))
    monkeypatch.delenv("BBMAP_SORT_PLAIN")
    monkeypatch.delenv("BBMAP_WIDE_UNLIMITED")
    print("sorted launches: %d with the switches on, %d with them off; band kernel launches %d / %d"
          % (stats["1"]["dp_sorted_launches"], stats["0"]["dp_sorted_launches"], stats["1"]["dp_narrow_launches"], stats["0"]["dp_narrow_launches"]))
    assert stats["1"]["dp_sorted_launches"] > stats["0"]["dp_sorted_launches"], (stats["1"], stats["0"])
    assert stats["1"]["dp_narrow_launches"] == stats["0"]["dp_narrow_launches"] > 0
    a, b = outs["1"], outs["0"]
    assert (a["nsites"] == b["nsites"]).all()
    cap = a["sites"].shape[1]
    live = np.arange(cap)[None, :] < np.maximum(a["nsites"], 0)[:, None]
    for f in SITE_FIELDS:                                            # (match_job is a log position: it follows the order concurrent fills took)
        assert (a["sites"][f][live] == b["sites"][f][live]).all(), f
    for f in FINAL_FIELDS:
        assert (a["final"][f] == b["final"][f]).all(), f
    for q in range(n):
        ml = int(a["final"]["match_len"][q])
        if ml > 0:
            oa, ob = int(a["final"]["match_off"][q]), int(b["final"]["match_off"][q])
            assert a["final_match"][oa:oa + ml].tobytes() == b["final_match"][ob:ob + ml].tobytes(), q
