"""GPU tests of the BBMap-profile mapper under non-default settings, against the CPU restatement run with THE SAME settings dict
(tests/config_problems.py: the workloads, the case table and the strict hand-over to bbmap_config and MapParams): site lists field by
field, every fill's window / minScore / score vector / iterations / traceback string, final records and match strings
(tests/mapper_check.py: compare).  tests/test_oracle_config.py shows on the oracle alone that every case's setting is live on its
workload, and holds the measured counts.

Beyond the comparison: stats()["refills"] equals the oracle's number of kind-1 fills in every case (scoreSlow's wider refill,
mapper.hip's phases 1 -> 2, BBMapThread.java:312-335: until these tests no mapper test ran it and nothing read the counter), the
refill cases run it at least ten times, single-ended and paired, also with logs that start at 64 entries (NO_ROOM in phase 0; the
first growth leaves room for the rest of these batches, so no phase-1 refill waits for room -- see tests/config_problems.py);
the minRatio cases run under both DP routes; the maxPairDist cases also pin the run statistics, which take the configured value (one
on the only input found where that value changes a counter, one where it provably cannot).

Every case prints its fills / refills / rescue fills / narrow launches."""
import numpy as np
import pytest

from bbmap_amd.index import DeviceIndex
from bbmap_amd.mapper import Mapper
from tests import config_problems as CP
from tests.mapper_check import compare, set_route

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def indexes():
    """name -> (DeviceIndex, OracleIndex) of a workload, built when first asked for and shared by every case on that workload"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (DeviceIndex.build([CP.workload(name)["ref"]], k=CP.K), CP.oracle_index(name))
        return made[name]
    yield get
    for di, _ in made.values():
        di.close()


def _map(case, indexes):
    """The case on the device and on the oracle, both from ONE dict: (Mapper -- the caller closes it --, out, stats, oracle result)"""
    w = CP.workload(case.workload)
    di, oi = indexes(case.workload)
    settings = dict(case.settings, **case.mapper)
    orc = CP.oracle_run(case.workload, settings, oi)                  # (refuses a key MapParams lacks, unless it is device-only)
    kw = CP.device_settings({k_: v for k_, v in settings.items() if k_ != "max_sites"})
    offs, ks = CP.keys()
    mp = Mapper(di, w["n"], CP.L, offs, ks, paired=w["paired"], max_sites=settings.get("max_sites", 32), **kw)
    mp.load_reads(w["reads"])
    mp.step()
    return mp, mp.fetch(), mp.stats(), orc


def _check(case, out, st, orc, route="latency"):
    w = CP.workload(case.workload)
    kinds = CP.kind_counts(orc)
    print("%s [%s] %r: fills %d + %d, refills %d, rescue fills %d, narrow launches %d, reads in the tier %d; oracle fills by kind %s"
          % (case.name, route, dict(case.settings, **case.mapper), st["fills"], st["gapped_fills"], st["refills"], st["rescue_fills"],
             st["dp_narrow_launches"], st["reads_reprobed"], kinds))
    assert st["reads_overflowed"] == 0
    if case.mapper.get("max_sites", 32) < 32:
        assert st["reads_reprobed"] > 0 and "overflow" in out
    bad = compare(out, orc, w["n"], paired=w["paired"])
    assert not bad, "%d differences\n" % len(bad) + "\n".join(bad[:20])
    assert st["refills"] == kinds[1], (st["refills"], kinds)
    if st["reads_reprobed"] == 0:                                      # (a pair the tier maps again may have been rescued twice)
        assert st["rescue_fills"] == kinds[2], (st["rescue_fills"], kinds)
    if "refills>=10" in case.effects:
        assert st["refills"] >= 10
    if case.mapper.get("jobsPerRead", 0) < 0:
        assert st["log_growths"] >= 1                                  # the logs ran full (in the first round: phase 0)


@pytest.mark.parametrize("case", CP.CASES, ids=lambda c: c.name)
def test_settings_match_oracle(monkeypatch, indexes, case):
    set_route(monkeypatch, "latency")
    mp, out, st, orc = _map(case, indexes)
    mp.close()
    _check(case, out, st, orc)


DEFAULTS = CP.Case("defaults", "pairs", {}, (), {}, {})


@pytest.mark.parametrize("case", [CP.BY_NAME["minRatio_0.30_pairs"], DEFAULTS, CP.BY_NAME["minRatio_0.90"], CP.BY_NAME["minRatio_0.30_diverged"]],
                         ids=lambda c: c.name)
def test_min_ratio_on_the_throughput_route(monkeypatch, indexes, case):
    """minRatio sets every fill's minScore and with it which fills the band kernel in front of the first pass takes; the narrow
    launches per ratio are printed (0.30, the default 0.56 and 0.90 on one workload), no order among them is asserted (measured: 4
    narrow launches at each of the three, 2 on the diverged reads)."""
    set_route(monkeypatch, "throughput")
    mp, out, st, orc = _map(case, indexes)
    mp.close()
    _check(case, out, st, orc, "throughput")
    assert st["dp_narrow_launches"] > 0, st                              # the route really ran


def _inner(a, b):
    """the inner distance of two mapped mates' final records, as calcStatistics1 takes it (AbstractMapThread.java:1542-1559)"""
    if a["start"] <= b["start"]:
        return int(b["start"]) - int(a["stop"])
    return int(a["start"]) - int(b["stop"])


@pytest.mark.parametrize("name, binds", [("maxPairDist_18_tip_indel", True), ("maxPairDist_500", False)])
def test_run_statistics_take_the_configured_max_pair_dist(monkeypatch, indexes, name, binds):
    """bbmap_add_run_stats forwards bbmap_config.maxPairDist to the clamp of the inner length (run_stats.hip; AbstractMapThread.java
    :1542-1559), which every other test leaves at 32000: every counter and the insert-size histogram against the sequential
    restatement given the configured value.

    The clamp only sees pairs with the `paired` flag, and pairing itself asks for an inner distance within maxPairDist, so on
    ordinary input it cannot bind: at maxPairDist = 500 on the wide-insert pairs 311 pairs are paired, the largest inner distance
    is 498, and the statistics equal those with the clamp at 32000 -- asserted, so that the statement is checked.  It binds where
    the final stage moves a paired mate after pairing: at maxPairDist = 18 on the tip-indel mates (tipSearchDist = 0) three of
    265 paired pairs end 19, 22 and 22 bases apart, and innerLengthSum is 9 less than with the clamp at 32000.  A library that
    forwards a constant, or ignores the field, fails that case."""
    from tests import runstats_check as RC
    set_route(monkeypatch, "latency")
    case = CP.BY_NAME[name]
    w = CP.workload(case.workload)
    mp, out, st, orc = _map(case, indexes)
    try:
        limit = case.settings["maxPairDist"]
        assert mp.cfg.maxPairDist == limit
        reads = w["reads"].reshape(-1, CP.L)
        got, want = RC.check_mapped(mp, reads, True, None)
        wide, _ = RC.run_stats(*RC.restate(mp, reads, True, None), True, None, 0, 0, 32000)
        fin = out["final"]
        over = [_inner(fin[r], fin[r + 1]) - limit for r in range(0, w["n"], 2)
                if fin[r]["paired"] and fin[r]["mapped"] and fin[r + 1]["mapped"] and _inner(fin[r], fin[r + 1]) > limit]
        print("%s: numMated %d, badPairs %d, innerLengthSum %d (%d with the clamp at 32000), paired pairs beyond the limit by %s"
              % (name, int(got["numMated"]), int(got["badPairs"]), int(got["innerLengthSum"]), int(wide["innerLengthSum"]), over))
        assert int(got["numMated"]) > 100 and int(got["badPairs"]) > 100          # pairs on both sides of the limit
        assert int(wide["innerLengthSum"]) - int(got["innerLengthSum"]) == sum(over)
        if binds:
            assert len(over) >= 3 and RC.differences(got, wide) != []
        else:
            assert over == [] and RC.differences(got, wide) == []
    finally:
        mp.close()
