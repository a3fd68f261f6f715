"""CPU tests of the cases the mapper's settings are tested with (tests/config_problems.py): for every case the oracle alone must show
that the setting is live on the case's workload -- the run under the case's settings differs from the run it is compared with (the
profile's defaults, or the case's `base`) in the named way, on at least 5 reads or fills (two exceptions, both stated in the table
of cases: an effect asked for on one record or more beside others that hold the floor, and the case made to equal its base).
tests/test_mapper_config_gpu.py compares
the device with the oracle under the same settings; without this module a case could pass there with a setting that moves nothing.

What the oracle measures (reads whose final record / site list / rescued sites / `paired` flag differ; fills at the same (read, seq)
whose window / minScore differ; kind-1 windows that differ; the run's fills by kind 0 first fill, 1 scoreSlow's wider refill,
2 rescue, 3 final stage, 4 the final stage's padded refill; the base run's fills / kind-1 fills):

    case                         workload         final sites  resc. paired windows  minSc. k1 win.  fills by kind 0,1,2,3,4 (base: all / kind 1)
    minRatio_0.30_pairs          pairs                0     0      0      0      0     363       0  428,0,34,375,0 (837 / 0)
    minRatio_0.30_diverged       diverged            16    16      0      0      0      44       0  402,0,0,384,0 (770 / 0)
    minRatio_0.76                pairs               10    10      0     10      0     404       0  428,0,34,370,0 (837 / 0)
    minRatio_0.90                pairs              194   194     13    194      0     503       0  428,0,32,275,0 (837 / 0)
    padding_0_single             tip_indel            8     8      0      0    438       6       1  393,1,0,413,16 (837 / 22)
    padding_1_single             tip_indel            7     7      0      0    430       6       1  393,4,0,413,17 (837 / 22)
    padding_20_single            tip_indel          107   107      0      0    757      51       1  393,0,0,409,0 (837 / 22)
    padding_0_paired             wide_pairs           0     0      0      0    706       0       1  696,1,10,659,0 (1365 / 0)
    padding_1_paired             wide_pairs           0     0      0      0    706       0       0  696,0,10,659,0 (1365 / 0)
    padding_20_paired            wide_pairs           0     0      0      0   1365       0       0  696,0,10,659,0 (1365 / 0)
    padding_12_refills           tip_indel_pairs    220   405     14      0   1502      96       1  793,9,34,923,0 (1804 / 26)
    extraPadding_0               tip_indel            0     0      0      0     22       0      22  393,22,0,413,9 (837 / 22)
    extraPadding_30              tip_indel            0     0      0      0     22       0      22  393,22,0,413,9 (837 / 22)
    extraPadding_0_padding_2     tip_indel_pairs      2     2      1      0     11       0      11  793,11,45,930,19 (1798 / 11)
    extraPadding_30_padding_2    tip_indel_pairs      2     2      1      0     11       0      11  793,11,45,930,19 (1798 / 11)
    tipSearchDist_0              tip_indel           92    92      0      0    350     275       1  393,22,0,413,9 (801 / 1)
    tipSearchDist_15             tip_indel            5     5      0      0     71      59       0  393,1,0,410,0 (801 / 1)
    refill_paired                tip_indel_pairs    435   491    313      4    695     543       1  793,26,42,929,14 (2024 / 1)
    refill_small_logs            tip_indel           92    92      0      0    350     275       1  393,22,0,413,9 (801 / 1)
    refill_paired_small_logs     tip_indel_pairs    435   491    313      4    695     543       1  793,26,42,929,14 (2024 / 1)
    maxPairDist_500              wide_pairs         576   576      0    576      0       0       0  696,0,10,659,0 (1365 / 0)
    maxPairDist_18_tip_indel     tip_indel_pairs    289   293     35    270      6       1       0  793,26,12,929,14 (1804 / 26)
    doRescue_0                   pairs               39    39     39      0      0       0       0  428,0,0,375,0 (837 / 0)
    maxRescueDist_250            pairs               39    39     39      0      0       0       0  428,0,0,375,0 (837 / 0)
    averagePairDist_550          pairs               39    39     39      0      0       0       0  430,0,34,375,0 (805 / 0)
    averagePairDist_551          pairs                0     0      0      0      0       0       0  430,0,0,375,0 (805 / 0)
    averagePairDist_400_wide     wide_pairs          93  1198    103      0      0       0       0  695,0,102,659,0 (1365 / 0)
    maxRescueMismatches_3        pairs               13    13     13      0      0       0       0  428,0,12,375,0 (837 / 0)
    maxRescueMismatches_0        pairs               25    25     25      0      0       0       0  428,0,0,375,0 (837 / 0)
    maxTrimSitesToRetain_2       repeat_pairs       119   121     92     20    244     147       0  661,0,53,260,0 (1382 / 0)
    maxTrimSitesToRetain_8       repeat_pairs        11    11      4      6     55      30       0  1108,0,30,233,0 (1382 / 0)
    clearzone3_0_repeats         repeat_pairs         0     3      1      0      0     898       0  1127,0,26,229,0 (1382 / 0)
    clearzone3_0_near_copy       near_copy          125   125      0      0      0     129       0  293,0,0,164,0 (457 / 0)
    combined                     wide_pairs         968   968     10    968    865     756       0  696,0,5,182,0 (1365 / 0)
    overflow_tier                repeat_pairs        83    83     14     78   1299     362       0  1127,0,23,189,0 (1382 / 0)

Notes on single rows.
  * averagePairDist 550 / 551 are compared with the same value at doRescue = 0 (averagePairDist also enters the paired scores, so
    neither run equals the defaults' site lists): at 550 rescue still changes 39 reads, at 551 nothing at all differs from the run
    without rescue.  Their final records equal those of the defaults (550) and of doRescue = 0 (551).
  * minRatio = 0.30 moves no record of the ordinary pairs (363 logged minScores); on the diverged reads 384 instead of 368 of 400 map.
  * clearzone3 = 0 moves no final record on the repeat pairs (898 of 1382 logged minScores); on the near-copy reads 125 of 500
    change their mapScore or their `ambiguous` flag.
  * extraPadding: at the default slowAlignPadding the refill's width moves all 22 kind-1 windows of the tip-indel reads and no site.
    At slowAlignPadding = 2 on the tip-indel mates it does: between extraPadding 0 and 30, 11 kind-1 windows, the fill one site
    adopts, and 2 final records differ -- one site, so those two cases require `final >= 1` besides the windows.
  * maxPairDist = 18 on the tip-indel mates is the one input found on which a pair keeps its `paired` flag with a final inner
    distance beyond the limit (3 of 265 paired pairs, by 1, 4 and 4 bases: the final stage realigns a tip indel after pairing); the
    run-statistics test needs it.  padding 12 / 12 on the same mates keeps 9 refills (20 / 20 keeps none).
  * At the profile's defaults the tip-indel reads log ONE kind-1 fill, the ordinary workloads none: tipSearchDist = 100 finds the tip
    indels before scoreSlow would refill.  With tipSearchDist = 0 there are 22 (400 reads) and 26 (400 pairs)."""
import pytest

from tests import config_problems as CP


@pytest.mark.parametrize("case", CP.CASES, ids=lambda c: c.name)
def test_the_setting_is_live_on_its_workload(case):
    missed, m = CP.missed_effects(case)
    print(case.name, case.settings, "fills by kind", CP.kind_counts(CP.oracle_run(case.workload, case.settings)), m)
    assert not missed, (missed, m)


def test_every_flag_field_has_a_case():
    """every bbmap_config field that mirrors a BBMap flag and no other test moves is moved by some case, and both arms of both
    pairing-ratio max()es run (AbstractMapThread.java:106-107)"""
    moved = set().union(*(c.settings for c in CP.CASES))
    assert moved >= {"minRatio", "slowAlignPadding", "slowRescuePadding", "extraPadding", "tipSearchDist", "maxPairDist", "averagePairDist",
                     "maxRescueDist", "maxRescueMismatches", "maxTrimSitesToRetain", "doRescue", "clearzone3"}
    arms = set()
    for c in CP.CASES:
        r = c.settings.get("minRatio", 0.56)
        arms.add(("paired", r * .80 > 1.0 - (1.0 - r) * 1.4))
        arms.add(("preRescue", r * .60 > 1.0 - (1.0 - r) * 1.8))
    assert len(arms) == 4


def test_a_key_either_side_lacks_is_refused():
    """ctypes takes an unknown name as a new Python attribute; the hand-over must not"""
    with pytest.raises(KeyError):
        CP.oracle_params(dict(minratio=0.9))
    with pytest.raises(KeyError):
        CP.device_settings(dict(minratio=0.9))
    with pytest.raises(KeyError):
        CP.device_settings(dict(msaMaxRows=200))                    # the oracle's alone
    p = CP.oracle_params(dict(minRatio=0.9, jobsPerRead=-64, max_sites=4, fastCols=384))
    assert abs(p.minRatio - 0.9) < 1e-6 and p.slowAlignPadding == 4 and not hasattr(p, "jobsPerRead")
    assert CP.device_settings(dict(fastCols=384, clearzone3=0)) == dict(fastCols=384, clearzone3=0)
