"""tests/runstats_check.py (the sequential restatement the device counters are compared with) against answers derived by hand from the
Java text; each docstring carries its derivation.  Also bbmap_amd.runstats: the record layout against the header, summary()."""
import os
import re

import numpy as np

from bbmap_amd import runstats as RS
from tests import runstats_check as RC

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbmap_amd.h")


def F(mapped=1, chrom=1, strand=0, start=0, stop=0, paired=0, ambiguous=0, perfect=0, rescued=0):
    return dict(mapped=mapped, chrom=chrom, strand=strand, start=start, stop=stop, paired=paired, ambiguous=ambiguous, perfect=perfect,
                rescued=rescued)


def S(score, chrom=1, strand=0, start=0, stop=0, slowScore=0, perfect=0, semiperfect=0):
    return dict(score=score, chrom=chrom, strand=strand, start=start, stop=stop, slowScore=slowScore, perfect=perfect, semiperfect=semiperfect)


UNMAPPED = dict(mapped=0, chrom=-1, strand=0, start=-1, stop=-1, paired=0, ambiguous=0, perfect=0, rescued=0)


def nonzero(stats):
    return {k: v for k, v in stats.items() if v}


def test_unequal_mates_pin_line_1481():
    """Mate 1 has 100 bases at [1000, 1099] plus, mate 2 has 150 at [1300, 1449] minus, paired.  :1481 gives len2 = r.length() = 100, so
    numMatedBases = 100 + 100 = 200 (not 250).  r.start <= r2.start: inner = 1300 - 1099 = 201, outer = 1449 - 1000 = 449;
    insertSizeSum uses the real lengths (:1559): 201 + 100 + 150 = 451.  Histogram: strands differ -> PlusLeft, r1 = plus mate,
    mid = 1300 - 1099 - 1 = 200, insert = 200 + 100 + 150 = 450."""
    f = [F(start=1000, stop=1099, paired=1), F(strand=1, start=1300, stop=1449, paired=1)]
    sites = [[S(9000, start=1000, stop=1099)], [S(12000, strand=1, start=1300, stop=1449)]]
    st, h = RC.run_stats(f, [b"m" * 100, b"m" * 150], sites, [100, 150], True)
    assert (st["numMated"], st["numMatedBases"], st["innerLengthSum"], st["outerLengthSum"], st["insertSizeSum"]) == (1, 200, 201, 449, 451)
    assert st["mappedRetainedBases1"] == 100 and st["mappedRetainedBases2"] == 150 and st["matchCountM2"] == 150
    assert h[450] == 1 and h.sum() == 1
    assert st["firstSiteCorrectPaired1"] == 1 and st["firstSiteCorrectP1"] == 1 and st["firstSiteCorrectM2"] == 1       # no truth: site 0 is its own original
    assert st["correctUniqueHit1"] == 1 and st["uniqueHit2"] == 1 and st["readsUsed2"] == 1 and st["basesUsed2"] == 150


def test_bad_pair_counts_mate_one_twice():
    """Both mapped, not paired: `else if(r2!=null && r2.mapped())` -> badPairs 1, badPairBases = len1 + len2 = 2 * 80 (:1481 again)."""
    f = [F(start=10, stop=89), F(chrom=2, start=500, stop=619)]
    st, h = RC.run_stats(f, [b"m" * 80, b"m" * 120], [[S(1, start=10, stop=89)], [S(1, chrom=2, start=500, stop=619)]], [80, 120], True)
    assert (st["badPairs"], st["badPairBases"], st["numMated"]) == (1, 160, 0) and h.sum() == 0
    assert st["firstSiteCorrectSolo1"] == 1


def test_inner_distance_clamp_both_ends():
    """inner = r2.start - r.stop.  Mates 40,000 apart: min(32000, 39901) = 32000.  Mate 2 far inside mate 1's span on the left
    (r.start <= r2.start, r2.start - r.stop = 1000 - 1400 = -400): max(-160, -400) = -160.  outer is not clamped."""
    f = [F(start=1000, stop=1099, paired=1), F(strand=1, start=41000, stop=41099, paired=1)]
    one = [[S(1)], [S(1)]]
    st, _ = RC.run_stats(f, [None, None], one, [100, 100], True)
    assert (st["innerLengthSum"], st["outerLengthSum"], st["insertSizeSum"]) == (32000, 40099, 32200)
    f = [F(start=1000, stop=1400, paired=1), F(strand=1, start=1000, stop=1099, paired=1)]
    st, _ = RC.run_stats(f, [None, None], one, [100, 100], True)
    assert (st["innerLengthSum"], st["outerLengthSum"], st["insertSizeSum"]) == (-160, 99, 40)


def test_mate_one_right_of_mate_two():
    """r.start > r2.start: inner = r.start - r2.stop = 700 - 599 = 101, outer = r.stop - r2.start = 799 - 500 = 299 (:1550-1553).
    Histogram: r1 minus, r2 plus -> PlusLeft swaps so that the plus read is r1: mid = 700 - 599 - 1 = 100, insert 300."""
    f = [F(strand=1, start=700, stop=799, paired=1), F(strand=0, start=500, stop=599, paired=1)]
    st, h = RC.run_stats(f, [None, None], [[S(1)], [S(1)]], [100, 100], True)
    assert (st["innerLengthSum"], st["outerLengthSum"]) == (101, 299) and h[300] == 1


def test_x_y_c_symbols():
    """countErrors: X, Y and I are insertions, C counts with N.  "CCmmXYmISDDNm": m 4, s 1, d 2, i 3 (X, Y, I), n 3 (C, C, N)."""
    assert RC.count_errors(b"CCmmXYmISDDNm") == (4, 1, 2, 3, 3)
    st, _ = RC.run_stats([F(stop=9)], [b"CCmmXYmISDDNm"], [[S(5, stop=9)]], [11], False)
    assert [st["matchCount%s1" % c] for c in "MSDIN"] == [4, 1, 2, 3, 3]
    assert [st["readCount%s1" % c] for c in "SDINE"] == [1, 1, 1, 1, 1]
    st, _ = RC.run_stats([F(stop=9)], [b"mmNmm"], [[S(5, stop=9)]], [5], False)
    assert st["readCountN1"] == 1 and st["readCountE1"] == 0            # N alone is no error read (:1529)


def test_three_groups_correct_in_group_two_is_low_hit():
    """Scores 900, 800, 800, 700: groups begin at sites 0, 1, 3.  Truth matches site 2 only -> correct found with group == 2:
    correctGroup 2 > 1 -> correctLowHit; firstElementCorrect 0 -> firstSiteIncorrect; truePositive by the READ's strand (:1613)."""
    sites = [S(900, start=5000, stop=5099), S(800, start=7000, stop=7099), S(800, start=100, stop=199), S(700, start=9000, stop=9099)]
    truth = [dict(chrom=1, strand=0, start=100, stop=199)]
    c = RC.calc_correctness(sites, truth[0], 0)
    assert c[0] == 2 and c[1] == 2 and c[2] == 3 and c[3] == 4 and c[6] == 1 and c[7] == 1 and c[8] == 0
    st, _ = RC.run_stats([F(strand=1, start=5000, stop=5099)], [None], [sites], [100], False, truth=truth)
    want = dict(readsUsed1=1, basesUsed1=100, mappedRetained1=1, mappedRetainedBases1=100, firstSiteIncorrect1=1, firstSiteIncorrectLoose1=1,
                siteSum1=4, topSiteSum1=1, uniqueHit1=1, truePositiveM1=1, totalCorrectSites1=1, correctLowHit1=1)
    assert nonzero(st) == want


def test_top_group_of_two_is_multi_hit():
    """Scores 900, 900, 500; truth = site 1.  sizeOfTopGroup 2, correct group 1 -> correctMultiHit; site 0 is not it -> firstSiteIncorrect."""
    sites = [S(900, start=5000, stop=5099), S(900, start=100, stop=199), S(500, start=100, stop=199, chrom=2)]
    st, _ = RC.run_stats([F(start=5000, stop=5099)], [None], [sites], [100], False, truth=[dict(chrom=1, strand=0, start=100, stop=199)])
    assert st["correctMultiHit1"] == 1 and st["topSiteSum1"] == 2 and st["uniqueHit1"] == 0 and st["firstSiteIncorrect1"] == 1
    assert st["truePositiveP1"] == 1 and st["correctUniqueHit1"] == 0


def test_loose_only():
    """Site 0 starts 15 off and stops 30 off the truth, thresh 0: strict needs both within 0 -> incorrect; loose needs either within
    0 + 20 -> |start| 15 <= 20 -> firstSiteCorrectLoose, and falsePositive (no strictly correct site anywhere).  With thresh 5 nothing
    changes; with thresh 30 strict holds too."""
    sites = [S(900, start=115, stop=229)]
    truth = [dict(chrom=1, strand=0, start=100, stop=199)]
    for thresh, strict in ((0, 0), (5, 0), (30, 1)):
        st, _ = RC.run_stats([F(start=115, stop=229)], [None], [sites], [100], False, truth=truth, thresh=thresh)
        assert st["firstSiteCorrectLoose1"] == 1 and st["firstSiteIncorrectLoose1"] == 0
        assert st["firstSiteIncorrect1"] == 1 - strict and st["falsePositive1"] == 1 - strict and st["firstSiteCorrectP1"] == strict
    st, _ = RC.run_stats([F(start=115, stop=229)], [None], [[S(900, strand=1, start=100, stop=199)]], [100], False, truth=truth)
    assert st["firstSiteIncorrectLoose1"] == 1                           # the strand differs: not even loose


def test_no_truth_site_zero_is_its_own_original():
    """original == ssl.get(0): site 0 is correct by construction; a second site at the same place and score is a second correct site."""
    sites = [S(900, start=100, stop=199, perfect=1, semiperfect=1, slowScore=9970), S(900, start=100, stop=199, semiperfect=1)]
    st, _ = RC.run_stats([F(start=100, stop=199, rescued=1)], [b"m" * 100], [sites], [100], False, truth=[dict(chrom=-1, strand=0, start=0, stop=0)])
    assert st["firstSiteCorrectP1"] == 1 and st["firstSiteCorrectRescued1"] == 1 and st["rescuedP1"] == 1
    assert st["totalCorrectSites1"] == 2 and st["correctMultiHit1"] == 1
    assert st["perfectHitCount1"] == 1 and st["semiPerfectHitCount1"] == 2 and st["semiperfectMatch1"] == 1 and st["semiperfectMatchBases1"] == 100
    # perfectMatch through the score: maxQuality(100) = 70 + 99 * 100 = 9970 (11ts); 90 + 9900 = 9990 (9PacBio) does not match
    assert st["perfectMatch1"] == 1 and st["perfectMatchBases1"] == 100
    st, _ = RC.run_stats([F(start=100, stop=199)], [None], [sites], [100], False, scheme=1)
    assert st["perfectMatch1"] == 0


def test_unmapped_reads():
    """Single-ended unmapped: bothUnmapped 1, noHit 1.  Pair, both unmapped: bothUnmapped 2 with both real lengths; only mate 1
    unmapped: no bothUnmapped, no badPair (badPairs sits in the elements > 0 branch of mate 1)."""
    st, _ = RC.run_stats([UNMAPPED], [None], [[]], [77], False)
    assert nonzero(st) == dict(readsUsed1=1, basesUsed1=77, bothUnmapped=1, bothUnmappedBases=77, noHit1=1)
    st, _ = RC.run_stats([UNMAPPED, UNMAPPED], [None, None], [[], []], [70, 90], True)
    assert (st["bothUnmapped"], st["bothUnmappedBases"], st["noHit1"], st["noHit2"]) == (2, 160, 1, 1)
    st, _ = RC.run_stats([UNMAPPED, F(stop=89, ambiguous=1)], [None, None], [[], [S(3)]], [70, 90], True)
    assert (st["bothUnmapped"], st["badPairs"], st["noHit1"], st["mappedRetained2"]) == (0, 0, 1, 1)
    assert st["ambiguousBestAlignment2"] == 1 and st["ambiguousBestAlignmentBases2"] == 90


def test_insert_of_zero_and_above_the_histogram():
    """A mate with start == stop gives insert 0 (:2634), which is not counted (x > 0).  Mates 50,000 apart: mid + a + b = 50,100 ->
    min(40000, .) = 40000, the last bin.  Same strand, same start: min(a, b)."""
    f = [F(start=1000, stop=1000, paired=1), F(strand=1, start=1200, stop=1299, paired=1)]
    _, h = RC.run_stats(f, [None, None], [[S(1)], [S(1)]], [100, 100], True)
    assert h.sum() == 0
    f = [F(start=1000, stop=1099, paired=1), F(strand=1, start=51000, stop=51099, paired=1)]
    _, h = RC.run_stats(f, [None, None], [[S(1)], [S(1)]], [100, 100], True)
    assert h[40000] == 1 and h.sum() == 1 and len(h) == 40001
    f = [F(start=1000, stop=1099, paired=1), F(start=1000, stop=1079, paired=1)]
    _, h = RC.run_stats(f, [None, None], [[S(1)], [S(1)]], [100, 80], True)
    assert h[80] == 1
    # plus read to the right of the minus read, disjoint: r1.start > r2.stop -> Unstranded(r2, r1) -> 500 - 199 - 1 + 200 = 500
    f = [F(strand=0, start=500, stop=599, paired=1), F(strand=1, start=100, stop=199, paired=1)]
    _, h = RC.run_stats(f, [None, None], [[S(1)], [S(1)]], [100, 100], True)
    assert h[500] == 1


def test_average_pair_dist_is_float_arithmetic():
    """innerLengthSum = 50,331,651 = 3 * 2^24 + 3 is not a float: between 2^25 and 2^26 floats lie 4 apart, and it is 3 above
    50,331,648 and 1 below 50,331,652, so it rounds to the nearer, 50,331,652 (no tie).  / 2 (numMated, exact) = 25,165,826 in float, while the integer quotient is 25,165,825."""
    s, n = 50331651, 2
    assert s > 2 ** 24 and float(np.float32(s)) == 50331652.0
    assert RC.java_average_pair_dist(s, n) == 25165826 and s // n == 25165825
    assert RC.java_average_pair_dist(300 * 1001 + 7, 1001) == 300
    st = dict(numMated=1001, innerLengthSum=300 * 1001 + 7, mappedRetained2=1001)
    assert RC.insert_length_rule(st, True, 100) == 300
    assert RC.insert_length_rule(st, False, 100) == 100                  # no paired read in the batch
    assert RC.insert_length_rule(dict(st, numMated=1000), True, 100) == 100          # `numMated>1000`


def test_rescue_skip_rule():
    """mappedRetained2 > 1000 && numMated * 20 < mappedRetained2: 1001 / 50 -> 1000 < 1001 skip; 1001 / 51 -> 1020 no; 1000 / 0 no."""
    assert RC.rescue_skip_rule(dict(mappedRetained2=1001, numMated=50))
    assert not RC.rescue_skip_rule(dict(mappedRetained2=1001, numMated=51))
    assert not RC.rescue_skip_rule(dict(mappedRetained2=1000, numMated=0))


def test_summary_on_hand_made_counters():
    """1,000 reads of 100 bases per mate; 600 mated, 50 bad pairs; match columns 90,000 m, 4,000 S, 2,000 D, 3,000 I, 1,000 N."""
    st = {n: 0 for n in RS.RUNSTATS_DTYPE.names}
    st.update(readsUsed1=1000, readsUsed2=1000, basesUsed1=100000, basesUsed2=100000, numMated=600, numMatedBases=120000, badPairs=50,
              badPairBases=10000, innerLengthSum=180000, outerLengthSum=300000, insertSizeSum=240000, mappedRetained1=900,
              mappedRetainedBases1=90000, matchCountM1=90000, matchCountS1=4000, matchCountD1=2000, matchCountI1=3000, matchCountN1=1000,
              firstSiteCorrectP1=400, firstSiteCorrectM1=410, firstSiteCorrectLoose1=850, firstSiteIncorrect1=90, noHit1=100)
    s = RS.summary(st)
    assert s["matedPercent"] == 60.0 and s["badPairsPercent"] == 5.0 and s["matedPercentBases"] == 60.0
    assert s["insertSizeAvg"] == 400.0 and s["innerLengthAvg"] == 300.0 and s["outerLengthAvg"] == 500.0
    assert s["mappedPercent"] == 90.0 and s["mappedPercentBases"] == 90.0 and s["noHitPercent"] == 10.0
    assert s["matchLen"] == 100000 and s["matchRate"] == 90.0 and s["errorRate"] == 9.0
    assert (s["subRate"], s["delRate"], s["insRate"], s["nRate"]) == (4.0, 2.0, 3.0, 1.0)
    assert s["truePositiveStrict"] == 81.0 and s["truePositiveLoose"] == 85.0 and s["falsePositive"] == 9.0
    assert np.isnan(RS.summary({n: 0 for n in RS.RUNSTATS_DTYPE.names})["insertSizeAvg"])
    assert RS.summary(RC.as_record(st))["matedPercent"] == 60.0         # a record works as well as a dict


def test_record_layout_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct bbmap_runstats \{(.*?)\} bbmap_runstats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"int64_t\s+(\w+);", body)
    assert names == list(RS.RUNSTATS_DTYPE.names)
    assert RS.RUNSTATS_DTYPE.itemsize == 8 * len(names) == 768
    assert re.search(r"BBMAP_INSERT_HIST_BINS = (\d+)", text).group(1) == str(RS.INSERT_HIST_BINS)
    assert re.search(r"BBMAP_RUNSTATS_MAX_WAVES = (\d+)", text).group(1) == str(RS.RUNSTATS_MAX_WAVES)
    assert re.search(r"BBMAP_ADAPT_INSERT_LENGTH = 1, BBMAP_ADAPT_RESCUE_SKIP = 2", text)
    assert "typedef struct bbmap_truth { int32_t chrom, strand, start, stop; } bbmap_truth;" in text and RS.TRUTH_DTYPE.itemsize == 16
