"""Pins the coverage restatement (tests/coverage_check.py) and the formatters of bbmap_amd/coverage.py by one worked example, derived
by hand below, plus Java's HALF_UP rounding and the minscaf / nzo filters.  No GPU.

The table: chromosome 1 holds scaffold chrA (10 bases at 1000) and chrB (8 bases at 1310, 300 N behind chrA); chromosome 2 holds
chrC (6 bases at 500).  pad = 300.  Single-ended reads (fraghits moves by 2):

  r0  chr 1  1002..1005  +  ACGT     isSingleScaffold: 1002+300 lies in chrA's range, 1005 < 1310.  mid 1003 -> chrA.  relative 2..5
  r1  chr 1  1004..1007  -  GGCC     relative 4..7, minus strand
  r2  chr 1   998..1001  +  AANN     mid (998+1001)/2 = 999 -> chrA.  relative -2..1, clamped to 0..1 (basehits 2)
  r3  chr 1  1008..1011  +  TTTT     relative 8..11, clamped to 8..9 (basehits 2)
  r4  chr 1  1005..1312  +  ACGT     spans chrA and chrB (1312 >= 1310): not counted, readsProcessed moves
  r5  chr 1  1311..1314  +  ACAC     1311+300 is past the last start: single.  mid 1312 -> chrB.  relative 1..4
  r6  chr 2   500..505   +  ACGTACG  match CmmDmImm.  relative 0..5 (default mode: the string is not looked at)
  r7  unmapped

  chrA  depth 1 1 1 1 2 2 1 1 1 1 (+ the extra slot 0)   basehits 12  readhits 4 (1 minus)  fraghits 8   reads' bases A3 C3 G3 T5
        median: 11 elements descending 2 2 1 1 1 1 1 1 1 1 0, element 10/2 = 5 -> 1
        Std_Dev over 11 elements: sum 12, sum of squares 16, variance 16/11 - (12/11)^2 = 32/121, sqrt = 0.5143 -> 0.51
        Read_GC 6/14 = 0.4286
  chrB  depth 0 1 1 1 1 0 0 0   basehits 4   median: 1 1 1 1 0 0 0 0 0, element 4 -> 0   variance 4/9 - 16/81 = 20/81 -> 0.4969 -> 0.50
  chrC  depth 1 1 1 1 1 1       basehits 6   median: element 3 of 1 1 1 1 1 1 0 -> 1    variance 6/7 - 36/49 = 6/49 -> 0.3499 -> 0.35
        Read_GC 4/7 = 0.5714
  histogram: depth 0: 4 (chrB), depth 1: 8 + 4 + 6 = 18, depth 2: 2
  totals: readsProcessed 8, mappedReads 6, mappedBases 4+4+4+4+4+7 = 27, refBases 24
  bins of 4: chrA 4/4, 6/4, 2/2 (short)   chrB 3/4, 1/4   chrC 4/4, 2/2 (short); RunningPos 0 4 8 | 10 14 | 18 22
        mean (1 + 1.5 + 1 + .75 + .25 + 1 + 1)/7 = 0.9286 -> 0.929; deviations^2 sum 0.839286, /7, sqrt = 0.3463 -> 0.346
  summary: 27 * (1.0/24) = 1.125 (the product is exact in binary here) -> 1.13 HALF_UP; global deviation over 24 elements: sum 22,
        squares 26, variance 26/24 - (22/24)^2 = 140/576 -> 0.4930 -> 0.49; 3 of 3 scaffolds; 20 of 24 bases = 83.33
  exclude-deletions mode, r6: C nothing, m 0, m 1, D skips 2, m 3, I nothing, m 4, m 5 -> depth 1 1 0 1 1 1, basehits 5"""
import numpy as np

from bbmap_amd import coverage as V
from tests import coverage_check as K

LOCS = [None, [1000, 1310], [500]]
LENGTHS = [None, [10, 8], [6]]
TABLE = (LOCS, LENGTHS, 300, [0, 0, 2])
NAMES = ["chrA", "chrB", "chrC"]
REFCOUNTS = [(3, 2, 3, 2), (1, 0, 0, 7), (1, 1, 1, 3)]
#            mapped chrom start stop strand bases        match
RECORDS = [(1, 1, 1002, 1005, 0, b"ACGT", None),
           (1, 1, 1004, 1007, 1, b"GGCC", None),
           (1, 1, 998, 1001, 0, b"AANN", None),
           (1, 1, 1008, 1011, 0, b"TTTT", None),
           (1, 1, 1005, 1312, 0, b"ACGT", None),
           (1, 1, 1311, 1314, 0, b"ACAC", None),
           (1, 2, 500, 505, 0, b"ACGTACG", b"CmmDmImm"),
           (0, -1, -1, -1, 0, b"ACGT", None)]


def pileup(flags=0, records=RECORDS):
    p = K.Pileup(TABLE, flags, NAMES, REFCOUNTS)
    for mapped, chrom, start, stop, strand, bases, match in records:
        p.process_read(bool(mapped), chrom, start, stop, strand, bases, match, 0)
    return p


def as_coverage(p, binsize=4):
    """The restatement's integers in the layout the device returns, for the formatters of bbmap_amd.coverage"""
    n = len(p.list)
    recs = np.zeros(n, V.COVREC_DTYPE)
    lengths = np.array([s.length for s in p.list], np.int64)
    covoff = np.concatenate([[0], np.cumsum(lengths + 1)])
    strands = 2 if p.flags & K.STRANDED else 1
    depth = [np.concatenate([p.depth(s, t) for s in p.list]) for t in range(strands)]
    for g, s in enumerate(p.list):
        r = recs[g]
        r["length"], r["basehits"], r["readhits"], r["readhitsMinus"], r["fraghits"] = s.length, s.basehits, s.readhits, s.readhitsMinus, s.fraghits
        r["readBases"], r["refBases"] = s.basecount[:4], s.refcount
        for t in range(strands):
            d = [int(x) for x in p.depth(s, t)[:s.length]]
            st = r["strand"][t]
            st["covered"], st["median"], st["max"], st["sumDepth"] = sum(x > 0 for x in d), p.median(s, t), max(d), sum(d)
            q = sum(x * x for x in d)
            st["sumSqLo"], st["sumSqHi"] = q & (2 ** 64 - 1), q >> 64
    totals = np.zeros(1, V.COVTOTALS_DTYPE)[0]
    totals["readsProcessed"], totals["mappedReads"], totals["mappedBases"], totals["refBases"] = p.readsProcessed, p.mappedReads, p.mappedBases, p.refBases
    nb = (lengths + binsize - 1) // binsize
    binoff = np.concatenate([[0], np.cumsum(nb)])
    return V.Coverage(p.flags, recs, totals, covoff, depth, [p.device_hist(t) for t in range(strands)], binsize, binoff,
                      [p.bin_sums(binsize, t) for t in range(strands)], NAMES)


HEADER = "#ID\tAvg_fold\tLength\tRef_GC\tCovered_percent\tCovered_bases\tPlus_reads\tMinus_reads\tMedian_fold\tRead_GC\tStd_Dev"
COVSTATS = [HEADER,
            "chrA\t1.2000\t10\t0.5000\t100.0000\t10\t3\t1\t1\t0.4286\t0.51",
            "chrB\t0.5000\t8\t0.0000\t50.0000\t4\t1\t0\t0\t0.5000\t0.50",
            "chrC\t1.0000\t6\t0.3333\t100.0000\t6\t1\t0\t1\t0.5714\t0.35"]
COVHIST = ["#Coverage\tnumBases", "0\t4", "1\t18", "2\t2"]
BINCOV = ["#Mean\t0.929", "#STDev\t0.346", "#RefName\tCov\tPos\tRunningPos",
          "chrA\t1.00\t4\t0", "chrA\t1.50\t8\t4", "chrA\t1.00\t10\t8",
          "chrB\t0.75\t4\t10", "chrB\t0.25\t8\t14",
          "chrC\t1.00\t4\t18", "chrC\t1.00\t6\t22"]
SUMMARY = ["", "Average coverage:                    \t1.13", "Standard deviation:                    \t0.49",
           "Percent scaffolds with any coverage: \t100.00", "Percent of reference bases covered:  \t83.33"]
DEPTH_A, DEPTH_B, DEPTH_C = [1, 1, 1, 1, 2, 2, 1, 1, 1, 1], [0, 1, 1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1]


def test_worked_example_counters_and_depths():
    p = pileup()
    a, b, c = p.list
    assert (p.readsProcessed, p.mappedReads, p.mappedBases, p.refBases) == (8, 6, 27, 24)
    assert [int(x) for x in p.depth(a)] == DEPTH_A + [0]
    assert [int(x) for x in p.depth(b)] == DEPTH_B + [0]
    assert [int(x) for x in p.depth(c)] == DEPTH_C + [0]
    assert (a.basehits, a.readhits, a.readhitsMinus, a.fraghits, a.basecount[:4]) == (12, 4, 1, 8, [3, 3, 3, 5])
    assert a.basecount[5] == 2                              # the two N of r2 go to slot 5, which is not reported
    assert (b.basehits, b.readhits, b.readhitsMinus, b.fraghits, b.basecount[:4]) == (4, 1, 0, 2, [2, 2, 0, 0])
    assert (c.basehits, c.readhits, c.readhitsMinus, c.fraghits, c.basecount[:4]) == (6, 1, 0, 2, [2, 2, 2, 1])
    assert [p.median(s) for s in p.list] == [1, 0, 1]
    assert [int(x) for x in p.bin_sums(4)] == [4, 6, 2, 3, 1, 4, 2]


def test_worked_example_text_of_the_restatement():
    p = pileup()
    lines, hist = p.write_stats()
    assert lines == COVSTATS
    assert p.write_hist(hist) == COVHIST
    assert p.write_binned(4) == BINCOV
    assert p.summary() == SUMMARY
    base = p.write_coverage_per_base()
    assert base[0] == "#RefName\tPos\tCoverage" and len(base) == 1 + 24
    assert base[1:11] == ["chrA\t%d\t%d" % (i, d) for i, d in enumerate(DEPTH_A)]
    assert base[11:19] == ["chrB\t%d\t%d" % (i, d) for i, d in enumerate(DEPTH_B)]
    assert base[19:] == ["chrC\t%d\t%d" % (i, d) for i, d in enumerate(DEPTH_C)]


def test_worked_example_text_of_the_formatters():
    """bbmap_amd.coverage derives the same text from the integers the device returns"""
    p = pileup()
    cov = as_coverage(p)
    assert V.covstats_lines(cov) == COVSTATS
    assert V.covhist_lines(cov) == COVHIST
    assert V.bincov_lines(cov) == BINCOV
    assert V.summary_lines(cov) == SUMMARY
    assert V.basecov_lines(cov) == p.write_coverage_per_base()


def test_paired_reads_move_fraghits_by_one():
    p = K.Pileup(TABLE, 0, NAMES, REFCOUNTS)
    p.process_read(True, 1, 1002, 1005, 0, b"ACGT", None, 1)
    assert p.list[0].fraghits == 1 and p.list[0].readhits == 1


def test_exclude_deletions_walks_the_string():
    p = pileup(K.EXCLUDE_DELETIONS, [RECORDS[6]])
    c = p.list[2]
    assert [int(x) for x in p.depth(c)] == [1, 1, 0, 1, 1, 1, 0] and c.basehits == 5
    # the clamped-start quirk: a record that begins 2 left of chrA walks its string from the scaffold's first base
    p = pileup(K.EXCLUDE_DELETIONS, [(1, 1, 998, 1001, 0, b"AAAA", b"mmmm")])
    assert [int(x) for x in p.depth(p.list[0])][:5] == [1, 1, 0, 0, 0] and p.list[0].basehits == 2
    # no string: the read counters move, no depth does
    p = pileup(K.EXCLUDE_DELETIONS, [(1, 1, 1002, 1005, 0, b"ACGT", None)])
    assert p.list[0].readhits == 1 and p.list[0].basehits == 0 and int(p.depth(p.list[0]).sum()) == 0


def test_start_only_and_stranded():
    p = pileup(K.START_ONLY | K.EXCLUDE_DELETIONS)          # START_ONLY wins (:626)
    assert [int(x) for x in p.depth(p.list[0])] == [1, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0]
    assert p.list[0].basehits == 12
    p = pileup(K.STRANDED)
    assert [int(x) for x in p.depth(p.list[0], 0)] == [1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 0]
    assert [int(x) for x in p.depth(p.list[0], 1)] == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    lines, _ = p.write_stats(1)
    assert lines[1] == "chrA\t1.2000\t10\t0.5000\t40.0000\t4\t3\t1\t0\t0.4286\t0.48"      # 4/11 - 16/121 = 28/121 -> 0.4810
    assert V.covstats_lines(as_coverage(p), 1) == lines


def test_a_record_left_of_its_scaffold_moves_basehits_down():
    """wholly inside the pad: relative -8..-5 -> start 0, stop -5: basehits -4, no depth (the assert at :608 is off)"""
    p = pileup(0, [(1, 1, 992, 995, 0, b"ACGT", None)])
    a = p.list[0]
    assert a.basehits == -4 and a.readhits == 1 and int(p.depth(a).sum()) == 0
    assert K.jdiv(-7, 2) == -3 and K.jdiv(7, 2) == 3        # the midpoint rule truncates toward zero


def test_java_rounds_half_up():
    assert "%.4f" % (1 / 32) == "0.0312"                    # Python: half-even on the exact tie
    assert V.jfmt(1 / 32, 4) == "0.0313" and K.jfmt(1 / 32, 4) == "0.0313"         # Java
    assert V.jfmt(1.125, 2) == "1.13" and V.jfmt(0.125, 2) == "0.13" and V.jfmt(2.5, 0) == "3"
    assert V.jfmt(0.1 + 0.2, 4) == "0.3000" and V.jfmt(1.005, 2) == "1.00"        # 1.005 is below the tie in binary
    assert V.jfmt(np.float32(1) / np.float32(3), 4) == "0.3333"


def test_minscaf_and_nzo_filters():
    p = pileup(0, [RECORDS[5]])                             # only chrB is touched
    cov = as_coverage(p)
    lines, hist = p.write_stats()
    assert lines == [HEADER,
                     "chrA\t0.0000\t10\t0.5000\t0.0000\t0\t0\t0\t-1\t0.0000\t0.00",     # no array: median -1, deviation 0
                     "chrB\t0.5000\t8\t0.0000\t50.0000\t4\t1\t0\t0\t0.5000\t0.50",
                     "chrC\t0.0000\t6\t0.3333\t0.0000\t0\t0\t0\t-1\t0.0000\t0.00"]
    assert V.covstats_lines(cov) == lines
    assert p.write_hist(hist) == ["#Coverage\tnumBases", "0\t4", "1\t4"]            # untouched scaffolds are not in the histogram
    assert V.covhist_lines(cov) == p.write_hist(hist)
    assert int(cov.hist[0][0]) == 4 + 10 + 6                                        # the device counts them; the formatter takes them out
    nz, _ = p.write_stats(nzo=True)
    assert nz == [HEADER, lines[2]] and V.covstats_lines(cov, nzo=True) == nz
    big, _ = p.write_stats(minscaf=8)
    assert big == lines[:3] and V.covstats_lines(cov, minscaf=8) == big
    binned = p.write_binned(4, minscaf=8)
    assert binned[3:] == ["chrA\t0.00\t4\t0", "chrA\t0.00\t8\t4", "chrA\t0.00\t10\t8", "chrB\t0.75\t4\t10", "chrB\t0.25\t8\t14"]
    assert V.bincov_lines(cov, minscaf=8) == binned
    assert len(V.basecov_lines(cov, minscaf=8)) == 1 + 18 and V.basecov_lines(cov, minscaf=8) == p.write_coverage_per_base(minscaf=8)
    assert V.summary_lines(cov) == p.summary()


def test_saturation_at_the_cap():
    t = ([None, [0]], [None, [3]], 300, [0, 0])
    p = K.Pileup(t, 0)
    p.cap = 2
    for _ in range(3):
        p.process_read(True, 1, 0, 2, 0, b"A", None, 0)
    assert [int(x) for x in p.depth(p.list[0])] == [2, 2, 2, 0] and p.list[0].basehits == 9
