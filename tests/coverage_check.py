"""Test-local restatement of jgi.CoveragePileup as BBMap feeds it, the yardstick of the coverage tests, sequential and loop for loop:
processRead (current/jgi/CoveragePileup.java:784-813), ScaffoldCoordinates.setFromIndex (current/stream/ScaffoldCoordinates.java:37-56),
addCoverage (:600-663), addCoverageIgnoringDeletions (:665-722), CoverageArray2/3.increment / incrementRange
(current/dna/CoverageArray2.java:145-164, CoverageArray3.java:155-174), and the output side: writeStats (:991-1106), writeHist
(:1113-1132), writeCoveragePerBase (:1143-1177), writeCoveragePerBaseBinned2 (:1276-1315), standardDeviation (:1405-1438),
standardDeviationBinned (:1349-1402), Tools.standardDeviation (current/align2/Tools.java:2050-2074), the summary of printOutput
(:885-898).  Assertions are off, as in a BBMap run.  Two stated deviations, the library's own (include/bbmap_amd.h): a start-only
record whose clamped start is at or past its scaffold's end adds no depth, and a record without a match string in exclude-deletions
mode adds the read counters and no depth."""
import math
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

try:
    from tests.scaffold_check import is_single_scaffold, scaffold_index
except ImportError:                         # (run from inside tests/)
    from scaffold_check import is_single_scaffold, scaffold_index

START_ONLY, EXCLUDE_DELETIONS, STRANDED, BITS32 = 1, 2, 4, 8

CHAR_TO_NUM = [6] * 256                     # AssemblyStats2.makeCharToNum (jgi/AssemblyStats2.java:1667-1683); only slots 0-3 are reported
for _c, _v in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3), ("Nn", 5), ("Xx", 4)):
    for _ch in _c:
        CHAR_TO_NUM[ord(_ch)] = _v


def jdiv(a, b):
    """Java's int division: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def jfmt(x, places):
    """String.format("%.<places>f", x): the double's exact decimal value rounded HALF_UP"""
    return str(Decimal(float(x)).quantize(Decimal(1).scaleb(-places), rounding=ROUND_HALF_UP))


class Scaffold:
    def __init__(self, name, length, refcount=(0, 0, 0, 0)):
        self.name, self.length = name, length
        self.basehits = self.readhits = self.readhitsMinus = self.fraghits = 0
        self.basecount = [0] * 8
        self.obj = [None, None]
        self.refcount = list(refcount)
        at, gc = refcount[0] + refcount[3], refcount[1] + refcount[2]
        self.gc = np.float32(gc) / np.float32(max(at + gc, 1))                  # ChromosomeArray.calcGC :204-209


class Pileup:
    """table = (locs, lengths, pad, base) as scaffold_check.table_of gives it; refcounts: A C G T per global scaffold or None."""

    def __init__(self, table, flags=0, names=None, refcounts=None):
        self.locs, self.lengths, self.pad, self.base = table
        self.flags = flags
        self.cap = 2 ** 31 - 1 if flags & BITS32 else 65535
        self.list = []
        for c in range(1, len(self.locs)):
            for i, length in enumerate(self.lengths[c]):
                g = len(self.list)
                self.list.append(Scaffold(names[g] if names else "scaffold_%d" % g, int(length), refcounts[g] if refcounts is not None else (0, 0, 0, 0)))
        self.refBases = sum(s.length for s in self.list)                        # loadScaffoldsFromIndex :445
        self.readsProcessed = self.mappedReads = self.mappedBases = 0

    # ---- accumulation
    def process_read(self, mapped, chrom, start, stop, strand, bases, match, mate_count):
        """processRead :784-813 with USE_SECONDARY and PHYSICAL_COVERAGE off"""
        self.readsProcessed += 1
        if not mapped:
            return False
        if not is_single_scaffold(self.locs, self.pad, chrom, start, stop):     # setFromIndex :43
            return False
        idx = scaffold_index(self.locs, self.pad, chrom, jdiv(start + stop, 2))
        scaf = self.list[self.base[chrom] + idx]
        rstart = start - int(self.locs[chrom][idx])                             # scaffoldRelativeLoc
        rstop = rstart - start + stop
        return self.add_coverage(scaf, bases, match, rstart, rstop, len(bases), strand, 2 - mate_count)

    def _array(self, scaf, strand):
        if scaf.obj[0] is None:                                                 # :635-640
            scaf.obj[0] = np.zeros(scaf.length + 1, np.int64)
            if self.flags & STRANDED:
                scaf.obj[1] = np.zeros(scaf.length + 1, np.int64)
        return scaf.obj[1 if (self.flags & STRANDED) and strand == 1 else 0]

    def add_coverage(self, scaf, seq, match, start0, stop0, readlen, strand, increment_frags):
        start, stop = max(start0, 0), min(stop0, scaf.length - 1)               # :605-606
        self.mappedBases += readlen
        self.mappedReads += 1
        scaf.readhits += 1
        scaf.fraghits += increment_frags
        if strand == 1:
            scaf.readhitsMinus += 1
        for b in seq:
            scaf.basecount[CHAR_TO_NUM[b]] += 1
        start_only = bool(self.flags & START_ONLY)
        if (self.flags & EXCLUDE_DELETIONS) and not start_only:                 # :626
            return self.add_coverage_ignoring_deletions(scaf, match, start, stop, strand)
        scaf.basehits += stop - start + 1                                       # :631-632, negative for a record left of its scaffold
        ca = self._array(scaf, strand)
        if start_only:
            if start < scaf.length:                                             # (stated deviation)
                ca[start] = min(ca[start] + 1, self.cap)                        # CoverageArray.increment
        else:
            lo, hi = max(start, 0), max(stop, -1)                                # incrementRange: `if(min<0){min=0;}`, `if(max<0){max=-1;}`
            if hi >= lo:                                                        # `for(i=min; i<=max; i++)`: each position +1, capped
                ca[lo:hi + 1] = np.minimum(ca[lo:hi + 1] + 1, self.cap)
        return True

    def add_coverage_ignoring_deletions(self, scaf, match, start, stop, strand):
        ca = self._array(scaf, strand)
        basehits = 0
        rpos, mpos = start, 0
        match = match or b""                                                    # (stated deviation: no string, no depth)
        while mpos < len(match) and rpos <= stop:                               # :682-695
            m = match[mpos]
            if m in b"mSN":
                ca[rpos] = min(ca[rpos] + 1, self.cap)
                basehits += 1
                rpos += 1
            elif m == ord("D"):
                rpos += 1
            mpos += 1
        scaf.basehits += basehits
        return True

    def add_batch(self, finals, matches, reads, paired):
        """finals: FINAL_DTYPE records; matches[r]: bytes or None; reads[r]: the read's bases (bytes)"""
        for r in range(len(finals)):
            f = finals[r]
            self.process_read(bool(int(f["mapped"])), int(f["chrom"]), int(f["start"]), int(f["stop"]), int(f["strand"]), reads[r], matches[r],
                              1 if paired else 0)

    # ---- what the device returns
    def depth(self, scaf, strand=0):
        """the scaffold's length + 1 elements (zeros when no read touched it)"""
        ca = scaf.obj[strand]
        return ca if ca is not None else np.zeros(scaf.length + 1, np.int64)

    def median(self, scaf, strand=0):
        """Arrays.sort, reverseInPlace, ca.get(length / 2) (:1033-1042)"""
        return int(np.sort(self.depth(scaf, strand))[::-1][scaf.length // 2])

    def device_hist(self, strand=0):
        """min(depth, histmax) over the positions < length of EVERY scaffold, as the library counts it"""
        histmax = 1000000 if self.flags & BITS32 else 65535
        h = np.zeros(histmax + 1, np.int64)
        for scaf in self.list:
            np.add.at(h, np.minimum(self.depth(scaf, strand)[:scaf.length], histmax), 1)
        return h

    def bin_sums(self, binsize, strand=0):
        """the sums writeCoveragePerBaseBinned2 divides (:1298-1311), every scaffold, in order"""
        out = []
        for scaf in self.list:
            ca = self.depth(scaf, strand)
            last, nxt, total = -1, binsize - 1, 0
            for i in range(scaf.length):
                total += int(ca[i])
                if i >= nxt or i == scaf.length - 1:
                    out.append(total)
                    nxt += binsize
                    last, total = i, 0
        return np.asarray(out, np.int64)

    # ---- the output side
    def write_stats(self, strand=0, minscaf=0, nzo=False):
        """writeStats :991-1106 -> (lines, hist)"""
        lines = ["#ID\tAvg_fold\tLength\tRef_GC\tCovered_percent\tCovered_bases\tPlus_reads\tMinus_reads\tMedian_fold\tRead_GC\tStd_Dev"]
        histmax = 1000000 if self.flags & BITS32 else 65535
        hist = np.zeros(histmax + 1, np.int64)
        self.scaffoldsWithCoverage = self.totalCoveredBases = 0
        for scaf in self.list:
            total, covered, median, stdev = scaf.basehits, 0, -1, 0.0
            ca = scaf.obj[strand]
            if ca is not None:
                for i in range(scaf.length):
                    x = int(ca[i])
                    hist[min(x, histmax)] += 1
                    if x > 0:
                        covered += 1
                stdev = standard_deviation(ca)
                median = self.median(scaf, strand)
            if total > 0:
                self.scaffoldsWithCoverage += 1
            if (total > 0 or not nzo) and scaf.length >= minscaf:
                bc = scaf.basecount
                gc = (bc[1] + bc[2]) * 1.0 / max(1, bc[0] + bc[1] + bc[2] + bc[3])
                lines.append("%s\t%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s" % (
                    scaf.name, jfmt(total / float(scaf.length), 4), scaf.length, jfmt(scaf.gc, 4), jfmt(covered * 100.0 / scaf.length, 4), covered,
                    scaf.readhits - scaf.readhitsMinus, scaf.readhitsMinus, median, jfmt(gc, 4), jfmt(stdev, 2)))
            self.totalCoveredBases += covered
        return lines, hist

    def write_hist(self, counts):
        """writeHist :1113-1132"""
        top = len(counts) - 1
        while top > 0 and counts[top] == 0:
            top -= 1
        return ["#Coverage\tnumBases"] + ["%d\t%d" % (i, int(counts[i])) for i in range(top + 1)]

    def write_coverage_per_base(self, strand=0, minscaf=0):
        """writeCoveragePerBase :1143-1177, deltaOnly false"""
        lines = ["#RefName\tPos\tCoverage"]
        for scaf in self.list:
            if scaf.length >= minscaf:
                ca = scaf.obj[strand]
                for i in range(scaf.length):
                    lines.append("%s\t%d\t%d" % (scaf.name, i, 0 if ca is None else int(ca[i])))
        return lines

    def standard_deviation_binned(self, binsize, strand=0, minscaf=0):
        """standardDeviationBinned :1349-1402"""
        depths = []
        for scaf in self.list:
            if scaf.length >= minscaf:
                ca = self.depth(scaf, strand)
                last, nxt, temp = -1, binsize - 1, 0
                for i in range(scaf.length):
                    temp += int(ca[i])
                    if i >= nxt or i == scaf.length - 1:
                        depths.append(temp / float(i - last))
                        nxt += binsize
                        last, temp = i, 0
        if not depths:
            return 0.0, 0.0
        total = 0.0
        for d in depths:
            total += d
        mean = total / len(depths)
        sumdev2 = 0.0
        for d in depths:
            dev = mean - d
            sumdev2 += dev * dev
        return mean, math.sqrt(sumdev2 / len(depths))

    def write_binned(self, binsize, strand=0, minscaf=0):
        """writeCoveragePerBaseBinned2 :1276-1315"""
        mean, stdev = self.standard_deviation_binned(binsize, strand, minscaf)
        lines = ["#Mean\t" + jfmt(mean, 3), "#STDev\t" + jfmt(stdev, 3), "#RefName\tCov\tPos\tRunningPos"]
        running = 0
        for scaf in self.list:
            ca = self.depth(scaf, strand)
            last, nxt, total = -1, binsize - 1, 0
            for i in range(scaf.length):
                total += int(ca[i])
                if i >= nxt or i == scaf.length - 1:
                    size = i - last
                    if scaf.length >= minscaf:
                        lines.append("%s\t%s\t%d\t%d" % (scaf.name, jfmt(np.float32(total) / np.float32(size), 2), i + 1, running))
                    running += size
                    nxt += binsize
                    last, total = i, 0
        return lines

    def standard_deviation(self, strand=0, minscaf=0):
        """standardDeviation :1405-1438 -> (mean, stdev) over `length` elements per scaffold"""
        total = bins = 0
        for scaf in self.list:
            if scaf.length >= minscaf:
                bins += scaf.length
                total += int(self.depth(scaf, strand)[:scaf.length].sum())
        if bins < 1:
            return 0.0, 0.0
        mean = total / float(bins)
        sumdev2 = 0.0
        for scaf in self.list:
            if scaf.length >= minscaf:
                temp = 0.0
                for x in self.depth(scaf, strand)[:scaf.length]:
                    dev = mean - int(x)
                    temp += dev * dev
                sumdev2 += temp
        return mean, math.sqrt(sumdev2 / bins)

    def summary(self, minscaf=0):
        """printOutput :885-898, after write_stats(0)"""
        mult = 1.0 / self.refBases
        return ["", "Average coverage:                    \t" + jfmt(self.mappedBases * mult, 2),
                "Standard deviation:                    \t" + jfmt(self.standard_deviation(0, minscaf)[1], 2),
                "Percent scaffolds with any coverage: \t" + jfmt(self.scaffoldsWithCoverage * 100.0 / len(self.list), 2),
                "Percent of reference bases covered:  \t" + jfmt(self.totalCoveredBases * 100 * mult, 2)]


def standard_deviation(numbers):
    """Tools.standardDeviation(char[] / int[]) :2050-2074"""
    if len(numbers) < 1:
        return 0.0
    total = 0
    for x in numbers:
        total += int(x)
    avg = total / float(len(numbers))
    sumdev2 = 0.0
    for x in numbers:
        dev = avg - int(x)
        sumdev2 += dev * dev
    return math.sqrt(sumdev2 / len(numbers))
