"""Coverage (bbmap_cov_* / bbpipe_coverage_* in include/bbmap_amd.h): the record layouts, the flag and tile constants, the raw device
calls, and the text of covstats= / covhist= / basecov= / bincov= with the summary block, character for character what
jgi.CoveragePileup's format strings give at the class's defaults (header with `#`, COUNT_GC on, KEEP_SHORT_BINS on).

The device returns integers only.  The float columns are derived here, each replacing one Java loop:
  Avg_fold          basehits / (double) length                                     writeStats :1071
  Ref_GC            gc / (float) max(at + gc, 1), float32 arithmetic               ChromosomeArray.calcGC :204-209
  Covered_percent   covered * 100d / length                                        the loop at writeStats :1023-1028
  Read_GC           (C + G) * 1d / max(1, A + C + G + T)                           writeStats :1064-1065
  Std_Dev           over the scaffold's length + 1 elements, from sum and sum of squares (exact integers, one division and one
                    square root in float64)                                        Tools.standardDeviation(char[] / int[]) :2050-2074
  the summary's standard deviation, over `length` elements of every scaffold     standardDeviation :1405-1438
  bincov's Cov      binsum / (float) binlength                                     writeCoveragePerBaseBinned2 :1298-1311
  bincov's Mean / STDev over the bins' depths                                      standardDeviationBinned :1349-1402
Java's %.4f rounds the exact decimal value of the double HALF_UP where Python's % rounds half-even (1/32 -> 0.0313 in Java), so every
float goes through decimal with ROUND_HALF_UP."""
import ctypes as C
import math
from decimal import ROUND_HALF_UP, Decimal
from fractions import Fraction

import numpy as np

from . import _lib as LL
from .index import READ_DTYPE

COV_START_ONLY, COV_EXCLUDE_DELETIONS, COV_STRANDED, COV_32BIT = 1, 2, 4, 8
COV_MAX_WAVES = 8192            # wavefronts of the accumulate kernel's persistent grid
COV_SCAN_TILE = 2048            # slots per workgroup of the prefix sum
COV_STATS_CHUNK = 65536         # slots per workgroup of the statistics pass and of the long median's counting pass
COV_MEDIAN_SHORT = 65536        # scaffolds up to this length: one-workgroup median; longer: many workgroups
COV_HIST_LDS_BINS = 1024        # depths below this go through a workgroup's LDS sub-histogram
COV_LDS_SCAFFOLDS = 512         # tables of up to this many scaffolds: per-scaffold counters are summed in LDS first

COVSTRAND_DTYPE = np.dtype([("covered", "<i8"), ("median", "<i8"), ("max", "<i8"), ("sumDepth", "<i8"), ("sumSqLo", "<u8"), ("sumSqHi", "<u8")])
COVREC_DTYPE = np.dtype([("length", "<i8"), ("basehits", "<i8"), ("readhits", "<i8"), ("readhitsMinus", "<i8"), ("fraghits", "<i8"),
                         ("readBases", "<i8", (4,)), ("refBases", "<i8", (4,)), ("strand", COVSTRAND_DTYPE, (2,))])
COVTOTALS_DTYPE = np.dtype([("readsProcessed", "<i8"), ("mappedReads", "<i8"), ("mappedBases", "<i8"), ("refBases", "<i8")])


class bbmap_cov_view(C.Structure):
    _fields_ = [("flags", C.c_int32), ("nscaf", C.c_int32), ("binsize", C.c_int32), ("depth_bytes", C.c_int32), ("slots", C.c_int64),
                ("hist_bins", C.c_int64), ("nbins", C.c_int64), ("covoff", C.c_void_p), ("depth", C.c_void_p * 2), ("recs", C.c_void_p),
                ("hist", C.c_void_p * 2), ("binoff", C.c_void_p), ("bins", C.c_void_p * 2), ("totals", C.c_void_p)]


def hist_bins(flags):
    """writeStats' histmax + 1 (:1009)"""
    return 1000001 if flags & COV_32BIT else 65536


def layout(lengths, binsize=0):
    """bbpipe_coverage_layout: (covoff int64[n + 1], binoff int64[n + 1] or None)."""
    L = LL.load()
    lengths = np.ascontiguousarray(lengths, np.int32)
    n = len(lengths)
    covoff = np.zeros(n + 1, np.int64)
    binoff = np.zeros(n + 1, np.int64) if binsize > 0 else None
    LL.check(L.bbpipe_coverage_layout(n, lengths.ctypes.data, int(binsize), covoff.ctypes.data, None if binoff is None else binoff.ctypes.data),
             "bbpipe_coverage_layout")
    return covoff, binoff


class Coverage:
    """What a finalize returns, as numpy arrays: recs (COVREC_DTYPE[nscaf]), totals (COVTOTALS_DTYPE scalar), covoff, depth (one array
    of `slots` entries per strand; scaffold s is depth[t][covoff[s] : covoff[s] + length]), hist (int64[hist_bins] per strand), binoff
    and bins (int64[nbins] per strand, None without a binsize), names (by global scaffold number, or None)."""

    def __init__(self, flags, recs, totals, covoff, depth, hist, binsize, binoff, bins, names=None):
        self.flags, self.recs, self.totals, self.covoff, self.depth, self.hist = flags, recs, totals, covoff, depth, hist
        self.binsize, self.binoff, self.bins, self.names = binsize, binoff, bins, names
        self.strands = 2 if flags & COV_STRANDED else 1

    def name(self, s):
        n = self.names[s] if self.names is not None else "scaffold_%d" % s
        return n.decode() if isinstance(n, bytes) else str(n)

    def scaffold_depth(self, s, strand=0):
        a = int(self.covoff[s])
        return self.depth[strand][a:a + int(self.recs[s]["length"])]


class DeviceState:
    """Device arrays of the raw calls for one scaffold table, owned by the caller (torch tensors): tests plant records and accumulate
    into it without mapping anything.  table = (locs, lengths, pad, base) as tests' table_of gives it, indexed by chromosome number."""

    def __init__(self, table, flags, device=0):
        import torch
        locs, lengths, pad, _ = table
        self.flags, self.pad, self.nchroms = flags, int(pad), len(locs) - 1
        off, loc, ln = [0, 0], [], []
        for c in range(1, self.nchroms + 1):
            loc += list(locs[c]); ln += list(lengths[c]); off.append(len(loc))
        self.lengths = np.asarray(ln, np.int32)
        self.nscaf = len(ln)
        self.covoff, _ = layout(self.lengths)
        self.slots = int(self.covoff[-1])
        dev = torch.device("cuda", device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        self.dev = dev
        self.d_off, self.d_loc, self.d_len, self.d_covoff = up(off, np.int32), up(loc, np.int32), up(ln, np.int32), up(self.covoff, np.int64)
        self.strands = 2 if flags & COV_STRANDED else 1
        self.diff = [torch.zeros(self.slots, dtype=torch.int32, device=dev) for _ in range(self.strands)]
        self.recs = torch.zeros(self.nscaf * COVREC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.totals = torch.zeros(4, dtype=torch.int64, device=dev)

    def add(self, reads, bases, finals, pool, paired=False):
        """bbpipe_coverage_add_device: reads / finals uint8 views of READ_DTYPE / FINAL_DTYPE records, bases and pool uint8 (device tensors)."""
        import torch
        L = LL.load()
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream().cuda_stream
        LL.check(L.bbpipe_coverage_add_device(C.c_void_p(stream), reads.numel() // READ_DTYPE.itemsize, int(paired), self.flags, ptr(reads), ptr(bases), ptr(finals),
                                              ptr(pool), self.nchroms, self.nscaf, ptr(self.d_off), ptr(self.d_loc), ptr(self.d_len), self.pad,
                                              ptr(self.d_covoff), ptr(self.diff[0]), ptr(self.diff[1]) if self.strands == 2 else None,
                                              ptr(self.recs), ptr(self.totals)), "bbpipe_coverage_add_device")
        torch.cuda.current_stream().synchronize()

    def finalize(self, binsize=0, names=None):
        """bbpipe_coverage_finalize_device -> Coverage."""
        import torch
        L = LL.load()
        dev, f32 = self.dev, bool(self.flags & COV_32BIT)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        depth = [torch.zeros(self.slots, dtype=torch.int32 if f32 else torch.int16, device=dev) for _ in range(self.strands)]
        hb = hist_bins(self.flags)
        hist = [torch.zeros(hb, dtype=torch.int64, device=dev) for _ in range(self.strands)]
        binoff = bins = d_binoff = None
        nbins = 0
        if binsize > 0:
            _, binoff = layout(self.lengths, binsize)
            nbins = int(binoff[-1])
            d_binoff = torch.from_numpy(binoff).to(dev)
            bins = [torch.zeros(max(1, nbins), dtype=torch.int64, device=dev) for _ in range(self.strands)]
        wb = L.bbpipe_coverage_workspace_bytes(self.nscaf, self.slots)
        ws = torch.zeros(max(8, wb), dtype=torch.uint8, device=dev)
        two = self.strands == 2
        stream = torch.cuda.current_stream().cuda_stream
        LL.check(L.bbpipe_coverage_finalize_device(C.c_void_p(stream), self.flags, self.nscaf, self.slots, ptr(self.d_len), ptr(self.d_covoff),
                                                   ptr(self.diff[0]), ptr(self.diff[1]) if two else None, ptr(depth[0]),
                                                   ptr(depth[1]) if two else None, ptr(self.recs), None, ptr(hist[0]), ptr(hist[1]) if two else None,
                                                   int(binsize), ptr(d_binoff), nbins, ptr(bins[0]) if bins else None,
                                                   ptr(bins[1]) if bins and two else None, ptr(self.totals), ptr(ws), wb),
                 "bbpipe_coverage_finalize_device")
        torch.cuda.current_stream().synchronize()
        host = lambda t: t.cpu().numpy()
        dd = [host(d).view(np.int32 if f32 else np.uint16) for d in depth]
        return Coverage(self.flags, host(self.recs).view(COVREC_DTYPE), host(self.totals).view(COVTOTALS_DTYPE)[0], self.covoff, dd,
                        [host(h) for h in hist], binsize, binoff, [host(b)[:nbins] for b in bins] if bins else None, names)


# ---------------------------------------------------------------------------------------------------------------------- text

def jfmt(x, places):
    """String.format("%.<places>f", x) for a finite double (or a float32 widened to one): the exact decimal value, HALF_UP."""
    return str(Decimal(float(x)).quantize(Decimal(1).scaleb(-places), rounding=ROUND_HALF_UP))


def _sumsq(st):
    return (int(st["sumSqHi"]) << 64) | int(st["sumSqLo"])


def _sqrt_fraction(fr):
    return math.sqrt(fr) if fr > 0 else 0.0


def scaffold_stdev(rec, strand=0):
    """Tools.standardDeviation over the scaffold's length + 1 elements (the extra slot is 0); 0 for a scaffold no read touched (its
    array was never made, writeStats :1044-1046)."""
    if int(rec["readhits"]) == 0:
        return 0.0
    st = rec["strand"][strand]
    n, s, q = int(rec["length"]) + 1, int(st["sumDepth"]), _sumsq(st)
    return _sqrt_fraction(Fraction(n * q - s * s, n * n))


def global_stdev(cov, strand=0, minscaf=0):
    """standardDeviation (:1405-1438): (mean, stdev) over the `length` elements of every scaffold of at least minscaf bases."""
    n = s = q = 0
    for rec in cov.recs:
        if int(rec["length"]) >= minscaf:
            st = rec["strand"][strand]
            n += int(rec["length"]); s += int(st["sumDepth"]); q += _sumsq(st)
    if n < 1:
        return 0.0, 0.0
    return s / n, _sqrt_fraction(Fraction(n * q - s * s, n * n))


def _touched(rec):
    return int(rec["readhits"]) > 0


COVSTATS_HEADER = "#ID\tAvg_fold\tLength\tRef_GC\tCovered_percent\tCovered_bases\tPlus_reads\tMinus_reads\tMedian_fold\tRead_GC\tStd_Dev"


def covstats_lines(cov, strand=0, minscaf=0, nzo=False):
    """writeStats (:991-1106) for one strand; nzo = NONZERO_ONLY."""
    out = [COVSTATS_HEADER]
    for s, rec in enumerate(cov.recs):
        length, total = int(rec["length"]), int(rec["basehits"])
        if not ((total > 0 or not nzo) and length >= minscaf):
            continue
        st = rec["strand"][strand]
        rb, fb = [int(x) for x in rec["readBases"]], [int(x) for x in rec["refBases"]]
        ref_gc = np.float32(fb[1] + fb[2]) / np.float32(max(fb[0] + fb[3] + fb[1] + fb[2], 1))
        read_gc = (rb[1] + rb[2]) * 1.0 / max(1, rb[0] + rb[1] + rb[2] + rb[3])
        covered = int(st["covered"]) if _touched(rec) else 0
        median = int(st["median"]) if _touched(rec) else -1
        out.append("%s\t%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%s" % (
            cov.name(s), jfmt(total / length, 4), length, jfmt(ref_gc, 4), jfmt(covered * 100.0 / length, 4), covered,
            int(rec["readhits"]) - int(rec["readhitsMinus"]), int(rec["readhitsMinus"]), median, jfmt(read_gc, 4),
            jfmt(scaffold_stdev(rec, strand), 2)))
    return out


def java_hist(cov, strand=0):
    """The histogram writeStats returns: the device counts every scaffold's bases, writeStats only those of the scaffolds a read
    touched (the others have no array, :1022), whose bases are all at depth 0."""
    h = np.array(cov.hist[strand], np.int64)
    h[0] -= sum(int(r["length"]) for r in cov.recs if not _touched(r))
    return h


def covhist_lines(cov, strand=0):
    """writeHist (:1113-1132)"""
    h = java_hist(cov, strand)
    nz = np.flatnonzero(h)
    top = int(nz[-1]) if len(nz) else 0
    return ["#Coverage\tnumBases"] + ["%d\t%d" % (i, int(h[i])) for i in range(top + 1)]


def basecov_lines(cov, strand=0, minscaf=0):
    """writeCoveragePerBase (:1143-1177), the plain form"""
    out = ["#RefName\tPos\tCoverage"]
    for s, rec in enumerate(cov.recs):
        if int(rec["length"]) >= minscaf:
            name = cov.name(s)
            out += ["%s\t%d\t%d" % (name, i, int(x)) for i, x in enumerate(cov.scaffold_depth(s, strand))]
    return out


def binned_mean_stdev(cov, strand=0, minscaf=0):
    """standardDeviationBinned (:1349-1402): (mean, stdev) of the bins' depths, each bin's own length as its divisor"""
    depths = []
    for s, rec in enumerate(cov.recs):
        length = int(rec["length"])
        if length >= minscaf:
            a, b = int(cov.binoff[s]), int(cov.binoff[s + 1])
            sizes = np.full(b - a, cov.binsize, np.int64)
            sizes[-1] = length - (b - a - 1) * cov.binsize
            depths.append(cov.bins[strand][a:b].astype(np.float64) / sizes)
    if not depths:
        return 0.0, 0.0
    d = np.concatenate(depths)
    mean = math.fsum(d) / len(d)
    return mean, math.sqrt(math.fsum((mean - d) ** 2) / len(d))


def bincov_lines(cov, strand=0, minscaf=0):
    """writeCoveragePerBaseBinned2 (:1276-1315): RunningPos counts the bases of every scaffold, printed or not"""
    mean, stdev = binned_mean_stdev(cov, strand, minscaf)
    out = ["#Mean\t" + jfmt(mean, 3), "#STDev\t" + jfmt(stdev, 3), "#RefName\tCov\tPos\tRunningPos"]
    running = 0
    for s, rec in enumerate(cov.recs):
        length, name = int(rec["length"]), cov.name(s)
        a, b = int(cov.binoff[s]), int(cov.binoff[s + 1])
        for k in range(b - a):
            last = min(length, (k + 1) * cov.binsize)
            size = last - k * cov.binsize
            if length >= minscaf:
                out.append("%s\t%s\t%d\t%d" % (name, jfmt(np.float32(int(cov.bins[strand][a + k])) / np.float32(size), 2), last, running))
            running += size
    return out


def summary_lines(cov, minscaf=0):
    """The block printOutput prints (:885-898), after writeStats' pass over strand 0."""
    ref = int(cov.totals["refBases"])
    mult = 1.0 / ref
    with_cov = sum(1 for r in cov.recs if int(r["basehits"]) > 0)
    covered = sum(int(r["strand"][0]["covered"]) for r in cov.recs if _touched(r))
    return ["", "Average coverage:                    \t" + jfmt(int(cov.totals["mappedBases"]) * mult, 2),
            "Standard deviation:                    \t" + jfmt(global_stdev(cov, 0, minscaf)[1], 2),
            "Percent scaffolds with any coverage: \t" + jfmt(with_cov * 100.0 / len(cov.recs), 2),
            "Percent of reference bases covered:  \t" + jfmt(covered * 100 * mult, 2)]
