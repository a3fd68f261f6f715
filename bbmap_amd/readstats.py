"""Read histograms (bbmap_hist_* / bbpipe_read_hist_* in include/bbmap_amd.h): the flag and tile constants, the state's layout, the
raw device call, and the text of mhist= / qhist= / bqhist= / bqhist overall / qchist= / bhist= / qahist= / indelhist= / ehist= /
lhist= / gchist= / idhist=, character for character what align2.ReadStats' writers give (current/align2/ReadStats.java:728-1255) at
the class's defaults (skipZeroIndel on, ID_BINS_AUTO / GC_BINS_AUTO / GC_PLOT_X off, gchist and idhist with printZeros as writeAll
calls them).

The device returns integers only.  What the class keeps as running float sums is derived here from the position x quality table:
  qualSum[mate][i]        = sum over q of q * bqualHist[mate][i][q]                         addToQualityHistogram :305
  qualSumDouble[mate][i]  = sum over q of bqualHist[mate][i][q] * (double) PROB_ERROR[q]    :306 (Java adds them read by read: the
                            two sums can differ in the last bits, so qhist's log column can differ in its last printed digit at an
                            exact tie; every other column comes from integers)
  bqualHistOverall[q]     = qcountHist[0][q] + qcountHist[1][q]                             :308-310
Java's %.Nf rounds the exact decimal value of the double HALF_UP where Python's % rounds half-even, so every float goes through
decimal with ROUND_HALF_UP."""
import ctypes as C
import math
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

from . import _lib as LL
from .index import READ_DTYPE

RH_MATCH, RH_QUALITY, RH_BASE, RH_ACCURACY, RH_INDEL, RH_ERROR, RH_LENGTH, RH_GC, RH_IDENTITY = 1, 2, 4, 8, 16, 32, 64, 128, 256
RH_ALL = 511
RH_GROUPS = (RH_MATCH, RH_QUALITY, RH_BASE, RH_ACCURACY, RH_INDEL, RH_ERROR, RH_LENGTH, RH_GC, RH_IDENTITY)
RH_MAXLEN, RH_MAXINSLEN, RH_MAXDELLEN, RH_MAXDELLEN2, RH_GC_BINS, RH_ID_BINS = 6000, 1000, 1000, 1000000, 100, 100
RH_MAX_POS = 6016               # the library's longest read: positions of bhist, bins of lhist / ehist
RH_QUAL_BINS, RH_ACC_BINS, RH_DEL2_BINS = 127, 99, RH_MAXDELLEN2 // 100 + 1
RH_MAX_BLOCKS = 256             # workgroups of the accumulate kernel's persistent grid
RH_CHUNK_UNITS = 2048           # pairs (single reads) a workgroup counts between two flushes of its LDS counters
RH_POS_TILE = 256               # positions below this are counted in LDS
RH_QUAL_TILE = 44               # bqualHist's LDS sub-table: positions below the tile x qualities below this
RH_ERR_LDS_BINS, RH_LEN_LDS_BINS, RH_DEL2_LDS_BINS = 256, 512, 64
MIN_CALLED_QUALITY, MAX_CALLED_QUALITY = 2, 41          # current/stream/Read.java:3407-3408

# QualityTools.makeQualityToFloat(127) (current/align2/QualityTools.java:519-527): float32 of 10^(-q/10), slot 0 = 0.8f
PROB_ERROR = np.array([np.float32(math.pow(10, 0 - .1 * i)) for i in range(127)], np.float32)
PROB_ERROR[0] = np.float32(.8)

# name -> shape, in the order of bbmap_readhist_view's pointers
SHAPES = [("match", (7, 2, RH_MAXLEN)), ("qual_length", (2, RH_MAXLEN)), ("bqual", (2, RH_MAXLEN, RH_QUAL_BINS)), ("qcount", (2, RH_QUAL_BINS)),
          ("base", (2, 5, RH_MAX_POS)), ("accuracy", (4, RH_ACC_BINS)), ("ins", (RH_MAXINSLEN + 1,)), ("del", (RH_MAXDELLEN,)),
          ("del2", (RH_DEL2_BINS,)), ("error", (RH_MAX_POS + 1,)), ("length", (RH_MAX_POS + 1,)), ("gc", (RH_GC_BINS + 2,)),
          ("identity", (2 * (RH_ID_BINS + 1) + 1,))]


class bbmap_readhist_view(C.Structure):
    _fields_ = [("flags", C.c_int32), ("reserved", C.c_int32), ("words", C.c_int64), ("state", C.c_void_p)] + \
        [(name if name != "del" else "del_", C.c_void_p) for name, _ in SHAPES]


def state_words(flags):
    """bbpipe_read_hist_bytes / 8"""
    L = LL.load()
    b = L.bbpipe_read_hist_bytes(int(flags))
    if b < 0:
        LL.check(int(b), "bbpipe_read_hist_bytes")
    return b // 8


def jfmt(x, places):
    """String.format("%.<places>f", x) for a double: the exact decimal value, HALF_UP; NaN and the infinities as Java prints them."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    return str(Decimal(x).quantize(Decimal(1).scaleb(-places), rounding=ROUND_HALF_UP))


def _div(a, b):
    """Java's double division"""
    a, b = float(a), float(b)
    if b == 0:
        return math.nan if a == 0 or math.isnan(a) else math.copysign(math.inf, a)
    return a / b


def _phred(prob):
    """QualityTools.probErrorToPhredDouble (:511-517)"""
    if prob >= 1:
        return 0.0
    if prob <= 0.000001:
        return 60.0
    return -10 * math.log10(prob)


# Tools' histogram helpers (current/align2/Tools.java:1319-1339, :1887-1913, :2089-2097, :2131-2145) over exact Python integers
def _ints(a):
    return [int(x) for x in a]


def _percentile(a, fraction):
    a = _ints(a)
    if not a:
        return 0
    target = int(sum(a) * fraction)
    s = 0
    for i, x in enumerate(a):
        s += x
        if s >= target:
            return i
    return len(a) - 1


def _mode(a):
    a = _ints(a)
    if not a:
        return 0
    median = _percentile(a, 0.5)
    mode = 0
    for i in range(1, len(a)):
        if a[i] > a[mode] or (a[i] == a[mode] and abs(i - median) < abs(mode - median)):
            mode = i
    return mode


def _average(a):
    a = _ints(a)
    return sum(x * i for i, x in enumerate(a)) / float(max(1, sum(a)))


def _stdev(a):
    a = _ints(a)
    s = max(1, sum(a))
    avg = sum(x * i for i, x in enumerate(a)) / float(s)
    dev2 = 0.0
    for i, x in enumerate(a):
        dev = avg - i
        dev2 += x * (dev * dev)
    return math.sqrt(dev2 / s)


def _first(a):
    nz = np.flatnonzero(a)
    return int(nz[0]) if len(nz) else 0


def _last(a):
    nz = np.flatnonzero(a)
    return int(nz[-1]) if len(nz) else 0


class ReadHist:
    """A host copy of the state: .flags, .block (int64[words]) and one array per selected group member under the names of
    bbmap_readhist_view (views of the block; "del" as .del_ too); an array of a group that is not selected is None."""

    def __init__(self, flags, block):
        L = LL.load()
        self.flags = int(flags)
        self.block = np.ascontiguousarray(block, np.int64)
        w = bbmap_readhist_view()
        LL.check(L.bbpipe_read_hist_view(self.flags, C.c_void_p(self.block.ctypes.data), C.byref(w)), "bbpipe_read_hist_view")
        assert w.words == self.block.size
        self.arrays = {}
        for name, shape in SHAPES:
            p = getattr(w, name if name != "del" else "del_")
            a = None
            if p:
                off = (p - self.block.ctypes.data) // 8
                a = self.block[off:off + int(np.prod(shape))].reshape(shape)
            self.arrays[name] = a
            setattr(self, name if name != "del" else "del_", a)

    # ---- the scalars and the derived arrays
    @property
    def gc_hist(self):
        return self.gc[:RH_GC_BINS + 1]

    @property
    def gc_max_read_len(self):
        return max(1, int(self.gc[RH_GC_BINS + 1]))          # the class starts at 1 (:1292)

    @property
    def id_hist(self):
        return self.identity[:RH_ID_BINS + 1]

    @property
    def id_base_hist(self):
        return self.identity[RH_ID_BINS + 1:2 * (RH_ID_BINS + 1)]

    @property
    def id_max_read_len(self):
        return max(1, int(self.identity[2 * (RH_ID_BINS + 1)]))

    def qual_sum(self):
        """qualSum[2][MAXLEN], exact"""
        return (self.bqual * np.arange(RH_QUAL_BINS, dtype=np.int64)).sum(axis=2)

    def qual_sum_double(self):
        """qualSumDouble[2][MAXLEN]"""
        return (self.bqual.astype(np.float64) * PROB_ERROR.astype(np.float64)).sum(axis=2)

    def bqual_overall(self):
        return self.qcount[0] + self.qcount[1]

    # ---- the files
    def mhist_lines(self, paired):
        """writeMatchToFile / writeMatchToFileUnpaired (:987-1047)"""
        out = ["#BaseNum\tMatch1\tSub1\tDel1\tIns1\tN1\tOther1" + ("\tMatch2\tSub2\tDel2\tIns2\tN2\tOther2" if paired else "")]
        ms, ss, ds, is_, ns, cs, os_ = self.match
        sums = ms + is_ + ss + ns + cs + os_                # no deletions
        for i in range(RH_MAXLEN):
            if sums[0][i] == 0 and (not paired or sums[1][i] == 0):
                break
            line = str(i + 1)
            for p in range(2 if paired else 1):
                inv = 1.0 / float(max(1, int(sums[p][i])))
                line += "".join("\t" + jfmt(int(v) * inv, 5) for v in (ms[p][i], ss[p][i], ds[p][i], is_[p][i], ns[p][i], os_[p][i] + cs[p][i]))
            out.append(line)
        return out

    def _measured(self, pos, p):
        """calcQualityAtPosition (:816-829)"""
        m, s, d, i = (int(self.match[k][p][pos]) for k in range(4))
        d2 = int(self.match[2][p][min(pos, RH_MAXLEN - 1)])
        good, total = max(0, m * 2 - d - d2), max(0, m * 2 + i * 2 + s * 2)
        return 0.0 if total < 1 else _phred((total - good) / float(total))

    def qhist_rows(self, paired):
        """writeQualityToFile's numbers before they are printed: [(linear, log, measured or None) per mate] per position"""
        measure = self.match is not None
        ql = np.cumsum(self.qual_length[:, ::-1], axis=1)[:, ::-1]          # the suffix sums of :773-776
        qs, qsd = self.qual_sum(), self.qual_sum_double()
        rows = []
        for i in range(RH_MAXLEN):
            if not (ql[0][i] > 0 or (paired and ql[1][i] > 0)):
                break
            row = []
            for p in range(2 if paired else 1):
                n = float(max(1, int(ql[p][i])))
                row.append((int(qs[p][i]) / n, _phred(float(qsd[p][i]) / n), self._measured(i, p) if measure else None))
            rows.append(row)
        return rows

    def qhist_lines(self, paired):
        """writeQualityToFile (:756-814); the "measured" column when the match histogram was collected"""
        measure = self.match is not None
        head = "\tRead%d_linear\tRead%d_log" + ("\tRead%d_measured" if measure else "")
        out = ["#BaseNum" + "".join(head % ((p,) * (3 if measure else 2)) for p in ((1, 2) if paired else (1,)))]
        for i, row in enumerate(self.qhist_rows(paired)):
            out.append("\t".join([str(i + 1)] + [jfmt(v, 3) for cols in row for v in cols if v is not None]))
        return out

    def bqhist_lines(self, paired):
        """writeBQualityToFile (:865-907)"""
        out = ["#BaseNum" + "".join("\tcount_%d\tmin_%d\tmax_%d\tmean_%d\tQ1_%d\tmed_%d\tQ3_%d\tLW_%d\tRW_%d" % ((p,) * 9)
                                    for p in ((1, 2) if paired else (1,)))]
        totals = self.bqual.sum(axis=2)
        for i in range(RH_MAXLEN):
            if totals[0][i] < 1 and totals[1][i] < 1:
                break
            cols = [str(i)]
            for p in range(2 if paired else 1):
                a = self.bqual[p][i]
                weighted = sum(q * int(x) for q, x in enumerate(a))
                cols += [str(int(totals[p][i])), str(_first(a)), str(_last(a)), jfmt(_div(weighted * 1.0, max(int(totals[p][i]), 0)), 2)] + \
                    [str(_percentile(a, f)) for f in (0.25, 0.5, 0.75, 0.02, 0.98)]
            out.append("\t".join(cols))
        return out

    def bqhist_overall_lines(self):
        """writeBQualityOverallToFile (:831-863)"""
        h = self.bqual_overall()
        h30 = h.copy()
        h30[:30] = 0
        total = int(h.sum())
        mult = 1.0 / max(1, total)
        out = ["#Median\t%d" % _percentile(h, 0.5), "#Mean\t" + jfmt(_average(h), 3), "#STDev\t" + jfmt(_stdev(h), 3),
               "#Mean_30\t" + jfmt(_average(h30), 3), "#STDev_30\t" + jfmt(_stdev(h30), 3), "#Quality\tbases\tfraction"]
        left = total
        for i, x in enumerate(_ints(h)):
            left -= x
            out.append("%d\t%d\t%s" % (i, x, jfmt(x * mult, 5)))
            if left <= 0:
                break
        return out

    def qchist_lines(self, paired):
        """writeQCountToFile (:728-754)"""
        out = ["#Quality\tcount1\tfraction1" + ("\tcount2\tfraction2" if paired else "")]
        h = self.qcount
        s1, s2 = int(h[0].sum()), int(h[1].sum())
        m1, m2 = 1.0 / max(1, s1), 1.0 / max(1, s2)
        left = s1 + s2
        for i in range(RH_QUAL_BINS):
            x1, x2 = int(h[0][i]), int(h[1][i])
            left -= x1 + x2
            out.append("%d\t%d\t%s" % (i, x1, jfmt(x1 * m1, 5)) + ("\t%d\t%s" % (x2, jfmt(x2 * m2, 5)) if paired else ""))
            if left <= 0:
                break
        return out

    def bhist_lines(self, paired):
        """writeBaseContentToFile (:1060-1102): mate 2's positions go on counting where mate 1's end"""
        out = ["#Pos\tA\tC\tG\tT\tN"]
        offset = 0
        for p in range(2 if paired else 1):
            lists = self.base[p]
            nz = np.flatnonzero(lists.sum(axis=0))
            size = int(nz[-1]) + 1 if len(nz) else 0        # LongList.size
            for i in range(size):
                v = [int(lists[k][i]) for k in (1, 2, 3, 4, 0)]
                mult = _div(1.0, sum(v))
                out.append("%d\t" % (i + offset) + "\t".join(jfmt(x * mult, 5) for x in v))
            offset = size
        return out

    def qahist_lines(self):
        """writeQualityAccuracyToFile (:909-985)"""
        qmatch, qsub, qins, qdel = self.accuracy
        mx = _last(qmatch + qsub + qins + qdel) + 1 if (qmatch + qsub + qins + qdel).any() else 0
        devsum = devsum_sub = 0.0
        observations = 0
        rows = []
        for i in range(mx):
            qm, qs, qi, qd = int(qmatch[i]) * 2, int(qsub[i]) * 2, int(qins[i]) * 2, int(qdel[i])
            s = qm + qs + qi + qd
            row = "%d\t%d\t%d\t%d\t%d" % (i, qm, qs, qi, qd)
            if s > 0:
                mult = 1.0 / s
                phred_sub, phred = _phred(qs * mult), _phred((qs + qi + qd) * mult)
                dev, dev_sub = phred - i, phred_sub - i
                top = i == MAX_CALLED_QUALITY and mx == MAX_CALLED_QUALITY + 1
                if (i == MIN_CALLED_QUALITY and dev < 0) or (i != MIN_CALLED_QUALITY and top and dev > 0):
                    dev = 0
                if (i == MIN_CALLED_QUALITY and dev_sub < 0) or (i != MIN_CALLED_QUALITY and top and dev_sub > 0):
                    dev_sub = 0
                devsum += abs(dev) * s
                devsum_sub += abs(dev_sub) * s
                observations += s
                row += "\t" + jfmt(phred, 2) + "\t" + jfmt(phred_sub, 2)
            else:
                row += "\t\t"
            rows.append(row)
        return ["#Deviation\t" + jfmt(_div(devsum, observations), 3), "#DeviationSub\t" + jfmt(_div(devsum_sub, observations), 3),
                "#Quality\tMatch\tSub\tIns\tDel\tTrueQuality\tTrueQualitySub"] + rows

    def indelhist_lines(self):
        """writeIndelToFile (:1104-1132) with skipZeroIndel; delHist2 has no file (:1119-1127)"""
        d = np.zeros(RH_MAXINSLEN + 1, np.int64)
        d[:RH_MAXDELLEN] = self.del_
        return ["#Length\tDeletions\tInsertions"] + ["%d\t%d\t%d" % (i, int(d[i]), int(self.ins[i])) for i in range(len(d))
                                                     if d[i] > 0 or self.ins[i] > 0]

    def ehist_lines(self):
        """writeErrorToFile (:1134-1136)"""
        return ["#Errors\tCount"] + ["%d\t%d" % (i, int(self.error[i])) for i in np.flatnonzero(self.error)]

    def lhist_lines(self):
        """writeLengthToFile (:1138-1140)"""
        return ["#Length\tCount"] + ["%d\t%d" % (i, int(self.length[i])) for i in np.flatnonzero(self.length)]

    def gchist_lines(self, print_zeros=True):
        """writeGCToFile (:1164-1218)"""
        h = self.gc_hist
        mult = 100.0 / max(1, len(h) - 1)
        out = ["#Mean\t" + jfmt(_average(h) * mult, 3), "#Median\t" + jfmt(_percentile(h, 0.5) * mult, 3), "#Mode\t" + jfmt(_mode(h) * mult, 3),
               "#STDev\t" + jfmt(_stdev(h) * mult, 3), "#GC\tCount"]
        return out + ["%s\t%d" % (jfmt(i * mult, 1), int(x)) for i, x in enumerate(h) if x > 0 or print_zeros]

    def idhist_lines(self, print_zeros=True):
        """writeIdentityToFile (:1220-1255)"""
        h, hb = self.id_hist, self.id_base_hist
        mult = 100.0 / (len(h) - 1)
        rnd = lambda x: int(math.floor(x + 0.5))            # (int)Math.round
        out = ["#Mean_reads\t" + jfmt(_average(h) * mult, 3), "#Mean_bases\t" + jfmt(_average(hb) * mult, 3),
               "#Median_reads\t%d" % rnd(_percentile(h, 0.5) * mult), "#Median_bases\t%d" % rnd(_percentile(hb, 0.5) * mult),
               "#Mode_reads\t%d" % rnd(_mode(h) * mult), "#Mode_bases\t%d" % rnd(_mode(hb) * mult),
               "#STDev_reads\t" + jfmt(_stdev(h) * mult, 3), "#STDev_bases\t" + jfmt(_stdev(hb) * mult, 3), "#Identity\tReads\tBases"]
        return out + ["%s\t%d\t%d" % (jfmt(i * mult, 1), int(h[i]), int(hb[i])) for i in range(len(h)) if h[i] > 0 or print_zeros]


class DeviceState:
    """The raw calls' state for one set of groups, owned by the caller (a torch tensor): tests plant records and accumulate into it
    without mapping anything."""

    def __init__(self, flags, device=0):
        import torch
        self.flags = int(flags)
        self.dev = torch.device("cuda", device)
        self.state = torch.zeros(max(1, state_words(flags)), dtype=torch.int64, device=self.dev)
        self.words = state_words(flags)

    def add(self, reads, bases, quality, finals, pool, paired=False):
        """bbpipe_read_hist_add_device: reads / finals uint8 views of READ_DTYPE / FINAL_DTYPE records, bases / quality / pool uint8
        (device tensors; quality may be None)."""
        import torch
        L = LL.load()
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = torch.cuda.current_stream().cuda_stream
        LL.check(L.bbpipe_read_hist_add_device(C.c_void_p(stream), reads.numel() // READ_DTYPE.itemsize, int(paired), self.flags, ptr(reads), ptr(bases), ptr(quality),
                                               ptr(finals), ptr(pool), ptr(self.state)), "bbpipe_read_hist_add_device")
        torch.cuda.current_stream().synchronize()

    def reset(self):
        self.state.zero_()

    def read(self):
        return ReadHist(self.flags, self.state.cpu().numpy()[:self.words])
