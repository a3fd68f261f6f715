"""Test-local restatement of align2.ReadStats as BBMap's mapping threads feed it, the yardstick of the read-histogram tests,
sequential and loop for loop (current/align2/ReadStats.java): addToQualityHistogram2 / addToQualityHistogram / addToBQualityHistogram /
addToQCountHistogram (:273-328), addToQualityAccuracy (:336-387), addToErrorHistogram (:395-399, Read.countSubs,
current/stream/Read.java:1916-1925), addToLengthHistogram (:407-411), addToGCHistogram (:413-438, Read.gc, Read.java:2530-2542),
addToIdentityHistogram (:446-452, Read.identityFlat, Read.java:1529-1596), addToIndelHistogram (:472-508), addToMatchHistogram2
(:516-576), addToBaseHistogram2 (:648-664), and the writers (:728-1255) with the helpers of current/align2/Tools.java they call
(sumHistogram :1319, minHistogram :1327, maxHistogram :1334, percentile :1887, calcMode :1900, averageHistogram :2089,
standardDeviationHistogram :2131) and QualityTools (probErrorToPhredDouble :511-517, makeQualityToFloat :519-527).  Assertions are
off, as in a BBMap run; usePairGC, FLAT_IDENTITY, skipZeroIndel at their defaults; ID_BINS_AUTO / GC_BINS_AUTO / GC_PLOT_X off.

The library's stated deviations (include/bbmap_amd.h) are restated as such: a mapped read without a string takes no part in the
match histogram; the accuracy walk stops when rpos reaches the read's length; a quality above 98 counts in accuracy bin 98, one above
126 in quality bin 126; the error histogram's last bin (MAX_POS) takes every larger count."""
import math
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

MAXLEN, MAXINSLEN, MAXDELLEN, MAXDELLEN2, GC_BINS, ID_BINS = 6000, 1000, 1000, 1000000, 100, 100         # :1312-1321
MAX_POS = 6016                              # the library's longest read: positions of baseHist, bins of lengthHist / errorHist
MIN_CALLED_QUALITY, MAX_CALLED_QUALITY = 2, 41                                                       # Read.java:3407-3408

BASE_TO_NUMBER = [-1] * 256                 # AminoAcid.baseToNumber (current/dna/AminoAcid.java:615-624); the table has 128 slots
for _c, _v in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _c:
        BASE_TO_NUMBER[ord(_ch)] = _v

f32 = np.float32
PROB_ERROR = [f32(math.pow(10, 0 - .1 * i)) for i in range(127)]                                     # makeQualityToFloat(127)
PROB_ERROR[0] = f32(.8)


def defined(b):
    return BASE_TO_NUMBER[b] >= 0           # AminoAcid.isFullyDefined


def jfmt(x, places):
    """String.format("%.<places>f", x): the double's exact decimal value rounded HALF_UP; NaN prints as NaN"""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    return str(Decimal(x).quantize(Decimal(1).scaleb(-places), rounding=ROUND_HALF_UP))


def jround(x):
    """(int)Math.round(double)"""
    return int(math.floor(x + 0.5))


def ddiv(a, b):
    """Java's double division: x/0 is NaN or an infinity"""
    a, b = float(a), float(b)
    if b == 0:
        return math.nan if a == 0 or math.isnan(a) else math.copysign(math.inf, a)
    return a / b


# ---- Tools
def sum_histogram(a):
    return sum(i * int(a[i]) for i in range(1, len(a)))


def min_histogram(a):
    return next((i for i in range(len(a)) if a[i] > 0), 0)


def max_histogram(a):
    return next((i for i in range(len(a) - 1, -1, -1) if a[i] > 0), 0)


def percentile(a, fraction):
    if len(a) < 1:
        return 0
    target = int(sum(int(x) for x in a) * fraction)
    s = 0
    for i in range(len(a)):
        s += int(a[i])
        if s >= target:
            return i
    return len(a) - 1


def calc_mode(a):
    if len(a) < 1:
        return 0
    median = percentile(a, 0.5)
    mode, count = 0, int(a[0])
    for i in range(1, len(a)):
        c = int(a[i])
        if c > count or (c == count and abs(i - median) < abs(mode - median)):
            mode, count = i, c
    return mode


def average_histogram(a):
    s = max(1, sum(int(x) for x in a))
    return sum(int(a[i]) * i for i in range(len(a))) / float(s)


def stdev_histogram(a):
    s = max(1, sum(int(x) for x in a))
    avg = sum(int(a[i]) * i for i in range(len(a))) / float(s)
    dev2 = 0.0
    for i in range(len(a)):
        dev = avg - i
        dev2 += int(a[i]) * (dev * dev)
    return math.sqrt(dev2 / s)


def prob_error_to_phred(prob):
    if prob >= 1:
        return 0.0
    if prob <= 0.000001:
        return 60.0
    return -10 * math.log10(prob)


def identity_flat(match):
    """Read.identityFlat on a long-format string: the loop as written, digits and all"""
    if not match:
        return f32(0)
    good = bad = n = current = 0
    mode = c = ord("0")

    def close(mode, current, good, bad, n):
        if mode == ord("m"):
            good += current
        elif mode in (ord("R"), ord("N")):
            n += current
        elif mode == ord("C"):
            pass
        elif mode != ord("0"):
            bad += current                  # INTRON_LIMIT is Integer.MAX_VALUE: every D counts
        return good, bad, n
    for c in match:
        if ord("0") <= c <= ord("9"):
            current = current * 10 + (c - ord("0"))
        elif mode == c:
            current = max(current + 1, 2)
        else:
            current = max(current, 1)
            good, bad, n = close(mode, current, good, bad, n)
            mode, current = c, 0
    if current > 0 or not (ord("0") <= c <= ord("9")):
        current = max(current, 1)
        good, bad, n = close(mode, current, good, bad, n)
    n = (n + 3) // 4
    good += n
    bad += 3 * n
    return f32(good) / f32(max(good + bad, 1))


def read_gc(bases):
    """Read.gc"""
    at = gc = 0
    for b in bases:
        x = BASE_TO_NUMBER[b]
        if x > -1:
            if x == 0 or x == 3:
                at += 1
            else:
                gc += 1
    if gc < 1:
        return f32(0)
    return f32(gc) * f32(1) / f32(at + gc)


class ReadStats:
    """flags as BBMAP_RH_*: a group that is not selected is not collected (the class's COLLECT_* switches)"""
    MATCH, QUALITY, BASE, ACCURACY, INDEL, ERROR, LENGTH, GC, IDENTITY = 1, 2, 4, 8, 16, 32, 64, 128, 256
    ALL = 511

    def __init__(self, flags=511):
        z = lambda *shape: np.zeros(shape, np.int64)
        self.flags = flags
        self.match = z(7, 2, MAXLEN)                        # matchSum subSum delSum insSum nSum clipSum otherSum
        self.qualLength, self.qualSum, self.qualSumDouble = z(2, MAXLEN), z(2, MAXLEN), np.zeros((2, MAXLEN), np.float64)
        self.bqualHist, self.qcountHist, self.bqualHistOverall = z(2, MAXLEN, 127), z(2, 127), z(127)
        self.baseHist = z(2, 5, MAX_POS)
        self.accuracy = z(4, 99)                            # qualMatch qualSub qualIns qualDel
        self.insHist, self.delHist, self.delHist2 = z(MAXINSLEN + 1), z(MAXDELLEN), z(MAXDELLEN2 // 100 + 1)
        self.errorHist, self.lengthHist = z(MAX_POS + 1), z(MAX_POS + 1)
        self.gcHist, self.idHist, self.idBaseHist = z(GC_BINS + 1), z(ID_BINS + 1), z(ID_BINS + 1)
        self.gcMaxReadLen = self.idMaxReadLen = 1           # :1292-1293

    # ---- accumulation
    def add_read(self, bases, quality, mapped, strand, match, pairnum):
        """the per-read calls of AbstractMapThread.run's tail; match = None or b"" is a null string"""
        match = match or None
        f = self.flags
        if f & self.QUALITY:
            self.add_quality(quality, pairnum)
        if f & self.BASE:
            self.add_base(bases, pairnum)
        if f & self.LENGTH:
            self.lengthHist[min(len(bases), MAX_POS)] += 1  # :409-410 (MAXLENGTHLEN is never reached)
        if f & self.MATCH:
            self.add_match(bases, mapped, strand, match, pairnum)
        if f & self.ACCURACY:
            self.add_accuracy(bases, quality, mapped, strand, match)
        if f & self.ERROR and len(bases) >= 1 and mapped and match is not None:      # :396-398
            self.errorHist[min(sum(1 for m in match if m == ord("S")), MAX_POS)] += 1
        if f & self.INDEL:
            self.add_indel(bases, mapped, match)
        if f & self.IDENTITY and len(bases) >= 1 and mapped and match is not None:   # :447-451
            idf = identity_flat(match)
            b = int(idf * f32(ID_BINS))
            self.idHist[b] += 1
            self.idBaseHist[b] += len(bases)
            self.idMaxReadLen = max(len(bases), self.idMaxReadLen)

    def add_quality(self, qual, pairnum):
        if qual is None or len(qual) < 1:                   # :275
            return
        qual = [min(q, 126) for q in qual]                  # (the deviation: Java's tables end at 126)
        limit = min(len(qual), MAXLEN)                      # :300
        self.qualLength[pairnum][limit - 1] += 1
        for i in range(limit):
            self.qualSum[pairnum][i] += qual[i]
            self.qualSumDouble[pairnum][i] += float(PROB_ERROR[qual[i]])
            self.bqualHist[pairnum][i][qual[i]] += 1        # :317-319
        for q in qual:
            self.bqualHistOverall[q] += 1                   # :308-310
            self.qcountHist[pairnum][q] += 1                # :325-327

    def add_base(self, bases, pairnum):
        for i in range(min(len(bases), MAX_POS)):           # :659-663
            self.baseHist[pairnum][BASE_TO_NUMBER[bases[i]] + 1][i] += 1

    def add_gc(self, bases1, bases2):
        """addToGCHistogram with usePairGC; bases2 = None for a single read"""
        if not self.flags & self.GC:
            return
        len1, len2 = len(bases1), 0 if bases2 is None else len(bases2)
        gc1 = read_gc(bases1) if len1 > 0 else f32(-1)
        gc2 = read_gc(bases2) if len2 > 0 else f32(-1)
        with np.errstate(all="ignore"):
            gc = gc1 if bases2 is None else (gc1 * f32(len1) + gc2 * f32(len2)) / f32(len1 + len2)
        if gc < 0 or len1 + len2 < 1:                       # :435 (NaN < 0 is false; the length test returns)
            return
        self.gcHist[min(GC_BINS, int(gc * f32(GC_BINS + 1)))] += 1
        self.gcMaxReadLen = max(len1 + len2, self.gcMaxReadLen)

    def add_match(self, bases, mapped, strand, match, pairnum):
        if len(bases) < 1 or not mapped or match is None:   # :517 (and the deviation: no string, no counts)
            return
        limit = min(len(bases), MAXLEN)
        ms, ss, ds, is_, ns, cs, os_ = (self.match[k][pairnum] for k in range(7))
        plus = strand == 0
        rpos, lastm, mpos = 0, ord("A"), 0
        while mpos < len(match) and rpos < limit:           # :543
            b = bases[rpos]
            m = match[mpos if plus else len(match) - mpos - 1]
            if b == ord("N"):
                if m == ord("D"):
                    if lastm != m:
                        ds[rpos] += 1
                    rpos -= 1
                else:
                    ns[rpos] += 1
            elif m == ord("m"):
                ms[rpos] += 1
            elif m == ord("S"):
                ss[rpos] += 1
            elif m == ord("I"):
                is_[rpos] += 1
            elif m == ord("N"):
                os_[rpos] += 1
            elif m == ord("C"):
                cs[rpos] += 1
            elif m == ord("D"):
                if lastm != m:
                    ds[rpos] += 1
                rpos -= 1
            else:
                os_[rpos] += 1
            rpos += 1
            lastm = m
            mpos += 1

    def add_accuracy(self, bases, qual, mapped, strand, match):
        if qual is None or len(qual) < 1 or not mapped or match is None:             # :337
            return
        qm, qs, qi, qd = self.accuracy
        plus = strand == 0
        rpos, lastm = 0, ord("A")
        for mpos in range(len(match)):                      # :347
            if rpos >= len(bases):                          # (the deviation: Java throws here)
                break
            b, q = bases[rpos], min(qual[rpos], 98)
            m = match[mpos if plus else len(match) - mpos - 1]
            if m == ord("m"):
                qm[q] += 1
            elif m == ord("S"):
                qs[q] += 1
            elif m == ord("I"):
                if defined(b):
                    qi[q] += 1
            elif m == ord("N") or m == ord("C"):
                pass
            elif m == ord("D"):
                if lastm != m:
                    x, y = rpos, rpos - 1
                    if x < len(qual) and defined(bases[x]):
                        qd[min(qual[x], 98)] += 1
                    if y >= 0 and defined(bases[y]):
                        qd[min(qual[y], 98)] += 1
                rpos -= 1
            rpos += 1
            lastm = m

    def add_indel(self, bases, mapped, match):
        if len(bases) < 1 or not mapped or match is None:   # :473
            return
        limit = min(len(bases), MAXLEN)
        rpos = streak = 0
        lastm = ord("A")

        def close(lastm, streak):
            if lastm == ord("D"):
                streak = min(streak, MAXDELLEN2)
                if streak < MAXDELLEN:
                    self.delHist[streak] += 1
                self.delHist2[streak // 100] += 1
            elif lastm == ord("I"):
                self.insHist[min(streak, MAXINSLEN)] += 1
        mpos = 0
        while mpos < len(match) and rpos < limit:           # :480
            m = match[mpos]
            if lastm != m:
                close(lastm, streak)
                streak = 0
            streak += 1
            rpos += 1
            lastm = m
            mpos += 1
        close(lastm, streak)                                # :500-507

    def add_batch(self, reads, quals, fin, matches, paired):
        """reads: byte strings; quals: byte strings or None; fin: records with mapped / strand; matches: byte strings or None"""
        for r, bases in enumerate(reads):
            q = None if quals is None else quals[r]
            self.add_read(bases, q, bool(fin[r]["mapped"]), int(fin[r]["strand"]), matches[r], r & 1 if paired else 0)
            if paired and r & 1:
                self.add_gc(reads[r - 1], bases)
            elif not paired:
                self.add_gc(bases, None)

    def arrays(self):
        """name -> array, in the shapes the library's state has (the running float sums are not part of it)"""
        f, out = self.flags, {}
        if f & self.MATCH:
            out["match"] = self.match
        if f & self.QUALITY:
            out.update(qual_length=self.qualLength, bqual=self.bqualHist, qcount=self.qcountHist)
        if f & self.BASE:
            out["base"] = self.baseHist
        if f & self.ACCURACY:
            out["accuracy"] = self.accuracy
        if f & self.INDEL:
            out.update(ins=self.insHist, **{"del": self.delHist}, del2=self.delHist2)
        if f & self.ERROR:
            out["error"] = self.errorHist
        if f & self.LENGTH:
            out["length"] = self.lengthHist
        if f & self.GC:
            out["gc"] = np.concatenate([self.gcHist, [self.gcMaxReadLen]])
        if f & self.IDENTITY:
            out["identity"] = np.concatenate([self.idHist, self.idBaseHist, [self.idMaxReadLen]])
        return out

    # ---- the writers: lists of lines
    def write_qcount(self, paired):                         # :728-754
        out = ["#Quality\tcount1\tfraction1" + ("\tcount2\tfraction2" if paired else "")]
        h = self.qcountHist
        sum1, sum2 = int(h[0].sum()), int(h[1].sum())
        mult1, mult2 = 1.0 / max(1, sum1), 1.0 / max(1, sum2)
        y = sum1 + sum2
        for i in range(h.shape[1]):
            x1, x2 = int(h[0][i]), int(h[1][i])
            y -= x1 + x2
            line = "%d\t%d\t%s" % (i, x1, jfmt(x1 * mult1, 5))
            if paired:
                line += "\t%d\t%s" % (x2, jfmt(x2 * mult2, 5))
            out.append(line)
            if y <= 0:
                break
        return out

    def calc_quality_at_position(self, pos, pairnum):       # :816-829
        m, s, d, i = (int(self.match[k][pairnum][pos]) for k in range(4))
        d2 = int(self.match[2][pairnum][min(pos, MAXLEN - 1)])
        good = max(0, m * 2 - d - d2)
        total = max(0, m * 2 + i * 2 + s * 2)
        bad = total - good
        if total < 1:
            return 0.0
        return prob_error_to_phred(bad / float(total))

    def quality_rows(self, paired):
        """writeQualityToFile's numbers before they are printed: [(blin, blog, bcalc or None) per mate] per position (:770-810)"""
        measure = bool(self.flags & self.MATCH)
        ql = self.qualLength.copy()                         # (the class sums in place; a second call would sum twice)
        for i in range(MAXLEN - 2, -1, -1):
            ql[0][i] += ql[0][i + 1]
            ql[1][i] += ql[1][i + 1]
        rows = []
        for i in range(MAXLEN):
            if not (ql[0][i] > 0 or (paired and ql[1][i] > 0)):
                break
            row = []
            for p in range(2 if paired else 1):
                lin = int(self.qualSum[p][i]) / float(max(1, int(ql[p][i])))
                log = prob_error_to_phred(float(self.qualSumDouble[p][i]) / float(max(1, int(ql[p][i]))))
                row.append((lin, log, self.calc_quality_at_position(i, p) if measure else None))
            rows.append(row)
        return rows

    def write_quality(self, paired):                        # :756-814
        measure = bool(self.flags & self.MATCH)
        if measure:
            out = ["#BaseNum\tRead1_linear\tRead1_log\tRead1_measured" + ("\tRead2_linear\tRead2_log\tRead2_measured" if paired else "")]
        else:
            out = ["#BaseNum\tRead1_linear\tRead1_log" + ("\tRead2_linear\tRead2_log" if paired else "")]
        for i, row in enumerate(self.quality_rows(paired)):
            out.append("\t".join([str(i + 1)] + [jfmt(v, 3) for cols in row for v in cols if v is not None]))
        return out

    def write_bquality_overall(self):                       # :831-863
        h = self.bqualHistOverall
        cp30 = h.copy()
        cp30[:30] = 0
        total = int(h.sum())
        mult = 1.0 / max(1, total)
        out = ["#Median\t%d" % percentile(h, 0.5), "#Mean\t" + jfmt(average_histogram(h), 3), "#STDev\t" + jfmt(stdev_histogram(h), 3),
               "#Mean_30\t" + jfmt(average_histogram(cp30), 3), "#STDev_30\t" + jfmt(stdev_histogram(cp30), 3), "#Quality\tbases\tfraction"]
        y = total
        for i in range(len(h)):
            x = int(h[i])
            y -= x
            out.append("%d\t%d\t%s" % (i, x, jfmt(x * mult, 5)))
            if y <= 0:
                break
        return out

    def write_bquality(self, paired):                       # :865-907
        out = ["#BaseNum\tcount_1\tmin_1\tmax_1\tmean_1\tQ1_1\tmed_1\tQ3_1\tLW_1\tRW_1" +
               ("\tcount_2\tmin_2\tmax_2\tmean_2\tQ1_2\tmed_2\tQ3_2\tLW_2\tRW_2" if paired else "")]
        for i in range(MAXLEN):
            a1, a2 = self.bqualHist[0][i], self.bqualHist[1][i]
            if a1.sum() < 1 and a2.sum() < 1:
                break
            cols = [str(i)]
            for a in (a1, a2) if paired else (a1,):
                s = int(a.sum())
                mean = ddiv(sum_histogram(a) * 1.0, max(s, 0))
                cols += [str(s), str(min_histogram(a)), str(max_histogram(a)), jfmt(mean, 2), str(percentile(a, 0.25)), str(percentile(a, 0.5)),
                         str(percentile(a, 0.75)), str(percentile(a, 0.02)), str(percentile(a, 0.98))]
            out.append("\t".join(cols))
        return out

    def write_quality_accuracy(self):                       # :909-985
        qmatch, qsub, qins, qdel = self.accuracy
        mx = len(qmatch)
        for i in range(mx - 1, -1, -1):
            if qmatch[i] + qsub[i] + qins[i] + qdel[i] > 0:
                break
            mx = i
        devsum = devsum_sub = 0.0
        observations = 0
        rows = []
        for i in range(mx):
            qm, qs, qi, qd = int(qmatch[i]) * 2, int(qsub[i]) * 2, int(qins[i]) * 2, int(qdel[i])
            phred = phred_sub = -1.0
            s = qm + qs + qi + qd
            if s > 0:
                mult = 1.0 / s
                phred_sub = prob_error_to_phred(qs * mult)
                phred = prob_error_to_phred((qs + qi + qd) * mult)
                dev, dev_sub = phred - i, phred_sub - i
                if i == MIN_CALLED_QUALITY and dev < 0:
                    dev = 0
                elif i == MAX_CALLED_QUALITY and mx == MAX_CALLED_QUALITY + 1 and dev > 0:
                    dev = 0
                if i == MIN_CALLED_QUALITY and dev_sub < 0:
                    dev_sub = 0
                elif i == MAX_CALLED_QUALITY and mx == MAX_CALLED_QUALITY + 1 and dev_sub > 0:
                    dev_sub = 0
                devsum += abs(dev) * s
                devsum_sub += abs(dev_sub) * s
                observations += s
            rows.append("%d\t%d\t%d\t%d\t%d" % (i, qm, qs, qi, qd) + ("\t" + jfmt(phred, 2) if phred >= 0 else "\t") +
                        ("\t" + jfmt(phred_sub, 2) if phred_sub >= 0 else "\t"))
        return ["#Deviation\t" + jfmt(ddiv(devsum, observations), 3), "#DeviationSub\t" + jfmt(ddiv(devsum_sub, observations), 3),
                "#Quality\tMatch\tSub\tIns\tDel\tTrueQuality\tTrueQualitySub"] + rows

    def write_match(self, paired):                          # :987-1047
        out = ["#BaseNum\tMatch1\tSub1\tDel1\tIns1\tN1\tOther1" + ("\tMatch2\tSub2\tDel2\tIns2\tN2\tOther2" if paired else "")]
        ms, ss, ds, is_, ns, cs, os_ = self.match
        for i in range(MAXLEN):
            sums = [int(ms[p][i] + is_[p][i] + ss[p][i] + ns[p][i] + cs[p][i] + os_[p][i]) for p in range(2)]      # no deletions
            if sums[0] == 0 and (not paired or sums[1] == 0):
                break
            line = str(i + 1)
            for p in range(2 if paired else 1):
                inv = 1.0 / float(max(1, sums[p]))
                line += "".join("\t" + jfmt(int(v) * inv, 5) for v in (ms[p][i], ss[p][i], ds[p][i], is_[p][i], ns[p][i], os_[p][i] + cs[p][i]))
            out.append(line)
        return out

    def write_base_content(self, paired):                   # :1060-1102
        out = ["#Pos\tA\tC\tG\tT\tN"]
        offset = 0
        for p in range(2 if paired else 1):
            lists = self.baseHist[p]
            nz = np.flatnonzero(lists.sum(axis=0))
            mx = int(nz[-1]) + 1 if len(nz) else 0          # LongList.size: one past the last position incremented
            for i in range(mx):
                a, c, g, t, n = (int(lists[k][i]) for k in (1, 2, 3, 4, 0))
                mult = ddiv(1.0, a + c + g + t + n)
                out.append("%d\t" % (i + offset) + "\t".join(jfmt(v * mult, 5) for v in (a, c, g, t, n)))
            offset = mx
        return out

    def write_indel(self):                                  # :1104-1132, skipZeroIndel
        out = ["#Length\tDeletions\tInsertions"]
        for i in range(max(len(self.insHist), len(self.delHist))):
            x = int(self.delHist[i]) if i < len(self.delHist) else 0
            y = int(self.insHist[i]) if i < len(self.insHist) else 0
            if x > 0 or y > 0:
                out.append("%d\t%d\t%d" % (i, x, y))
        return out

    @staticmethod
    def _write_histogram(header, hist):                     # :1146-1162, printZeros false
        return [header] + ["%d\t%d" % (i, int(x)) for i, x in enumerate(hist) if x > 0]

    def write_error(self):                                  # :1134-1136
        return self._write_histogram("#Errors\tCount", self.errorHist)

    def write_length(self):                                 # :1138-1140
        return self._write_histogram("#Length\tCount", self.lengthHist)

    def write_gc(self, print_zeros=True):                   # :1164-1218
        hist = self.gcHist
        bins = len(hist)
        gc_mult = 100.0 / max(1, bins - 1)
        out = ["#Mean\t" + jfmt(average_histogram(hist) * gc_mult, 3), "#Median\t" + jfmt(percentile(hist, 0.5) * gc_mult, 3),
               "#Mode\t" + jfmt(calc_mode(hist) * gc_mult, 3), "#STDev\t" + jfmt(stdev_histogram(hist) * gc_mult, 3), "#GC\tCount"]
        for i in range(bins):
            x = int(hist[i])
            if x > 0 or print_zeros:
                out.append("%s\t%d" % (jfmt(i * gc_mult, 1), x))
        return out

    def write_identity(self, print_zeros=True):             # :1220-1255
        hist, histb = self.idHist, self.idBaseHist
        mx = len(hist)
        mult = 100.0 / (mx - 1)
        out = ["#Mean_reads\t" + jfmt(average_histogram(hist) * mult, 3), "#Mean_bases\t" + jfmt(average_histogram(histb) * mult, 3),
               "#Median_reads\t%d" % jround(percentile(hist, 0.5) * mult), "#Median_bases\t%d" % jround(percentile(histb, 0.5) * mult),
               "#Mode_reads\t%d" % jround(calc_mode(hist) * mult), "#Mode_bases\t%d" % jround(calc_mode(histb) * mult),
               "#STDev_reads\t" + jfmt(stdev_histogram(hist) * mult, 3), "#STDev_bases\t" + jfmt(stdev_histogram(histb) * mult, 3),
               "#Identity\tReads\tBases"]
        for i in range(mx):
            x, x2 = int(hist[i]), int(histb[i])
            if x > 0 or print_zeros:
                out.append("%s\t%d\t%d" % (jfmt(i * mult, 1), x, x2))
        return out
