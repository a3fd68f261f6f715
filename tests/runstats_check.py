"""A sequential restatement of the reference's run statistics, read by read, as the Java text has them:
AbstractMapThread.calcStatistics1 / calcStatistics2 (current/align2/AbstractMapThread.java:1478-1641, :1644-1770), calcCorrectness
(:2615-2689), Read.countErrors (current/stream/Read.java:2189-2240), Read.insertSizeMapped* (:2618-2670),
ReadStats.addToInsertHistogram (current/align2/ReadStats.java:578-592) and the two adaptive rules (BBMapThread.java:1307-1309,
AbstractMapThread.java:1146).  Fixed defaults: AMBIGUOUS_TOSS = false, OUTPUT_PAIRED_ONLY = false, INTRON_LIMIT = Integer.MAX_VALUE.
perfectHit and lowQualityReadsDiscarded are not restated (they need quickMap's return value): an unmapped read is a noHit.

Inputs are plain Python: per read a final record (anything indexable by bbmap_final's field names), its match string (bytes or None),
its site list (a sequence of records with bbmap_msite's field names), its length and its truth record (or None)."""
import numpy as np

from bbmap_amd.runstats import INSERT_HIST_BINS, PAIR_LEVEL, PER_MATE, RUNSTATS_DTYPE

MIN_PAIR_DIST, MAX_PAIR_DIST = -160, 32000                  # AbstractMapThread.java:2974-2975
MAXINSERTLEN = INSERT_HIST_BINS - 1                         # ReadStats.java:1313
POINTS = {0: (70, 100), 1: (90, 100)}                       # POINTS_MATCH, POINTS_MATCH2: MultiStateAligner11ts / MultiStateAligner9PacBio


def max_quality(scheme, length):
    """MSA.maxQuality(len) = POINTS_MATCH + (len - 1) * POINTS_MATCH2"""
    a, b = POINTS[scheme]
    return a + (length - 1) * b


def count_errors(match):
    """Read.countErrors (:2189-2240) -> (m, s, d, i, n); the splice count is left out (minSplice = Integer.MAX_VALUE)"""
    m = s = d = i = n = 0
    for b in bytes(match):
        c = chr(b)
        if c == "m":
            m += 1
        elif c in "NC":
            n += 1
        elif c in "XY":
            i += 1
        elif c == "I":
            i += 1
        elif c == "D":
            d += 1
        elif c == "S":
            s += 1
        else:
            raise ValueError("Unknown symbol %r" % c)
    return m, s, d, i, n


def _absdif(a, b):
    return a - b if a > b else b - a


def is_correct_hit(ss, chrom, strand, start, stop, thresh):             # :2692-2700
    if int(ss["chrom"]) != chrom or int(ss["strand"]) != strand:
        return False
    return _absdif(int(ss["start"]), start) <= thresh and _absdif(int(ss["stop"]), stop) <= thresh


def is_correct_hit_loose(ss, chrom, strand, start, stop, thresh):       # :2712-2719
    if int(ss["chrom"]) != chrom or int(ss["strand"]) != strand:
        return False
    return _absdif(int(ss["start"]), start) <= thresh or _absdif(int(ss["stop"]), stop) <= thresh


def calc_correctness(sites, truth, thresh):
    """calcCorrectness (:2615-2689) -> the reference's eleven values, in its order"""
    if sites is None or len(sites) == 0:
        return [-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    original = truth if truth is not None and int(truth["chrom"]) >= 0 else sites[0]       # :2623-2627
    oc, os_, oa, ob = (int(original[k]) for k in ("chrom", "strand", "start", "stop"))
    group, correct_group, group_size, correct_group_size = 0, -1, 0, -1
    prev_score = 2 ** 31 - 1
    size_of_top_group = 0
    correct = None
    first_correct = first_loose = first_group_loose = num_correct = 0
    for i, ss in enumerate(sites):
        if int(ss["score"]) == int(sites[0]["score"]):
            size_of_top_group += 1
        if prev_score != int(ss["score"]):
            if correct_group == group:
                correct_group_size = group_size
            group += 1
            group_size = 0
            prev_score = int(ss["score"])
        group_size += 1
        b = is_correct_hit(ss, oc, os_, oa, ob, thresh)
        b2 = is_correct_hit_loose(ss, oc, os_, oa, ob, thresh + 20)
        if b:
            if i == 0:
                first_correct = 1
            num_correct += 1
            if correct is None:
                correct = ss
                correct_group = group
        if b2:
            if i == 0:
                first_loose = 1
            if group == 0:
                first_group_loose = 1
    if correct_group == group:
        correct_group_size = group_size
    return [correct_group, correct_group_size, group, len(sites), 0 if correct is None else int(correct["score"]), int(sites[0]["score"]),
            size_of_top_group, num_correct, first_correct, first_loose, first_group_loose]


class _R:                                                   # the fields of stream.Read the insert size reads
    def __init__(self, f, length):
        self.strand, self.start, self.stop, self.chrom = (int(f[k]) for k in ("strand", "start", "stop", "chrom"))
        self.mapped, self.length = bool(int(f["mapped"])), length


def insert_unstranded(r1, r2):                              # Read.java:2643-2670 (r2 != null)
    if r1.start > r2.start:
        return insert_unstranded(r2, r1)
    if r1.start == r1.stop or r2.start == r2.stop:
        return 0
    if r1.chrom != r2.chrom:
        return 0
    a, b = r1.length, r2.length
    if r1.start < r2.start:
        mid = r2.start - r1.stop - 1
        if -mid >= a + b:
            return 0
        return mid + a + b
    return min(a, b)


def insert_plus_left(r1, r2):                               # :2629-2641
    if r1.strand > r2.strand:
        return insert_plus_left(r2, r1)
    if r1.strand == r2.strand or r1.start > r2.stop:
        return insert_unstranded(r2, r1)
    if r1.chrom != r2.chrom:
        return 0
    if r1.start == r1.stop or r2.start == r2.stop:
        return 0
    a, b = r1.length, r2.length
    mid = r2.start - r1.stop - 1
    if -mid >= a + b:
        return insert_unstranded(r1, r2)
    return mid + a + b


def insert_size_mapped(r1, r2, ignore_strand=False):        # :2622-2626
    if ignore_strand or r2 is None or not r1.mapped or not r2.mapped or r1.strand == r2.strand:
        return insert_unstranded(r1, r2)
    return insert_plus_left(r1, r2)


def _stats_one(S, sfx, f, match, sites, length, truth, scheme, thresh):
    """the part calcStatistics1 and calcStatistics2 share; returns calcCorrectness' `elements`"""
    add = lambda k, v=1: S.__setitem__(k + sfx, S[k + sfx] + int(v))
    mapped, plus = bool(int(f["mapped"])), int(f["strand"]) == 0
    if int(f["ambiguous"]) and mapped:                      # :1484 / :1647
        add("ambiguousBestAlignment"); add("ambiguousBestAlignmentBases", length)
    c = calc_correctness(sites, truth, thresh)
    correct_group, elements, size_of_top, num_correct, first_correct, first_loose = c[0], c[3], c[6], c[7], c[8] == 1, c[9] == 1
    if elements > 0:
        if match is not None:
            m, s, d, i, n = count_errors(match)
            add("matchCountM", m); add("matchCountS", s); add("matchCountD", d); add("matchCountI", i); add("matchCountN", n)
            add("readCountS", s > 0); add("readCountD", d > 0); add("readCountI", i > 0); add("readCountN", n > 0)
            add("readCountE", s > 0 or d > 0 or i > 0)
        add("mappedRetained"); add("mappedRetainedBases", length)
        if int(f["rescued"]):
            add("rescuedP" if plus else "rescuedM")
        max_sw = max_quality(scheme, length)
        if int(f["perfect"]) or (max_sw > 0 and int(sites[0]["slowScore"]) == max_sw):       # :1565 / :1693
            add("perfectMatch"); add("perfectMatchBases", length)
        found_semi = 0
        for ss in sites:
            if int(ss["perfect"]):
                add("perfectHitCount")
            if int(ss["semiperfect"]):
                add("semiPerfectHitCount")
                found_semi = 1
        add("semiperfectMatch", found_semi)
        if found_semi:
            add("semiperfectMatchBases", length)
        if first_correct:
            add("firstSiteCorrectP" if plus else "firstSiteCorrectM")
            add("firstSiteCorrectPaired" if int(f["paired"]) else "firstSiteCorrectSolo")
            if int(f["rescued"]):
                add("firstSiteCorrectRescued")
        else:
            add("firstSiteIncorrect")
        add("firstSiteCorrectLoose" if first_loose else "firstSiteIncorrectLoose")
        add("siteSum", elements); add("topSiteSum", size_of_top)
        if size_of_top == 1:
            add("uniqueHit")
        if correct_group > 0:
            add("truePositiveP" if plus else "truePositiveM")
            add("totalCorrectSites", num_correct)
            if correct_group == 1:
                add("correctUniqueHit" if size_of_top == 1 else "correctMultiHit")
            else:
                add("correctLowHit")
        else:
            add("falsePositive")
    else:
        add("noHit")
    return elements


def run_stats(finals, matches, site_lists, lens, paired, truth=None, scheme=0, thresh=0, max_pair_dist=MAX_PAIR_DIST, stats=None, hist=None):
    """Adds a batch to (stats, hist) -- made when None -- and returns them: stats a dict of RUNSTATS_DTYPE's names, hist int64[40001]."""
    S = stats if stats is not None else {n: 0 for n in RUNSTATS_DTYPE.names}
    H = hist if hist is not None else np.zeros(INSERT_HIST_BINS, np.int64)
    n = len(finals)
    tr = lambda r: None if truth is None else truth[r]
    step = 2 if paired else 1
    for r in range(0, n, step):
        f, length = finals[r], int(lens[r])
        has_mate = paired
        f2 = finals[r + 1] if has_mate else None
        # ---- calcStatistics1
        len1 = length
        len2 = 0 if not has_mate else length                # :1481 `len2=(r2==null ? 0 : r.length())`
        S["readsUsed1"] += 1; S["basesUsed1"] += length
        mapped = bool(int(f["mapped"]))
        mate_mapped = has_mate and bool(int(f2["mapped"]))
        if not mapped and (not has_mate or not mate_mapped):            # :1489-1496
            S["bothUnmapped"] += 1; S["bothUnmappedBases"] += length
            if has_mate:
                S["bothUnmapped"] += 1; S["bothUnmappedBases"] += int(lens[r + 1])
        elements = _stats_one(S, "1", f, matches[r], site_lists[r], length, tr(r), scheme, thresh)
        if elements > 0:
            if int(f["paired"]):                            # :1542-1559
                S["numMated"] += 1; S["numMatedBases"] += len1 + len2
                if int(f["start"]) <= int(f2["start"]):
                    inner, outer = int(f2["start"]) - int(f["stop"]), int(f2["stop"]) - int(f["start"])
                else:
                    inner, outer = int(f["start"]) - int(f2["stop"]), int(f["stop"]) - int(f2["start"])
                inner = min(max_pair_dist, inner)
                inner = max(MIN_PAIR_DIST, inner)
                S["innerLengthSum"] += inner; S["outerLengthSum"] += outer
                S["insertSizeSum"] += inner + length + int(lens[r + 1])
            elif has_mate and mate_mapped:
                S["badPairs"] += 1; S["badPairBases"] += len1 + len2
        if has_mate:
            # ---- calcStatistics2
            S["readsUsed2"] += 1; S["basesUsed2"] += int(lens[r + 1])
            _stats_one(S, "2", f2, matches[r + 1], site_lists[r + 1], int(lens[r + 1]), tr(r + 1), scheme, thresh)
            # ---- AbstractMapThread.java:524 + ReadStats.addToInsertHistogram(r, false)
            if int(f["paired"]) and mapped and mate_mapped:
                x = min(MAXINSERTLEN, insert_size_mapped(_R(f, length), _R(f2, int(lens[r + 1])), False))
                if x > 0:
                    H[x] += 1
    return S, H


def java_average_pair_dist(inner_length_sum, num_mated):
    """(int)(innerLengthSum*1f/numMated) (BBMapThread.java:1308): long -> float, float * 1f, / (float)numMated, truncation"""
    q = np.float32(np.float32(np.float32(inner_length_sum) * np.float32(1.0)) / np.float32(num_mated))
    return int(q)


def insert_length_rule(stats, batch_held_paired, current):
    """DYNAMIC_INSERT_LENGTH (BBMapThread.java:1307-1309), once per batch"""
    if int(stats["numMated"]) > 1000 and batch_held_paired:
        return java_average_pair_dist(int(stats["innerLengthSum"]), int(stats["numMated"]))
    return current


def rescue_skip_rule(stats):
    """`if(mappedRetained2>1000 && numMated*20L<mappedRetained2){return;}` (AbstractMapThread.java:1146)"""
    return int(stats["mappedRetained2"]) > 1000 and int(stats["numMated"]) * 20 < int(stats["mappedRetained2"])


def as_record(stats):
    out = np.zeros(1, RUNSTATS_DTYPE)
    for k in RUNSTATS_DTYPE.names:
        out[0][k] = stats[k]
    return out[0]


def differences(got, want):
    """names whose values differ between a RUNSTATS_DTYPE scalar and a restatement dict"""
    return [(k, int(got[k]), int(want[k])) for k in RUNSTATS_DTYPE.names if int(got[k]) != int(want[k])]


def merged_site_lists(out):
    """per-read site lists of a Mapper.fetch() result, the overflow tier's lists in place of the reads it mapped"""
    ns, sites = out["nsites"], out["sites"]
    lists = [sites[r][:max(0, int(ns[r]))] for r in range(len(ns))]
    ov = out.get("overflow")
    if ov is not None:
        for i, r in enumerate(ov["read_ids"]):
            if int(ns[int(r)]) == -3:
                lists[int(r)] = ov["sites"][i][:max(0, int(ov["nsites"][i]))]
    return lists


# ---- a Mapper's last step against the restatement (GPU tests; the device imports stay inside)
def restate(mp, reads, paired, truth, scheme=0):
    """(final records, match strings, site lists, lengths) of a Mapper's last step as run_stats takes them; a read the overflow tier
    mapped takes the tier's record, string and list.  reads: anything whose items have the reads' lengths."""
    import ctypes as C

    from bbmap_amd.mapper import FINAL_DTYPE, _copy, bbmap_overflow_output
    out = mp.fetch(with_match=False)
    fin, blob = mp.final()
    matches = [blob[int(f["match_off"]): int(f["match_off"]) + int(f["match_len"])].tobytes() if int(f["match_len"]) > 0 else None for f in fin]
    lists = merged_site_lists(out)
    lens = [len(r) for r in reads]
    # a read the tier mapped (nsites == -3 in the main list) takes the tier's own record and string, read from the tier's output
    ov = bbmap_overflow_output()
    assert mp.L.bbmap_get_overflow_output(mp.h, C.byref(ov)) == 0
    if ov.n_reads > 0:
        nt = int(ov.n_reads)
        tf = _copy(ov.out.final, nt * FINAL_DTYPE.itemsize).view(FINAL_DTYPE)
        tpool = _copy(ov.out.final_match, int(ov.out.final_match_bytes))
        ids = _copy(ov.read_ids, nt * 4).view(np.int32)
        fin = fin.copy()
        for i, r in enumerate(ids):
            if int(out["nsites"][int(r)]) == -3:
                fin[int(r)] = tf[i]
                o, ml = int(tf[i]["match_off"]), int(tf[i]["match_len"])
                matches[int(r)] = tpool[o: o + ml].tobytes() if ml > 0 else None
    return fin, matches, lists, lens


def check_mapped(mp, reads, paired, truth, scheme=0):
    """bbmap_add_run_stats / bbmap_get_run_stats over a Mapper's last step against run_stats given the context's maxPairDist: every
    counter and the insert-size histogram, and what holds independently of the restatement.  Returns (got, want)."""
    fin, matches, lists, lens = restate(mp, reads, paired, truth, scheme)
    want, whist = run_stats(fin, matches, lists, lens, paired, truth, scheme, 0, mp.cfg.maxPairDist)
    mp.reset_run_stats()
    mp.add_run_stats(truth)
    got, hist = mp.run_stats()
    assert not differences(got, want), differences(got, want)
    assert np.array_equal(hist, whist)
    # ---- independent of the restatement
    withstr = sum(lens[r] for r in range(len(fin)) if len(lists[r]) > 0 and matches[r] is not None)
    assert sum(int(got["matchCount%s%d" % (c, m)]) for c in "MSIN" for m in (1, 2)) == withstr
    for m in ("1", "2"):
        assert sum(int(got[k + m]) for k in ("firstSiteCorrectP", "firstSiteCorrectM", "firstSiteIncorrect")) == int(got["mappedRetained" + m])
    if paired:
        pos = 0
        for r in range(0, len(fin), 2):
            a, b = fin[r], fin[r + 1]
            if a["paired"] and a["mapped"] and b["mapped"]:
                pos += insert_size_mapped(_R(a, lens[r]), _R(b, lens[r + 1])) > 0
        assert int(hist.sum()) == pos
    else:
        assert hist.sum() == 0
    return got, want


assert len(PER_MATE) == 43 and len(PAIR_LEVEL) == 9
