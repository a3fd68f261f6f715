"""Inputs for the tests of pairs whose mates differ in length, and of mixed-length batches (BBMap profile).

Real paired input is rarely equal-length after adapter and quality trimming, and processReadPair carries len1 and len2 apart
(BBMapThread.java:948, :983-986, :998-999, :1027-1053, :1085-1092; rescue(anchor, loose, ...), AbstractMapThread.java:1144-1243).
trimmed_pairs draws pairs at DRAW_LEN bases and cuts every mate to the length its class prescribes; mixed_single does the same
for single-ended reads.  Keys come from bbmap_amd.keys.make_batch (make_records), so every read has the key count of its own
length: with k = 12 a 12-base mate has one key, an 11- or 9-base mate none (quickMap's `L < k` return,
AbstractMapThread.java:646); a mate of 10 bases or more may still be rescued, a shorter one never (quickRescue).

coverage() counts, from any per-read site lists and the reads of the rescue fills, what the tests need to have happened -- the
oracle's output and the device's go through the same function."""
import numpy as np

from bbmap_amd import workload as W

K_TEST = 12
# (len1, len2).  (150,150): control.  (150,100) / (100,150): both rescue directions with anchor != loose.  (150,36) / (40,150):
# maxReadLen and outerDistLimit dominated by one mate, maxMismatches = 0.60 L - 1 below maxRescueMismatches, a loose mate with
# 2-3 keys.  (151,149): an off-by-one.  (64,65) / (128,127): the 64-lane strides of the revcomp, key and rescue kernels.
# (150,12): one key.  (150,11): no key, rescue may find it.  (9,150): no key and never rescued.
CLASSES = ((150, 150), (150, 100), (100, 150), (150, 36), (40, 150), (151, 149), (64, 65), (128, 127), (150, 12), (150, 11), (9, 150))
SUB_K = ((150, 12), (150, 11), (9, 150))
DRAW_LEN = 151                  # the pairs are drawn at the longest length any class asks for, then cut
# One pair in eight is a chimera: its mate 2 is the mate 2 of the pair STRAY_STEP further on, from somewhere else on the reference.
# Without them nearly every top site ends up paired (rescue finds a mate the probe missed: 1 unpaired top site in 1,200), and what
# the stages do with a list that stays unpaired -- scans that find nothing, the unpaired branch of the final stage -- would not run
# in most classes.  One chimera in two is cut at the 5' end.
STRAY_TURNS, STRAY_STEP = (2, 7), 37
MIXED_LENS = (12, 13, 14, 35, 63, 64, 65, 100, 127, 128, 129, 150, 151, 250, 300)


def _cut(read, length, five_prime):
    """read[:length]: a cut at the stored read's 3' end, what a quality trimmer does; five_prime: the other end"""
    return read[len(read) - length:].copy() if five_prime else read[:length].copy()


def trimmed_pairs(ref, n_pairs, seed, classes=CLASSES, pad=2000):
    """Pair p is of class classes[p % len(classes)] (a class named twice gets twice the pairs); within a class every fourth pair is
    cut at the 5' end, the others at the 3' end.  Returns (reads: list of uint8 arrays, mates interleaved; cls: the class of every
    pair; truth: dict start / strand / len per READ, start = leftmost reference coordinate of the mate's alignment after the cut).
    A 3' cut moves a minus-strand mate's leftmost coordinate by DRAW_LEN - len (its stored bases are the reverse complement), a 5'
    cut a plus-strand mate's."""
    raw, t = W.make_pairs(ref, n_pairs, read_len=DRAW_LEN, seed=seed, pad=pad, hard_frac=0.08)
    raw = raw.reshape(2 * n_pairs, DRAW_LEN)
    reads, cls = [], []
    start, strand, lens = np.zeros(2 * n_pairs, np.int64), np.zeros(2 * n_pairs, np.int32), np.zeros(2 * n_pairs, np.int32)
    for p in range(n_pairs):
        c = classes[p % len(classes)]
        turn = p // len(classes)
        five = turn % 4 == 3
        cls.append(tuple(c))
        for w in (0, 1):
            q = (p + STRAY_STEP) % n_pairs if (w == 1 and turn % 16 in STRAY_TURNS) else p         # a stray mate 2
            r, ln = 2 * p + w, int(c[w])
            st, a = int(t["strand%d" % (w + 1)][q]), int(t["start%d" % (w + 1)][q])
            reads.append(_cut(raw[2 * q + w], ln, five))
            if (st == 1) != five:
                a += DRAW_LEN - ln
            start[r], strand[r], lens[r] = a, st, ln
    return reads, cls, dict(start=start, strand=strand, len=lens)


def mixed_single(ref, n, seed, pad=2000):
    """Single-ended reads (all from the plus strand) with lengths MIXED_LENS in turn, drawn at the longest and cut as in
    trimmed_pairs.  Returns (reads list, truth dict start / len per read)."""
    top = max(MIXED_LENS)
    raw, _, t = W.make_reads_and_jobs(ref, n, read_len=top, seed=seed, pad=pad, long_del_frac=0.3, hard_frac=0.05)
    raw = raw.reshape(n, top)
    reads, start, lens = [], np.zeros(n, np.int64), np.zeros(n, np.int32)
    for i in range(n):
        ln = MIXED_LENS[i % len(MIXED_LENS)]
        five = (i // len(MIXED_LENS)) % 4 == 3
        reads.append(_cut(raw[i], ln, five))
        start[i], lens[i] = int(t["start"][i]) + (top - ln if five else 0), ln
    return reads, dict(start=start, len=lens)


def make_records(reads, k=K_TEST):
    """(recs, blob, baseScores, keyinfo) of the reads, keys placed by the product's key stage for quality-less input"""
    from bbmap_amd import keys as K
    return K.make_batch(reads, None, K.default_config(0, k=k))


def oracle_lists(orc):
    """per-read site lists of an oracle.map_reads result"""
    return [orc["sites"][r, :max(0, int(orc["nsites"][r]))] for r in range(len(orc["nsites"]))]


def oracle_rescue_reads(orc):
    """the read of every slowRescue fill (kind 2: the loose mate)"""
    return orc["log"]["read"][orc["log"]["kind"] == 2].tolist()


def device_rescue_reads(out):
    """the same from a Mapper.fetch() result, the overflow tier's logs in place of the reads it mapped"""
    from tests.mapper_check import gpu_fills
    tier = out.get("overflow")
    moved = set() if tier is None else {int(r) for r in tier["read_ids"] if int(out["nsites"][int(r)]) == -3}
    reads = [r for (r, _), v in gpu_fills(out).items() if v["kind"] == 2 and r not in moved]
    if tier is not None:
        reads += [int(tier["read_ids"][i]) for (i, _), v in gpu_fills(tier).items() if v["kind"] == 2 and int(tier["read_ids"][i]) in moved]
    return reads


def coverage(lists, rescue_reads, lens, cls):
    """What happened in a paired run.  lists: one site list per read (structured arrays with MSITE_DTYPE's fields); rescue_reads: the
    loose mate of every rescue fill; lens: per read; cls: per pair.  Returns a dict:
      fills_anchor_longer / fills_anchor_shorter / fills_equal: rescue fills by len(anchor) against len(loose),
      rescued_anchor_longer / rescued_anchor_shorter / rescued_equal: rescued sites in the lists, the same way,
      per class: pairs, mapped (reads with a site), paired / unpaired (top sites with pairedScore > 0 / == 0), rescued (reads whose
      list holds a rescued site), short_rescued / short_sites (the same two counts over the class's shorter mate alone)."""
    which = lambda a, l: "anchor_longer" if a > l else ("anchor_shorter" if a < l else "equal")
    cov = {"%s_%s" % (x, y): 0 for x in ("fills", "rescued") for y in ("anchor_longer", "anchor_shorter", "equal")}
    for r in rescue_reads:
        cov["fills_" + which(int(lens[r ^ 1]), int(lens[r]))] += 1
    per = {}
    for p, c in enumerate(cls):
        d = per.setdefault(c, dict(pairs=0, mapped=0, paired=0, unpaired=0, rescued=0, short_rescued=0, short_sites=0))
        d["pairs"] += 1
        short = 0 if c[0] < c[1] else 1
        for w in (0, 1):
            r = 2 * p + w
            s = lists[r]
            nres = int(np.count_nonzero(s["rescued"])) if len(s) else 0
            cov["rescued_" + which(int(lens[r ^ 1]), int(lens[r]))] += nres
            d["mapped"] += len(s) > 0
            d["rescued"] += nres > 0
            if len(s):
                d["paired" if int(s[0]["pairedScore"]) > 0 else "unpaired"] += 1
            if w == short and c[0] != c[1]:
                d["short_rescued"] += nres > 0
                d["short_sites"] += len(s)
    cov["classes"] = per
    return cov


def check_coverage(cov):
    """The conditions a run over CLASSES has to meet, on the oracle's output and on the device's alike; returns the list of those it
    misses (empty = all met)."""
    bad = []
    if cov["fills_anchor_longer"] < 20:
        bad.append("rescue fills with len(anchor) > len(loose): %d < 20" % cov["fills_anchor_longer"])
    if cov["fills_anchor_shorter"] < 20:
        bad.append("rescue fills with len(anchor) < len(loose): %d < 20" % cov["fills_anchor_shorter"])
    per = cov["classes"]
    for c in ((150, 11), (150, 12)):
        if per[c]["short_rescued"] < 1:
            bad.append("no short mate of class %r was rescued" % (c,))
    if per[(9, 150)]["short_sites"] != 0:
        bad.append("a 9-base mate has a site")
    for c, d in per.items():
        if c != (9, 150) and not (d["paired"] > 0 and d["unpaired"] > 0):
            bad.append("class %r: %d top sites with pairedScore > 0, %d with 0" % (c, d["paired"], d["unpaired"]))
    return bad


# ---------------------------------------------------------------------------------------------- the batch the tests share
# Every class once, and the five classes in which a LONGER mate gets rescued from a shorter anchor often enough once more: at 600
# pairs over CLASSES alone the oracle fills 7 such rescues, fewer than the 20 the tests ask for (see tests/test_oracle_pairs.py).
TEST_CLASSES = CLASSES + ((100, 150), (150, 100), (128, 127), (151, 149), (64, 65))
N_PAIRS = 1760                  # 110 pairs of a class named once, 220 of one named twice
_cache = {}


def reference():
    if "ref" not in _cache:
        _cache["ref"] = W.make_reference(300000, seed=6, pad=2000, repeat_frac=0.15)
    return _cache["ref"]


def oracle_index(ref):
    from oracle import oracle as O
    oi = O.OracleIndex([ref], k=K_TEST)
    oi.s.p.quitAfterTwoPerfects = 0             # as BBMap sets it for paired input (BBMap.java:434)
    return oi


def oracle_map(ref, recs, blob, bs, ki, paired, cap=64, **params):
    from oracle import oracle as O
    oi = oracle_index(ref)
    if not paired:
        oi.s.p.quitAfterTwoPerfects = 1
    return O.map_reads(oi, recs, blob, ki, base_scores=bs, paired=paired, cap=cap, threads=8, match_stride=4200,
                       params=O.map_default_params(**params) if params else None)


def pair_batch():
    """The trimmed pairs every test of unequal mates maps, made once: dict ref, reads, cls, truth, records (recs, blob, bs, ki)."""
    if "pairs" not in _cache:
        ref = reference()
        reads, cls, truth = trimmed_pairs(ref, N_PAIRS, seed=4, classes=TEST_CLASSES)
        _cache["pairs"] = dict(ref=ref, reads=reads, cls=cls, truth=truth, records=make_records(reads))
    return _cache["pairs"]


def pair_oracle():
    """oracle.map_reads over pair_batch(), run once; nobody writes to it"""
    if "pairs_oracle" not in _cache:
        b = pair_batch()
        _cache["pairs_oracle"] = oracle_map(b["ref"], *b["records"], paired=True)
    return _cache["pairs_oracle"]


def equal_batch(n_pairs=600):
    """An all-150 batch on the same reference, laid out as records: (reads uint8[2 n, 150], records)"""
    key = ("equal", n_pairs)
    if key not in _cache:
        reads, _ = W.make_pairs(reference(), n_pairs, read_len=150, seed=4, pad=2000, hard_frac=0.08)
        reads = reads.reshape(-1, 150)
        _cache[key] = (reads, make_records(list(reads)))
    return _cache[key]


def truth_shares(lists, truth, cls):
    """class -> share of its reads whose top site lies within 40 bases of the truth, on the right strand"""
    ok, tot = {}, {}
    for p, c in enumerate(cls):
        for r in (2 * p, 2 * p + 1):
            s = lists[r]
            tot[c] = tot.get(c, 0) + 1
            ok[c] = ok.get(c, 0) + int(len(s) > 0 and abs(int(s[0]["start"]) - int(truth["start"][r])) <= 40
                                       and int(s[0]["strand"]) == int(truth["strand"][r]))
    return {c: ok[c] / tot[c] for c in tot}
