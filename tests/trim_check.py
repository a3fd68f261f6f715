"""A sequential restatement of align2.TrimRead (current/align2/TrimRead.java) for the trim stage's tests: trim(Read, ...) :47-63 with
testOptimal :264-324, testRightWindow :349-365, testLeft / testRight :327-385, testLeftN / testRightN :388-413 and the constructor's
clamp trim(int, int, int) :164-197; and untrim() :415-463 / untrim(SiteScore) :465-508 over FINAL_DTYPE records, MSITE_DTYPE site
lists and their match strings.  Plain Python over one read at a time; the optimal mode's score is a numpy float32 scalar, so every
add rounds as Java's float does."""
import functools

import numpy as np

MODE_OPTIMAL, MODE_WINDOW, MODE_INTERVAL = 0, 1, 2
F = np.float32
# QualityTools.PROB_ERROR (current/align2/QualityTools.java:475-480): (float)Math.pow(10, 0 - .1 * i), [0] = .8f
PROB_ERROR = [F(10.0 ** (0 - .1 * i)) for i in range(128)]
PROB_ERROR[0] = F(.8)
NPROB = F(0.75)                                             # :564
N = ord("N")


class Config:
    """TrimRead's statics and the arguments of trim(): what bbtrim_config holds"""

    def __init__(self, mode=MODE_OPTIMAL, trimLeft=0, trimRight=0, trimq=6, minLength=60, windowLength=4, minGoodInterval=2, optimalBias=-1.0):
        self.mode, self.trimLeft, self.trimRight, self.trimq, self.minLength = mode, trimLeft, trimRight, trimq, minLength
        self.windowLength, self.minGoodInterval, self.optimalBias = windowLength, minGoodInterval, optimalBias

    @classmethod
    def of(cls, c):
        """from a bbmap_amd.trim.bbtrim_config"""
        return cls(c.mode, c.trimLeft, c.trimRight, c.trimq, c.minLength, c.windowLength, c.minGoodInterval, c.optimalBias)


def test_left_n(bases, min_good):                           # :388-399
    good, last_bad, i = 0, -1, 0
    while i < len(bases) and good < min_good:
        if bases[i] != N:
            good += 1
        else:
            good, last_bad = 0, i
        i += 1
    return last_bad + 1


def test_right_n(bases, min_good):                          # :402-413
    good, last_bad, i = 0, len(bases), len(bases) - 1
    while i >= 0 and good < min_good:
        if bases[i] != N:
            good += 1
        else:
            good, last_bad = 0, i
        i -= 1
    return len(bases) - last_bad


@functools.lru_cache(maxsize=None)
def _optimal_scan(bases, qual, avg):
    """the loop of testOptimal :270-316 (bytes, bytes, float32) -> (left, right)"""
    max_score, score = F(0), F(0)
    max_loc, max_count, count = -1, -1, 0
    nprob = max(min(F(avg * F(1.1)), F(1)), NPROB)          # :276
    for i in range(len(bases)):
        pe = nprob if bases[i] == N else PROB_ERROR[qual[i]]
        delta = F(avg - pe)
        score = F(score + delta)
        if score > 0:
            count += 1
            if score > max_score or (score == max_score and count > max_count):
                max_score, max_count, max_loc = score, count, i
        else:
            score, count = F(0), 0
    if max_score > 0:
        return max_loc - max_count + 1, len(bases) - max_loc - 1
    return 0, len(bases)


def test_optimal(bases, qual, trimq, bias, min_good):       # :264-324
    avg = PROB_ERROR[trimq]
    if bias >= 0:
        avg = F(bias)
    if len(bases) == 0:
        return 0, 0
    if qual is None:
        return (0, 0) if avg >= 1 else (test_left_n(bases, min_good), test_right_n(bases, min_good))
    return _optimal_scan(bytes(bases), bytes(qual), avg)


@functools.lru_cache(maxsize=None)
def test_right_window(bases, qual, trimq, window, min_good):        # :349-365 (bytes, bytes or None)
    if len(bases) == 0:
        return 0
    if qual is None or len(qual) < window:
        return 0 if trimq > 0 else test_right_n(bases, min_good)
    thresh = max(window * trimq, 1)
    total, j = 0, -window
    for i in range(len(qual)):
        total += int(qual[i])
        if j >= -1:
            if j >= 0:
                total -= int(qual[j])
            if total < thresh:
                return len(qual) - j - 1
        j += 1
    return 0


def test_left(bases, qual, trimq, min_good):                # :327-346
    if len(bases) == 0:
        return 0
    if qual is None:
        return 0 if trimq < 0 else test_left_n(bases, min_good)
    good, last_bad, i = 0, -1, 0
    while i < len(bases) and good < min_good:
        if qual[i] > trimq:
            good += 1
        else:
            good, last_bad = 0, i
        i += 1
    return last_bad + 1


def test_right(bases, qual, trimq, min_good):               # :368-385
    if len(bases) == 0:
        return 0
    if qual is None:
        return 0 if trimq < 0 else test_right_n(bases, min_good)
    good, last_bad, i = 0, len(bases), len(bases) - 1
    while i >= 0 and good < min_good:
        if qual[i] > trimq:
            good += 1
        else:
            good, last_bad = 0, i
        i -= 1
    return len(bases) - last_bad


def clamp(n, a, b, minlen):
    """the constructor :131-147 and trim(int, int, int) :164-197: (leftTrimmed, rightTrimmed) for a + b > 0"""
    minlen = max(minlen, 0)
    max_trim = min(n, n - minlen)
    if a + b > max_trim:
        excess = a + b - max_trim
        if a > 0 and excess > 0:
            a = max(0, a - excess)
            excess = a + b - max_trim
        if b > 0 and excess > 0:
            b = max(0, b - excess)
    return a, b


def trim(bases, qual, c):
    """TrimRead.trim(r, trimLeft, trimRight, trimq, minlen) :47-63 -> (left, right); (0, 0) where Java returns null"""
    bases = bytes(bases)
    qual = None if qual is None else bytes(qual)
    if c.mode == MODE_OPTIMAL:
        a, b = test_optimal(bases, qual, c.trimq, c.optimalBias, c.minGoodInterval)
        a, b = (a if c.trimLeft else 0), (b if c.trimRight else 0)
    elif c.mode == MODE_WINDOW:
        a, b = 0, (test_right_window(bases, qual, c.trimq, c.windowLength, c.minGoodInterval) if c.trimRight else 0)
    else:
        a = test_left(bases, qual, c.trimq, c.minGoodInterval) if c.trimLeft else 0
        b = test_right(bases, qual, c.trimq, c.minGoodInterval) if c.trimRight else 0
    if a + b == 0:
        return 0, 0
    return clamp(len(bases), a, b, c.minLength)


def _pad(match, lt, rt):                                    # :436-447 / :492-503
    return None if match is None else b"C" * lt + bytes(match) + b"C" * rt


def untrim(fin, matches, sites, nsites, site_matches, trims, ids=None):
    """TrimRead.untrim over one context's output.  fin: FINAL_DTYPE[n]; matches[i]: bytes or None; sites: MSITE_DTYPE[n, cap];
    nsites: int[n] (negative = no list); site_matches[i][s]: bytes or None for the sites of the list; trims: (left, right) per BATCH
    read; ids: record i is batch read ids[i] (the overflow tier), None = read i.  Returns new (fin, matches, sites, site_matches).
    The one declared difference from Java: an unmapped record keeps its start and stop."""
    fin, sites = fin.copy(), sites.copy()
    matches = list(matches)
    site_matches = [list(x) for x in site_matches]
    for i in range(len(fin)):
        left, right = (int(x) for x in trims[i if ids is None else int(ids[i])])
        if left == 0 and right == 0:                        # :416
            continue
        f = fin[i]
        f["perfect"] = 0                                    # :417
        lt, rt = (left, right) if int(f["strand"]) == 0 else (right, left)     # :420-426
        matches[i] = _pad(matches[i], lt, rt)
        f["match_len"] = len(matches[i]) if matches[i] is not None else f["match_len"]
        if int(f["mapped"]):
            f["start"] -= lt                                # :451-452
            f["stop"] += rt
        for s in range(max(0, int(nsites[i]))):             # :458-460, untrim(SiteScore) :465-508
            ss = sites[i][s]
            ss["perfect"] = ss["semiperfect"] = 0
            lt, rt = (left, right) if int(ss["strand"]) == 0 else (right, left)
            m = _pad(site_matches[i][s], lt, rt)
            site_matches[i][s] = m
            if m is not None:
                ss["reserved"][1] = len(m)
            ss["start"] -= lt                               # setLimits :505
            ss["stop"] += rt
    return fin, matches, sites, site_matches
