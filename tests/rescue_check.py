"""A sequential tracer of the rescue scan: AbstractMapThread.quickRescue and SiteScore.setPerfect restated in plain Python from
the Java, one start after the other, plus a record of which branches a job took in the device kernel's geometry (64 consecutive
starts per block in search order, 64 bases per setPerfect chunk).  It shares no code with oracle/rescue_oracle.c or the kernel.

Java's inner loop walks the read base by base until the mismatch count passes minMismatches.  trace_quick_rescue() gets each
start's mismatch positions from one numpy comparison and walks those instead; quick_rescue_literal() is the base-by-base form,
kept to pin that shortcut."""
import numpy as np

INT_MAX = 2 ** 31 - 1
BLOCK = 64              # starts the kernel scores at once
CHUNK = 64              # bases per ballot of the kernel's setPerfect
_N = ord("N")


def _absdif(a, b):
    return a - b if a > b else b - a


def set_perfect(bases, ref, start, stop):
    """SiteScore.setPerfect(bases).  Returns (perfect, semiperfect, exit_chunk, n_over_limit): exit_chunk is the 64-base chunk
    of the read position at which the loop returned early (-1: it ran to the end), n_over_limit whether that return was the
    reference-N count passing len / 2."""
    if len(bases) != stop - start + 1:
        return 0, 0, -1, False
    perfect = semiperfect = True
    refloc, readloc, N = start, 0, 0
    mx, nlimit = min(stop, len(ref) - 1), len(bases) // 2
    if start < 0:
        N -= start
        readloc -= start
        refloc -= start
        perfect = False
    if stop >= len(ref):
        N += stop - len(ref) + 1
        perfect = False
    if N > nlimit:
        return 0, 0, -1, True
    first = readloc
    while refloc <= mx:
        c, r = bases[readloc], ref[refloc]
        if c != r or c == _N:
            perfect = False
            if c == _N:
                semiperfect = False
            if r != _N:
                return 0, 0, (readloc - first) // CHUNK, False
            N += 1
            if N > nlimit:
                return 0, 0, (readloc - first) // CHUNK, True
        refloc += 1
        readloc += 1
    semiperfect = semiperfect and N <= nlimit
    perfect = perfect and semiperfect and N == 0
    return int(perfect), int(semiperfect), -1, False


def _bounds(blen, reflen, minIndex, loc, searchDist, searchRight):
    if searchRight:
        return max(minIndex, loc), min(reflen - blen, loc + searchDist)
    return max(minIndex, loc - searchDist), min(reflen - blen, loc)


def _result(bases, ref, bestStart, minMismatches, maxContigMatches, pointsMatch, pointsMatch2, useAffine, baseHitScore):
    blen = len(bases)
    if useAffine:
        scoreOut = pointsMatch + pointsMatch2 * (blen - 1 - minMismatches)
    else:
        scoreOut = maxContigMatches + baseHitScore * (blen - minMismatches)
    p, sp, chunk, over = set_perfect(bases, ref, bestStart, bestStart + blen - 1)
    return dict(start=bestStart, stop=bestStart + blen - 1, score=scoreOut, mismatches=minMismatches, perfect=p, semiperfect=sp,
                contig=maxContigMatches), chunk, over


def quick_rescue_literal(bases, ref, minIndex, loc, searchDist, searchRight, idealStart, maxAllowedMismatches,
                         pointsMatch=70, pointsMatch2=100, useAffine=True, baseHitScore=100):
    """quickRescue base by base, exactly as the Java loops read.  Slow; no record."""
    blen = len(bases)
    if blen < 10:
        return None
    lowerBound, upperBound = _bounds(blen, len(ref), minIndex, loc, searchDist, searchRight)
    minMismatches = maxAllowedMismatches + 1
    maxContigMatches, bestScore, bestStart, bestAbsdif = 0, 0, -1, INT_MAX
    start = lowerBound if searchRight else upperBound
    while start <= upperBound if searchRight else start >= lowerBound:
        mismatches = contig = currentContig = 0
        j = 0
        while j < blen and mismatches <= minMismatches:
            c, r = bases[j], ref[start + j]
            if c != r or c == _N:
                mismatches += 1
                contig = max(contig, currentContig)
                currentContig = 0
            else:
                currentContig += 1
            j += 1
        score = (blen - mismatches) + contig
        absdif = _absdif(start, idealStart)
        if mismatches <= minMismatches and (score > bestScore or (score == bestScore and absdif < bestAbsdif)):
            bestStart, minMismatches, maxContigMatches, bestScore, bestAbsdif = start, mismatches, contig, score, absdif
            if mismatches == 0:
                if searchRight:
                    upperBound = min(upperBound, idealStart + absdif)
                else:
                    lowerBound = max(lowerBound, idealStart - absdif)
        start += 1 if searchRight else -1
    if bestStart < 0:
        return None
    return _result(bases, ref, bestStart, minMismatches, maxContigMatches, pointsMatch, pointsMatch2, useAffine, baseHitScore)[0]


def new_record(blen):
    return dict(narrow=0, narrow_in_block=0, narrow_stops_later_block=0, stale_cap=0, improve=0, tie_win=0, tie_lose=0,
                tie_equal_absdif=0, tail_bytes=blen % 4, sp_exit_chunk=-1, sp_n_over_limit=False,
                clip_low=False, clip_high=False, starts=0, first_accept=-1)


def trace_quick_rescue(bases, ref, minIndex, loc, searchDist, searchRight, idealStart, maxAllowedMismatches,
                       pointsMatch=70, pointsMatch2=100, useAffine=True, baseHitScore=100):
    """Returns (result, record): result is what oracle.oracle.quick_rescue returns (None or a dict), record counts the branches.
    The counters count starts (events), except narrow_stops_later_block, which is 0 or 1 for the job."""
    bases, ref = bytes(bases), bytes(ref)
    blen = len(bases)
    rec = new_record(blen)
    if blen < 10:
        return None, rec
    lowerBound, upperBound = _bounds(blen, len(ref), minIndex, loc, searchDist, searchRight)
    if searchRight:
        rec["clip_low"], rec["clip_high"] = minIndex > loc, len(ref) - blen < loc + searchDist
    else:
        rec["clip_low"], rec["clip_high"] = minIndex > loc - searchDist, len(ref) - blen < loc
    if lowerBound > upperBound:
        return None, rec
    lower0, upper0 = lowerBound, upperBound
    rd = np.frombuffer(bases, np.uint8)
    window = np.frombuffer(ref, np.uint8)[lower0:upper0 + blen]
    bad = (np.lib.stride_tricks.sliding_window_view(window, blen) != rd) | (rd == _N)      # [start - lower0, j]: Java's test
    full = bad.sum(axis=1).tolist()
    minMismatches = maxAllowedMismatches + 1
    maxContigMatches, bestScore, bestStart, bestAbsdif = 0, 0, -1, INT_MAX
    first = lower0 if searchRight else upper0
    step = 1 if searchRight else -1
    k, capBlock, narrowBlock = 0, minMismatches, -1
    while True:
        start = first + step * k
        if start > upperBound if searchRight else start < lowerBound:
            break
        if k % BLOCK == 0:
            capBlock = minMismatches
        fullMM = full[start - lower0]
        if minMismatches < fullMM <= capBlock:
            rec["stale_cap"] += 1
        if fullMM <= minMismatches:                       # the loop runs to the end of the read
            mismatches, contig, prev = 0, 0, -1
            for p in np.flatnonzero(bad[start - lower0]).tolist():
                mismatches += 1
                contig = max(contig, p - prev - 1)
                prev = p
            score = (blen - mismatches) + contig
            absdif = _absdif(start, idealStart)
            if bestStart >= 0 and score == bestScore:
                rec["tie_win" if absdif < bestAbsdif else "tie_lose" if absdif > bestAbsdif else "tie_equal_absdif"] += 1
            if score > bestScore or (score == bestScore and absdif < bestAbsdif):
                if bestStart >= 0 and mismatches < minMismatches:
                    rec["improve"] += 1
                if bestStart < 0:
                    rec["first_accept"] = k
                bestStart, minMismatches, maxContigMatches, bestScore, bestAbsdif = start, mismatches, contig, score, absdif
                if mismatches == 0:
                    if searchRight:
                        new = min(upperBound, idealStart + absdif)
                        blockLast = min(upperBound, first + (k // BLOCK) * BLOCK + BLOCK - 1)
                        tightened, inBlock = new < upperBound, new < blockLast
                        upperBound = new
                    else:
                        new = max(lowerBound, idealStart - absdif)
                        blockLast = max(lowerBound, first - (k // BLOCK) * BLOCK - BLOCK + 1)
                        tightened, inBlock = new > lowerBound, new > blockLast
                        lowerBound = new
                    if tightened:
                        rec["narrow"] += 1
                        rec["narrow_in_block"] += inBlock
                        narrowBlock = k // BLOCK
        # else: Java's loop stopped at mismatches == minMismatches + 1 and the start is rejected
        k += 1
    rec["starts"] = k
    if narrowBlock >= 0 and (k - 1) // BLOCK > narrowBlock:
        rec["narrow_stops_later_block"] = 1
    if bestStart < 0:
        return None, rec
    res, rec["sp_exit_chunk"], rec["sp_n_over_limit"] = _result(bases, ref, bestStart, minMismatches, maxContigMatches,
                                                              pointsMatch, pointsMatch2, useAffine, baseHitScore)
    return res, rec


def first_divergence(bases, ref, minIndex, loc, searchDist, searchRight, idealStart, maxAllowedMismatches, got):
    """For a failure message: the tracer's result and record, and how the start in `got` (a result dict or None) compares."""
    res, rec = trace_quick_rescue(bases, ref, minIndex, loc, searchDist, searchRight, idealStart, maxAllowedMismatches)
    lo, hi = _bounds(len(bases), len(ref), minIndex, loc, searchDist, searchRight)
    msg = ["tracer result %r" % (res,), "tracer record %r" % (rec,), "window [%d, %d] searched %s" % (lo, hi, "right" if searchRight else "left")]
    for name, r in (("tracer", res), ("other", got)):
        if r is not None and lo <= r["start"] <= hi:
            st = r["start"]
            k = st - lo if searchRight else hi - st
            mm = sum(1 for j in range(len(bases)) if bases[j] != ref[st + j] or bases[j] == _N)
            msg.append("%s start %d: search position %d (block %d, lane %d), %d mismatches over the whole read, absdif %d"
                       % (name, st, k, k // BLOCK, k % BLOCK, mm, _absdif(st, idealStart)))
    return "\n".join(msg)
