// What the three index-probe kernels share that is not a kernel's own schedule (index_probe.hip: one read per lane;
// index_probe_wave.hip: one read per wavefront; index_probe_long.hip: one read per wavefront, many keys, both profiles):
//   * the two class families' constants (ProfBBMap = BBIndex + MultiStateAligner11tsJNI, ProfPacBio = BBIndexPacBio +
//     MultiStateAligner9PacBio) and the small functions that depend on nothing else: calcApproxHitsCutoff, the gap scores of
//     calcAffineScore, adjustSite, overlap, Solver.valueOfElement;
//   * for the two wave-cooperative kernels, the code that sees the read only through its location array: calcAffineScore,
//     makeGapArray, SiteScore.setPerfect, and slowWalk3's site bookkeeping (walkBegin / recordSite / walkEnd; the long kernel
//     uses it, the wave kernel keeps a marked copy of recordSite over its own locals: DESIGN 7.7 has the measurement).  These are
//     templates over the kernel's own state structs (u: ix, c, blen, lane; S: base[2], bsc, gaps) and a location-array policy
//     LOC with ld(u, S, i), st(u, S, i, v) and ngaps(S): LocInts below, Loc16 in index_probe_long.hip.
// The heap stand-ins, pops, quick scores, extendScore, the greedy trim and the kernels themselves stay with each kernel; so do
// the debug hooks (phase timers, batch statistics): nothing in here carries one.
// It is a header of its own rather than part of index_common.h because the index build and the host contexts include that one
// and have no use for wave primitives or device-only templates.
#pragma once
#include "index_common.h"
#include "wave_prims.h"

namespace bbidx {

struct ProfBBMap {      // BBIndex.java:3168-3305 ; MultiStateAligner11tsJNI.java:871-1027, jni/MultiStateAligner11tsJNI.c:18-98
    static constexpr int Z_MULT = 20, SMALL_LIST = 20, MIN_LISTS_RETAIN = 6, INDEL_MULT = 20, PERFECT_RED = 0;
    static constexpr float HIT_FRACTION = 0.85f, MIN_SCORE_MULT = 0.15f, MIN_QSCORE_MULT = 0.025f, MIN_QSCORE_MULT2 = 0.1f, DYN_SCORE = 0.84f;
    static constexpr int RELAX1 = 4, RELAX2 = 3, RELAX3 = 3, RELAX4 = 2;
    __device__ static inline int indelPenalty(int bkhs) { return bkhs / 2 - 1; }
    static constexpr int MATCH = 70, MATCH2 = 100, SUB = -127, SUB2 = -51, SUB3 = -25;
    static constexpr int INS = -395, INS2 = -39, DEL = -472, DEL2 = -33, DEL3 = -9, DEL4 = -1, DEL5 = -1, GAP = -2;
    static constexpr int INS_DIF_PLUS = 0;              // POINTS_INS_ARRAY_C[min(loc - lastLoc, 5)]
};
struct ProfPacBio {     // BBIndexPacBio.java:2461-2596 ; MultiStateAligner9PacBio.java:2375-2407, :1681-1870
    static constexpr int Z_MULT = 25, SMALL_LIST = 80, MIN_LISTS_RETAIN = 12, INDEL_MULT = 25, PERFECT_RED = 2;
    static constexpr float HIT_FRACTION = 0.97f, MIN_SCORE_MULT = 0.02f, MIN_QSCORE_MULT = 0.005f, MIN_QSCORE_MULT2 = 0.005f, DYN_SCORE = 0.64f;
    static constexpr int RELAX1 = 20, RELAX2 = 18, RELAX3 = 16, RELAX4 = 14;
    __device__ static inline int indelPenalty(int bkhs) { return bkhs / 8 - 1; }
    static constexpr int MATCH = 90, MATCH2 = 100, SUB = -137, SUB2 = -49, SUB3 = -25;
    static constexpr int INS = -205, INS2 = -42, DEL = -292, DEL2 = -37, DEL3 = -17, DEL4 = -2, DEL5 = -1, GAP = -2;
    static constexpr int INS_DIF_PLUS = 1;              // dif = min(loc - lastLoc + 1, 5), :1729
};

// BBIndex.calcApproxHitsCutoff :3267-3294 (BBIndexPacBio.java:2562-2585)
template <class PF> __device__ __forceinline__ int calcApproxHitsCutoff(const bbidx_params &p, int keys, int hits, int currentCutoff, bool perfect) {
    const int reduction = min(max(hits / p.hitReductionDiv, p.maxHitsReduction2), max(p.maximumMaxHitsReduction, keys / 8));
    int r = max(p.minApproxHitsToKeep, max(currentCutoff, hits - reduction));
    if (perfect) r = max(r, keys - PF::PERFECT_RED);
    return r;
}

// calcAffineScore's helpers, in plain points
template <class PF> __device__ __forceinline__ int calcDelScoreApprox(int len) {      // calcDelScore(len, approximateGaps = true), MultiStateAligner11tsJNI.java:1347-1376
    if (len <= 0) return 0;
    int score = PF::DEL;
    if (len > MINGAP) { const int rem = len % 128, div = (len - 128) / 128; score += div * PF::GAP; len = rem + 128; }
    if (len > 80) { score += ((len - 80 + 3) / 4) * PF::DEL5; len = 80; }
    if (len > 20) { score += (len - 20) * PF::DEL4; len = 20; }
    if (len > 5) { score += (len - 5) * PF::DEL3; len = 5; }
    if (len > 1) score += (len - 1) * PF::DEL2;
    return score;
}
template <class PF> __device__ __forceinline__ int insCum(int n) { return PF::INS + (n > 1 ? (n - 1) * PF::INS2 : 0); }     // POINTS_INS_ARRAY_C[n], n in 1..5
template <class PF> __device__ __forceinline__ int subArr(int t) { return t > 5 ? PF::SUB3 : (t > 1 ? PF::SUB2 : PF::SUB); }   // POINTS_SUB_ARRAY[t]

__device__ __forceinline__ int adjustSite(const Codec &c, int a, int offset, int baseChrom) {
    // a site in the first `offset` bases of its chromosome maps to position 0 of that chromosome (branch-free: both forms
    // are a handful of ALU ops, and a per-lane branch here would sit in the innermost loop of the probe)
    const int below = c.toNumber(0, c.chromOf(a, baseChrom));
    return (a & c.siteMask) >= offset ? a - offset : below;
}
__device__ __forceinline__ bool overlap(int a1, int b1, int a2, int b2) { return a2 <= b1 && b2 >= a1; }

// Solver.valueOfElement (current/align2/Solver.java:97-151)
__device__ __forceinline__ long long valueOfElement(const int *offsets, int noffsets, const int *lengths, float keyWeight, int chunk,
                                                    const int *lists, int numlists, int index, long long pointsPerSite) {
    const long long PPL = 30000, PPB1 = 6000, BONUS_END = 40000, WIDTH = 5500, SPACING = -30;
    if (numlists < 1) return 0;
    const int prospect = lists[index];
    if (lengths[prospect] == 0) return -999999;
    long long valuep = PPL + (PPL * 2 / numlists) + ((PPL * 10) / lengths[prospect]);
    const long long valuem = pointsPerSite * lengths[prospect];
    if (prospect == 0 || prospect == noffsets - 1) valuep += BONUS_END;
    if (numlists == 1) { valuep += (WIDTH + PPB1) * chunk; return ((long long)__fmul_rn((float)valuep, keyWeight)) + valuem; }
    const int first = lists[0], last = lists[numlists - 1];
    const int offL = (prospect == first ? -1 : offsets[lists[index - 1]]);
    const int offP = offsets[prospect];
    const int offR = (prospect == last ? offsets[noffsets - 1] + 1 : offsets[lists[index + 1]]);
    const int oldL = offP - offL, oldR = offR - offP, newS = offR - offL;
    valuep += (long long)((oldL * oldL + oldR * oldR) - (newS * newS)) * SPACING;
    int uniquelyCovered;
    if (prospect == first) uniquelyCovered = offR - offP;
    else if (prospect == last) uniquelyCovered = offP - offL;
    else { const int b = offR - (offL + chunk); uniquelyCovered = b > 0 ? b : 0; }
    if (prospect == first || prospect == last) valuep += (PPB1 + WIDTH) * uniquelyCovered;
    else valuep += PPB1 * uniquelyCovered;
    return ((long long)__fmul_rn((float)valuep, keyWeight)) + valuem;
}

// ------------------------------------------------------------------------------- one read per wavefront: the location array
using namespace wavep;

// the location array as plain ints with the gap count next to it (index_probe_wave.hip's WaveLds)
struct LocInts {
    template <class UT, class ST> __device__ static __forceinline__ int ld(const UT &, const ST &S, int i) { return S.loc[i]; }
    template <class UT, class ST> __device__ static __forceinline__ void st(const UT &, ST &S, int i, int v) { S.loc[i] = v; }
    template <class ST> __device__ static __forceinline__ int &ngaps(ST &S) { return S.ngaps; }
};

// MultiStateAligner11tsJNI.calcAffineScore(locArray, baseScores, bases, minContig) :871-1027 (MultiStateAligner9PacBio.java:1681-1870)
// over the LDS location array, 64 bases per step.  Sequential state of the reference and how it is recovered:
//   lastValue  = the previous element                       -> loc[p-1]
//   lastLoc    = the last positive element before p         -> highest set bit of the "positive" ballot below p
//   timeInMode = length of the run of -1 ending at p        -> distance to the highest "not -1" bit below p
//   contig     = equal-to-previous streak                   -> popcount of "equal" events since the last reset event
template <class PF, class LOC, class UT, class ST> __device__ __forceinline__ int calcAffineScore(const UT &u, const ST &S, int strand, int minContig) {
    const int blen = u.blen, lane = u.lane;
    int score = 0, carryLastLoc = -3, carryRun = 0, carryContig = 0, maxContig = 0;
    for (int base = 0; base < blen; base += 64) {
        const int p = base + lane;
        const bool valid = p < blen;
        const int loc = valid ? LOC::ld(u, S, p) : 0;
        const int prev = (valid && p > 0) ? LOC::ld(u, S, p - 1) : -1;
        const bool pos = valid && loc > 0, neg1 = valid && loc == -1;
        const u64 posM = __ballot(pos), n1M = __ballot(neg1);
        const u64 lt = lt_mask(lane);
        const u64 mlo = posM & lt;
        const int lastLoc = mlo ? LOC::ld(u, S, base + hibit(mlo)) : carryLastLoc;
        int c = 0, ev = 0;                                   // ev: 1 equal, 2 restart, 3 indel
        if (pos) {
            const int bs = S.bsc[strand ? blen - 1 - p : p];
            if (loc == prev) { c = PF::MATCH2 + bs; ev = 1; }
            else if (loc == lastLoc || lastLoc < 0) { c = PF::MATCH + bs; ev = 2; }
            else if (loc < lastLoc) { c = PF::MATCH + bs + calcDelScoreApprox<PF>(lastLoc - loc + 1); ev = 3; }
            else { c = PF::MATCH + bs + insCum<PF>(min(loc - lastLoc + PF::INS_DIF_PLUS, 5)); ev = 3; }
        } else if (neg1) {
            const u64 nb = ~n1M & lt;
            const int t = nb ? lane - hibit(nb) : lane + 1 + carryRun;
            c = subArr<PF>(t);
        }
        score += wsum(c);
        if (minContig > 1) {
            const u64 EM = __ballot(ev == 1), SM = __ballot(ev == 2), IM = __ballot(ev == 3), RM = SM | IM;
            int cval = 0;
            if (ev == 1) {
                const u64 rlo = RM & lt;
                if (rlo) { const int r = hibit(rlo); cval = popc(EM & lt & gt_mask(r)) + 1 + (int)((SM >> r) & 1); }
                else cval = popc(EM & lt) + 1 + carryContig;
            } else if (ev == 2) cval = 1;
            maxContig = max(maxContig, wmax(cval));
            const u64 all = EM | RM;
            if (all) carryContig = rl(cval, hibit(all));
        }
        if (posM) carryLastLoc = rl(loc, hibit(posM));
        const int last = min(63, blen - 1 - base);
        if ((n1M >> last) & 1) {
            const u64 nbAll = ~n1M & (lt_mask(last) | (1ull << last));
            carryRun = nbAll ? last - hibit(nbAll) : last + 1 + carryRun;
        } else carryRun = 0;
    }
    if (minContig > 1 && maxContig < minContig) score = min(score, -50 * blen);
    return score;
}

// BBIndex.makeGapArray :2837-2878 -- rare (a site spanning more than MINGAP + read length); one lane walks LDS
// (the array is rewritten in place as the reference does; with Loc16, positions plus base indices still fit the 16-bit offsets)
template <class LOC, class UT, class ST> __device__ __forceinline__ int makeGapArray(const UT &u, ST &S, int minLoc, int minGap) {
    if (u.lane == 0) {
        auto LA = [&](int i) -> int { return LOC::ld(u, S, i); };
        auto SET = [&](int i, int v) { LOC::st(u, S, i, v); };
        const int n = u.blen;
        int gaps = 0; bool doSort = false;
        if (LA(0) < 0) SET(0, minLoc);
        for (int i = 1; i < n; i++) {
            if (LA(i) < 0) SET(i, LA(i - 1) + 1); else SET(i, LA(i) + i);
            if (LA(i) < LA(i - 1)) doSort = true;
        }
        if (doSort) {
            for (int i = 1; i < n; i++) { const int v = LA(i); int j = i - 1; while (j >= 0 && LA(j) > v) { SET(j + 1, LA(j)); j--; } SET(j + 1, v); }
        }
        for (int i = 1; i < n; i++) if (LA(i) - LA(i - 1) > minGap) gaps++;
        int len = 0;
        if (gaps >= 1) {
            len = 2 + gaps * 2;
            if (len > BBIDX_MAX_GAPS) len = -1;
            else {
                S.gaps[0] = LA(0); S.gaps[len - 1] = LA(n - 1);
                for (int i = 1, j = 1; i < n; i++) if (LA(i) - LA(i - 1) > minGap) { S.gaps[j] = LA(i - 1); S.gaps[j + 1] = LA(i); j += 2; }
            }
        }
        LOC::ngaps(S) = len;
    }
    wsync();
    return __builtin_amdgcn_readfirstlane(LOC::ngaps(S));
}

// SiteScore.setPerfect (current/stream/SiteScore.java:239-292): order-independent form
template <class UT, class ST> __device__ __forceinline__ void setPerfect(const UT &u, const ST &S, int chrom, int strand, int start, int stop, int &perfectOut, int &semiOut) {
    const int blen = u.blen;
    perfectOut = 0; semiOut = 0;
    if (blen != stop - start + 1) return;
    const uint8_t *ref = u.ix->chromArr[chrom];
    const int reflen = u.ix->chromArrLen[chrom];
    const uint8_t *rb = S.base[strand];
    bool perfect = true;
    int refloc = start, readloc = 0, N = 0;
    const int mx = min(stop, reflen - 1), nlimit = blen / 2;
    if (start < 0) { N -= start; readloc -= start; refloc -= start; perfect = false; }
    if (stop >= reflen) { N += (stop - reflen + 1); perfect = false; }
    if (N > nlimit) return;
    bool anyHard = false, anyCN = false, anyBad = false;
    const int total = uni(mx - refloc + 1);                 // bases compared; lanes past the end re-read the last one
    for (int j0 = 0; j0 < total; j0 += 64) {
        const bool in = j0 + u.lane < total;
        const int j = in ? j0 + u.lane : total - 1;
        const int c = rb[readloc + j], r = ref[refloc + j];
        const bool bad = in && (c != r || c == 'N'), hard = bad && r != 'N', cn = bad && c == 'N';
        const u64 badM = __ballot(bad);
        if (badM) {
            anyBad = true;
            if (__ballot(hard)) { anyHard = true; break; }
            if (__ballot(cn)) anyCN = true;
            N += popc(badM);
            if (N > nlimit) break;
        }
    }
    if (anyHard || N > nlimit) return;
    const bool semi = !anyCN;
    semiOut = semi ? 1 : 0;
    perfectOut = (perfect && !anyBad && semi && N == 0) ? 1 : 0;
}

// ------------------------------------------------------------------------------- one read per wavefront: slowWalk3's bookkeeping
struct SiteOut { bbidx_site *v; int n, cap; bool overflow; };
struct PrevSite { int idx, chrom, strand, start, stop, score, perfect, semiperfect, ngaps; };

// the mutable state of one slowWalk3 call (BBIndex.slowWalk3 :1219-1706), all of it wave-uniform
struct WalkState {
    SiteOut &ssl;
    int approxHitsCutoff, cutoff, qcutoff, currentTopScore, maxHits, perfectsFound, bestqscore;
    bool finished;
    PrevSite pv;
    // loop-carried uniform state is re-declared uniform at the top of every round (see wavep::uni)
    __device__ __forceinline__ void reuni() {
        approxHitsCutoff = uni(approxHitsCutoff); cutoff = uni(cutoff); qcutoff = uni(qcutoff); currentTopScore = uni(currentTopScore);
        maxHits = uni(maxHits); perfectsFound = uni(perfectsFound); bestqscore = uni(bestqscore);
        pv.idx = uni(pv.idx); pv.chrom = uni(pv.chrom); pv.strand = uni(pv.strand); pv.start = uni(pv.start); pv.stop = uni(pv.stop);
        pv.score = uni(pv.score); pv.perfect = uni(pv.perfect); pv.semiperfect = uni(pv.semiperfect); pv.ngaps = uni(pv.ngaps);
        ssl.n = uni(ssl.n); ssl.overflow = uni(ssl.overflow); finished = uni(finished);
    }
};

// The state at the start of a walk, from the read's bestScores[] (:1240-1262); false when the walk has nothing to do.
template <class PF> __device__ __forceinline__ bool walkBegin(WalkState &w, const bbidx_params &p, const int *bestScores, int numKeys, int numHits, int mqs, int maxScore) {
    const int minScore = (int)(PF::MIN_SCORE_MULT * maxScore);
    const int minQuickScore = (int)(PF::MIN_QSCORE_MULT * mqs);
    w.currentTopScore = bestScores[0];
    w.cutoff = max(minScore, (int)(w.currentTopScore * PF::DYN_SCORE));
    w.qcutoff = max(bestScores[2], minQuickScore);
    w.bestqscore = bestScores[3]; w.maxHits = bestScores[1]; w.perfectsFound = bestScores[5];
    w.approxHitsCutoff = calcApproxHitsCutoff<PF>(p, numKeys, w.maxHits, p.minApproxHitsToKeep, w.currentTopScore >= maxScore);
    if (w.approxHitsCutoff > numHits) return false;
    if (w.currentTopScore >= maxScore) w.qcutoff = max(w.qcutoff, (int)(mqs * DYN_QSCORE_PERFECT));
    w.pv.idx = -1; w.pv.chrom = w.pv.strand = w.pv.start = w.pv.stop = w.pv.score = w.pv.perfect = w.pv.semiperfect = w.pv.ngaps = 0;
    w.finished = false;
    return true;
}
// ... and back into bestScores[] at its end (:1693-1704)
__device__ __forceinline__ void walkEnd(const WalkState &w, int *bestScores, int mqs) {
    bestScores[0] = max(bestScores[0], w.currentTopScore);
    bestScores[1] = max(bestScores[1], w.maxHits);
    bestScores[2] = max(bestScores[2], w.qcutoff);
    bestScores[3] = max(bestScores[3], w.bestqscore);
    bestScores[4] = mqs;
    bestScores[5] = w.perfectsFound;
}

// A site has scored (:1478-1632): raises the cutoffs, then merges the site into the previous one (same limits; extension at the
// same start or at the same stop) or appends it to the list.  mapStart / mapStop are the lowest and highest diagonal as site
// numbers; locArrayValid says that the location array holds this site's extension (a gap array can be made from it).
template <class PF, class LOC, class UT, class ST>
__device__ __forceinline__ void recordSite(const UT &u, ST &S, WalkState &w, int numKeys, int baseChrom, int strand, int approxHits, int score,
                                           int mapStart, int mapStop, bool locArrayValid, int maxScore, bool fullyDefined) {
    if (score < w.cutoff) return;
    const bbidx_params &p = u.ix->p;
    const int blen = u.blen, lane = u.lane;
    SiteOut &ssl = w.ssl;
    PrevSite &pv = w.pv;
    if (score > w.currentTopScore) {
        w.maxHits = max(approxHits, w.maxHits);
        w.approxHitsCutoff = calcApproxHitsCutoff<PF>(p, numKeys, w.maxHits, w.approxHitsCutoff, w.currentTopScore >= maxScore);
        w.cutoff = max(w.cutoff, (int)(score * PF::DYN_SCORE));
        if (score >= maxScore) w.cutoff = max(w.cutoff, (int)(score * 0.95f));
        w.currentTopScore = score;
    }
    const int chrom = u.c.chromOf(mapStart, baseChrom);
    const int site2 = u.c.siteOf(mapStart);
    const int site3 = u.c.siteOf(mapStop) + blen - 1;
    int ngaps = 0;
    if (site3 - site2 >= MINGAP + blen && locArrayValid) {
        ngaps = makeGapArray<LOC>(u, S, site2, MINGAP);
        if (ngaps < 0) ngaps = 0;
        if (ngaps > 0) {
            if (lane == 0) { S.gaps[0] = min(S.gaps[0], site2); S.gaps[ngaps - 1] = max(S.gaps[ngaps - 1], site3); }
            wsync();
        }
    }
    ngaps = uni(ngaps);
    const bool perfect1 = (score == maxScore && fullyDefined);
    const bool inbounds = (site2 >= 0 && site3 < u.ix->chromLengths[chrom]);
    const bool havePrev = pv.idx >= 0;
    bool makeNew = false, withGaps = false;
    int wb = 0;
    if (inbounds && ngaps == 0 && havePrev && pv.chrom == chrom && pv.strand == strand && overlap(pv.start, pv.stop, site2, site3)) {
        const int betterScore = max(score, pv.score);
        const int minStart = min(pv.start, site2), maxStop = max(pv.stop, site3);
        const bool perfect2 = (pv.score == maxScore && fullyDefined);
        const bool shortEnough = (maxStop - minStart < 2 * blen);
        bbidx_site *pd = &ssl.v[pv.idx];
        if (pv.start == site2 && pv.stop == site3) {
            pv.score = betterScore;
            pv.perfect = (pv.perfect || perfect1 || perfect2) ? 1 : 0;
            if (pv.perfect) pv.semiperfect = 1;
            wb = 1;
        } else if (shortEnough && pv.start == site2 && !pv.semiperfect) {
            if (perfect2) { }
            else if (perfect1) {
                pv.stop = site3;
                if (!pv.perfect) w.perfectsFound++;
                pv.perfect = pv.semiperfect = 1;
            } else {
                pv.stop = maxStop;
                setPerfect(u, S, pv.chrom, pv.strand, pv.start, pv.stop, pv.perfect, pv.semiperfect);
            }
            pv.score = betterScore;
            wb = 2;
        } else if (shortEnough && pv.stop == site3 && !pv.semiperfect) {
            if (perfect2) { }
            else if (perfect1) {
                pv.start = site2;
                if (!pv.perfect) w.perfectsFound++;
                pv.perfect = pv.semiperfect = 1;
            } else {
                pv.start = minStart;
                setPerfect(u, S, pv.chrom, pv.strand, pv.start, pv.stop, pv.perfect, pv.semiperfect);
            }
            pv.score = betterScore;
            wb = 3;
        } else makeNew = true;
        // the merged site goes back to the list after the if-chain: a lane-0 store inside an arm would share its
        // join block with the chain, and every value merged there would count as divergent
        wb = uni(wb);
        if (wb && lane == 0) {
            if (wb == 2) { pd->stop = pv.stop; if (pv.ngaps) pd->gaps[pv.ngaps - 1] = pv.stop; }
            if (wb == 3) { pd->start = pv.start; if (pv.ngaps) pd->gaps[0] = pv.start; }
            pd->perfect = pv.perfect; pd->semiperfect = pv.semiperfect; pd->score = pv.score;
        }
    } else if (inbounds) { makeNew = true; withGaps = true; }
    pv.chrom = uni(pv.chrom); pv.strand = uni(pv.strand); pv.start = uni(pv.start); pv.stop = uni(pv.stop);
    pv.score = uni(pv.score); pv.perfect = uni(pv.perfect); pv.semiperfect = uni(pv.semiperfect); w.perfectsFound = uni(w.perfectsFound);
    if (uni(makeNew)) {
        int sp = perfect1 ? 1 : 0, ssemi = sp;
        if (!perfect1) setPerfect(u, S, chrom, strand, site2, site3, sp, ssemi);
        sp = uni(sp); ssemi = uni(ssemi);
        const int sg = withGaps ? ngaps : 0;
        if (ssl.n >= ssl.cap) { ssl.overflow = true; w.finished = true; }
        else {
            int wv = 0;
            switch (lane) {
                case 0: wv = chrom; break; case 1: wv = strand; break; case 2: wv = site2; break; case 3: wv = site3; break;
                case 4: wv = approxHits; break; case 5: wv = score; break; case 6: wv = sp; break; case 7: wv = ssemi; break;
                case 8: wv = sg; break;
                default: wv = (lane < 9 + sg) ? S.gaps[lane - 9] : 0; break;
            }
            if (lane < 25) ((int *)&ssl.v[ssl.n])[lane] = wv;
            const int idx = ssl.n++;
            bool stopNow = false;
            if (sp) {
                if (!havePrev || !pv.perfect || !(pv.chrom == chrom && pv.strand == strand && overlap(site2, site3, pv.start, pv.stop))) {
                    w.perfectsFound++;
                    if (p.quitAfterTwoPerfects && w.perfectsFound >= 2) stopNow = true;
                }
            }
            pv.idx = idx; pv.chrom = chrom; pv.strand = strand; pv.start = site2; pv.stop = site3; pv.score = score;
            pv.perfect = sp; pv.semiperfect = ssemi; pv.ngaps = sg;
            if (stopNow) w.finished = true;
        }
    }
}

}  // namespace bbidx
