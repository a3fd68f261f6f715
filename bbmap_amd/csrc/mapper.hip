// Mapper control flow around the index probe and the DP, device-resident (include/bbmap_amd.h, "Mapper control flow").
//
// The reference runs this logic in Java, one read (pair) at a time, between its two hot kernels:
//   BBMapThread.processRead      current/align2/BBMapThread.java:389-490
//   BBMapThread.processReadPair  current/align2/BBMapThread.java:943-1098
// A GPU cannot go back to the host between the probe and every single alignment, so the same decisions are taken here by
// small kernels over the whole batch.  Design:
//   * one thread per read (per pair where the two mates interact, per rescue search in the rescue stage): the logic is
//     short, branchy, list-shaped code over a handful of 128-byte site records; a read's records are contiguous in HBM;
//   * scoreSlow is a per-read SEQUENCE (a site's minScore depends on the results of the sites before it, and a fill can ask
//     for a second, wider fill), so every read carries a small state machine and the DP kernels run in ROUNDS: round j
//     aligns the j-th fill of every read that still has one.  Round 1 holds nearly all the work (most reads have one
//     candidate); later rounds are small.  The host only reads three counters per round;
//   * rescue is a stage per anchor mate (mate 1, then mate 2: the second pass sees the sites the first one added):
//     plan (which anchor sites search) -> quick_rescue_kernel (pipeline.hip) -> prepare (ungapped score, tip deletions, DP
//     job) -> DP -> finish (retain / pair / append / merge duplicates).
// Every function names the reference lines it follows.
#include <hip/hip_runtime.h>

#include "index_common.h"
#include "mapper_dev.h"

namespace bbmapper {

// The argument block of a Dev kernel (mapper_dev.h, DEV_KERNEL): the by-value parameter, or the bytes the launch wrote for it at the
// start of the kernel-argument segment (Dev is every such kernel's only parameter).  That segment is read-only global memory, so the
// reference may go to any helper.
template <bool KARG> __device__ __forceinline__ const Dev &dev_of(const Dev &byValue) {
    if (KARG) return *(const Dev *)__builtin_amdgcn_kernarg_segment_ptr();
    return byValue;
}

__device__ inline int imin(int a, int b) { return a < b ? a : b; }
__device__ inline int imax(int a, int b) { return a > b ? a : b; }
__device__ inline int iabsdif(int a, int b) { return a > b ? a - b : b - a; }
__device__ inline int max_quality(const Settings &S, int len) { return S.ptsMatch + (len - 1) * S.ptsMatch2; }      // MSA.maxQuality
__device__ inline int max_imperfect(const Settings &S, int len) { return max_quality(S, len) + S.impDelta; }      // maxImperfectScore

// ---------------------------------------------------------------------------------------------- SiteScore / GapTools
__device__ void fix_gaps2(Site &ss) {                                                        // GapTools.fixGaps2 :127-175
    int ra[BBMSA_MAX_GAPS / 2], rb[BBMSA_MAX_GAPS / 2];
    bool alive[BBMSA_MAX_GAPS / 2];
    const int nr = ss.ngaps / 2;
    for (int i = 0; i < nr; i++) { ra[i] = ss.gaps[2 * i]; rb[i] = ss.gaps[2 * i + 1]; alive[i] = true; }
    for (int i = 1; i < nr; i++)
        if (alive[i - 1] && ra[i] - rb[i - 1] <= MINGAP) { ra[i] = imin(ra[i - 1], ra[i]); rb[i] = imax(rb[i - 1], rb[i]); alive[i - 1] = false; }
    int m = 0;
    for (int i = 0; i < nr; i++) if (alive[i]) { ss.gaps[2 * m] = ra[i]; ss.gaps[2 * m + 1] = rb[i]; m++; }
    ss.ngaps = m < 2 ? 0 : 2 * m;
}
__device__ void fix_gaps(Site &ss) {                                                         // GapTools.fixGaps :27-72
    if (ss.ngaps == 0) return;
    const int a = ss.start, b = ss.stop, n = ss.ngaps;
    int *g = ss.gaps;
    if (!(g[0] <= b && g[n - 1] >= a)) { ss.ngaps = 0; return; }
    int changed = 0;
    if (g[0] != a) { g[0] = a; changed++; }
    if (g[n - 1] != b) { g[n - 1] = b; changed++; }
    for (int i = 0; i < n; i++) { if (g[i] < a) { g[i] = a; changed++; } else if (g[i] > b) { g[i] = b; changed++; } }
    for (int i = 1; i < n; i++) if (g[i - 1] > g[i]) { g[i] = g[i - 1]; changed++; }
    if (changed == 0) return;
    g[0] = a; g[n - 1] = b;
    int remove = 0;
    for (int i = 0; i < n; i += 2) {
        g[i] = imin(imax(g[i], a), b); g[i + 1] = imin(imax(g[i + 1], a), b);
        if (g[i] == g[i + 1]) remove++;
    }
    if (remove) fix_gaps2(ss);
}
__device__ bool check_gaps(const Site &ss) {                                                 // SiteScore.CHECKGAPS
    if (ss.ngaps == 0) return true;
    if (ss.ngaps & 1) return false;
    for (int i = 1; i < ss.ngaps; i++) if (ss.gaps[i - 1] > ss.gaps[i]) return false;
    return ss.gaps[0] == ss.start && ss.gaps[ss.ngaps - 1] == ss.stop;
}
__device__ void set_limits(Site &ss, int a, int b) {                                         // SiteScore.java:905-914
    ss.start = a; ss.stop = b;
    if (ss.ngaps) { ss.gaps[0] = a; ss.gaps[ss.ngaps - 1] = b; if (!check_gaps(ss)) fix_gaps(ss); }
}
__device__ void set_start(Site &ss, int a) {                                                 // :933-942
    ss.start = a;
    if (ss.ngaps) { ss.gaps[0] = a; if (ss.gaps[0] > ss.gaps[1]) fix_gaps(ss); }
}
__device__ void set_stop(Site &ss, int b) {                                                  // :943-951
    ss.stop = b;
    if (ss.ngaps) { ss.gaps[ss.ngaps - 1] = b; fix_gaps(ss); }
}
__device__ void set_slow_score(Site &ss, int x) {                                            // :962-983
    if (x <= 0) ss.pairedScore = x;
    else if (ss.pairedScore > 0) ss.pairedScore = ss.slowScore > 0 ? x + (ss.pairedScore - ss.slowScore) : x + 1;
    ss.slowScore = x;
}
__device__ int calc_gref_len(const Site &ss) {                                               // GapTools.calcGrefLen :80-92
    int total = ss.stop - ss.start + 1;
    for (int i = 2; i < ss.ngaps; i += 2) total -= imax(0, (ss.gaps[i] - ss.gaps[i - 1] - GAPBUFFER2) / GAPLEN) * (GAPLEN - 1);
    return total;
}

// ---------------------------------------------------------------------------------------------- byte scans (one thread)
// A thread's consecutive bytes through aligned 32-bit loads: one thread per read means 64 lanes in 64 different cache lines, and a
// byte load costs the L1 as much as a dword load -- four bytes per access instead of one.  Only words that hold a byte below `n`
// are touched.
struct Words {
    const unsigned *w; unsigned lo; int sh, n, k;
    __device__ void init(const uint8_t *p, int n_) {
        sh = (int)((unsigned long long)p & 3ull); w = (const unsigned *)(p - sh); n = n_; k = 0;
        lo = n > 0 ? w[0] : 0u;
    }
    __device__ unsigned next() {                       // bytes p[4k .. 4k+3] of the k-th call
        k++;
        const unsigned hi = (4 * k - sh < n) ? w[k] : 0u;
        const unsigned x = sh ? __builtin_amdgcn_alignbyte(hi, lo, (unsigned)sh) : lo;
        lo = hi;
        return x;
    }
    // What the next eight calls of next() return, with their eight loads issued together: one trip to L2 / HBM per 32 bytes of a
    // stream instead of eight in a row.  Needs n > 0.  A word next() would not load (none of its bytes is below n) is not loaded here
    // either: the load goes to the last word that holds such a byte, which init() or next() reads as well, and its value is dropped.
    __device__ void next8(unsigned (&x)[8]) {
        const int last = (n + sh - 1) >> 2;
        unsigned hi[8];
#pragma unroll
        for (int j = 0; j < 8; j++) hi[j] = w[k + j + 1 < last ? k + j + 1 : last];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (k + j + 1 > last) hi[j] = 0u;
            x[j] = sh ? __builtin_amdgcn_alignbyte(hi[j], lo, (unsigned)sh) : lo;
            lo = hi[j];
        }
        k += 8;
    }
};
// The byte loops below take two streams four bytes at a time (Words::next) or, with Settings.chunkLoads, eight words at a time
// (Words::next8), and run the same step over every word: step(c4, r4, i) sees bytes i .. i + 3 of both and returns false to stop.
template <class F> __device__ __forceinline__ void words_loop(const Settings &S, int n, Words &A, Words &B, F step) {
    if (S.chunkLoads) {
        for (int i0 = 0; i0 < n; i0 += 32) {
            unsigned c8[8], r8[8];
            A.next8(c8); B.next8(r8);
            // (one copy of the step: the chunk moves down a word per turn instead of being indexed)
#pragma nounroll
            for (int i = i0; i < i0 + 32 && i < n; i += 4) {
                if (!step(c8[0], r8[0], i)) return;
#pragma unroll
                for (int j = 0; j < 7; j++) { c8[j] = c8[j + 1]; r8[j] = r8[j + 1]; }
            }
        }
    } else {
        for (int i = 0; i < n; i += 4) { const unsigned c4 = A.next(), r4 = B.next(); if (!step(c4, r4, i)) return; }
    }
}
// MSA.scoreNoIndels(read, ref, refStart) (MultiStateAligner11tsJNI.java:1034-1089; MultiStateAligner9PacBio.java:1876-1937 is the
// same statement with its own points)
__device__ int score_no_indels(const Settings &S, const uint8_t *read, int len, const uint8_t *ref, int reflen, int refStart) {
    int readStart = 0, readStop = len;
    if (refStart < 0) readStart = -refStart;
    if (refStart + len > reflen) readStop -= (refStart + len - reflen);
    int score = 0, mode = -1, t = 0;                  // mode 0 = match streak, 1 = substitution streak
    const int n = readStop - readStart;
    if (n <= 0) return 0;
    Words A, B;
    A.init(read + readStart, n); B.init(ref + refStart + readStart, n);
    words_loop(S, n, A, B, [&](unsigned c4, unsigned r4, int i) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (i + q < n) {
                const int c = (int)((c4 >> (8 * q)) & 255u), r = (int)((r4 >> (8 * q)) & 255u);
                if (c == r && c != 'N') { if (mode == 0) { t++; score += S.ptsMatch2; } else { t = 0; score += S.ptsMatch; } mode = 0; }
                else if (c >= 128 || c == 'N') { }
                else if (r >= 128 || r == 'N') { }
                else { if (mode == 1) t++; else t = 0; score += (t + 1 > 5 ? S.ptsSub3 : (t + 1 > 1 ? S.ptsSub2 : S.ptsSub)); mode = 1; }
            }
        }
        return true;
    });
    return score;
}
// SiteScore.setPerfect(bases) (current/stream/SiteScore.java:239-292)
__device__ void set_perfect(const Settings &S, Site &ss, const uint8_t *bases, int len, const uint8_t *ref, int reflen) {
    ss.perfect = 0; ss.semiperfect = 0;
    if (len != ss.stop - ss.start + 1) return;
    bool perfect = true, semi = true;
    int refloc = ss.start, readloc = 0, N = 0;
    const int mx = imin(ss.stop, reflen - 1), nlimit = len / 2;
    if (ss.start < 0) { N -= ss.start; readloc -= ss.start; refloc -= ss.start; perfect = false; }
    if (ss.stop >= reflen) { N += (ss.stop - reflen + 1); perfect = false; }
    if (N > nlimit) return;
    const int n = mx - refloc + 1;
    if (n > 0) {
        Words A, B;
        A.init(bases + readloc, n); B.init(ref + refloc, n);
        bool gaveUp = false;
        words_loop(S, n, A, B, [&](unsigned c4, unsigned r4, int i) __attribute__((always_inline)) {
            if (c4 == r4 && !(((c4 ^ 0x4E4E4E4Eu) - 0x01010101u) & ~(c4 ^ 0x4E4E4E4Eu) & 0x80808080u) && i + 4 <= n) return true;   // four equal bases, none of them 'N'
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (i + q < n) {
                    const int c = (int)((c4 >> (8 * q)) & 255u), r = (int)((r4 >> (8 * q)) & 255u);
                    if (c != r || c == 'N') {
                        perfect = false;
                        if (c == 'N') semi = false;
                        if (r != 'N' || (N = N + 1) > nlimit) { gaveUp = true; return false; }
                    }
                }
            }
            return true;
        });
        if (gaveUp) return;
    }
    semi = semi && N <= nlimit;
    perfect = perfect && semi && N == 0;
    ss.perfect = perfect; ss.semiperfect = semi;
}
// findTipDeletionsRight / Left (AbstractMapThread.java:2178-2292); ChromosomeArray.minIndex is 0 for these arrays
__device__ int tip_right(const uint8_t *bases, int len, const uint8_t *ref, int reflen, int originalStop, int searchDist, int tiplen) {
    if (originalStop < tiplen - 1) return 0;
    int bestStart = originalStop, lastMismatch = 0, originalMismatches = 0, contig = 0;
    const int tipCoord = len - 1;
    for (int i = 0; i < tiplen && contig < 5; i++) {
        if (bases[tipCoord - i] != ref[originalStop - i]) { originalMismatches++; lastMismatch = i; contig = 0; } else contig++;
    }
    if (originalMismatches < 3) return 0;
    int minMismatches = originalMismatches;
    tiplen = lastMismatch + 1;
    if (tiplen < 4) return 0;
    searchDist = imin(searchDist, 30 * originalMismatches);
    const int last = imin(reflen - 1, originalStop + searchDist);
    // The tip (byte j = bases[tipCoord - j]) against a sliding window of the reference (byte j = ref[start - j]): one reference byte
    // enters per position and the mismatches of the first `tiplen` bytes are counted in one go -- the same count the byte loop
    // reaches whenever it stays below minMismatches, which is all the comparison uses.
    unsigned long long T = 0, Wd = 0;
    for (int j = 0; j < 8; j++) T |= (unsigned long long)bases[tipCoord - j] << (8 * j);
    for (int j = 1; j < 8; j++) Wd |= (unsigned long long)ref[originalStop + 1 - j] << (8 * (j - 1));      // the window of start - 1, about to shift
    const unsigned long long keep = tiplen >= 8 ? 0x8080808080808080ull : ((1ull << (8 * tiplen)) - 1) & 0x8080808080808080ull;
    for (int start = originalStop + 1; start <= last && minMismatches > 0; start++) {
        Wd = (Wd << 8) | ref[start];
        const unsigned long long x = Wd ^ T;
        const int mm = __builtin_popcountll((((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x) & keep);
        if (mm < minMismatches) { bestStart = start; minMismatches = mm; }
    }
    if (minMismatches > 2 || originalMismatches - minMismatches < 2) return 0;
    return bestStart - originalStop;
}
__device__ int tip_left(const uint8_t *bases, const uint8_t *ref, int reflen, int originalStart, int searchDist, int tiplen) {
    if (originalStart + tiplen >= reflen) return 0;
    if (0 >= originalStart) return 0;
    int bestStart = originalStart, lastMismatch = 0, originalMismatches = 0, contig = 0;
    for (int i = 0; i < tiplen && contig < 5; i++) {
        if (bases[i] != ref[originalStart + i]) { originalMismatches++; lastMismatch = i; contig = 0; } else contig++;
    }
    if (originalMismatches < 3) return 0;
    int minMismatches = originalMismatches;
    tiplen = lastMismatch + 1;
    if (tiplen < 4) return 0;
    searchDist = imin(searchDist, 16 + 16 * originalMismatches + 8 * tiplen);
    const int last = imax(0, originalStart - searchDist);
    // as in tip_right: tip byte j = bases[j], window byte j = ref[start + j]; the window moves left one reference byte at a time
    unsigned long long T = 0, Wd = 0;
    for (int j = 0; j < 8; j++) T |= (unsigned long long)bases[j] << (8 * j);
    for (int j = 1; j < 8; j++) Wd |= (unsigned long long)ref[originalStart - 1 + j] << (8 * (j - 1));     // the window of start + 1, about to shift
    const unsigned long long keep = tiplen >= 8 ? 0x8080808080808080ull : ((1ull << (8 * tiplen)) - 1) & 0x8080808080808080ull;
    for (int start = originalStart - 1; start >= last && minMismatches > 0; start--) {
        Wd = (Wd << 8) | ref[start];
        const unsigned long long x = Wd ^ T;
        const int mm = __builtin_popcountll((((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x) & keep);
        if (mm < minMismatches) { bestStart = start; minMismatches = mm; }
    }
    if (minMismatches > 2 || originalMismatches - minMismatches < 2) return 0;
    return originalStart - bestStart;
}
// findTipDeletions(ss, bases, maxImperfectScore, lookRight, lookLeft) (AbstractMapThread.java:1107-1141)
__device__ bool find_tip_deletions(const Settings &S, Site &ss, const uint8_t *bases, int len, const uint8_t *ref, int reflen,
                                   int maxImp, bool lookRight, bool lookLeft) {
    if (ss.slowScore >= maxImp) return false;
    if (len <= 2 * TIP_MAX_TIPLEN) return false;
    int maxSearch = imin(S.tipSearchDist, S.alignColumns - (S.slowRescuePadding + 8 + imax(len, ss.stop - ss.start)));
    if (maxSearch < 1) return false;
    bool changed = false;
    if (lookRight) {
        const int x = tip_right(bases, len, ref, reflen, ss.stop, maxSearch, TIP_MAX_TIPLEN);
        if (x > 0) {
            set_stop(ss, ss.stop + x); changed = true;
            maxSearch = imin(maxSearch, S.alignColumns - (S.slowRescuePadding + 8 + imax(len, ss.stop - ss.start)));
            if (maxSearch < 1) return changed;
        }
    }
    if (lookLeft) {
        const int y = tip_left(bases, ref, reflen, ss.start, maxSearch, TIP_MAX_TIPLEN);
        if (y > 0) { set_start(ss, ss.start - y); changed = true; }
    }
    return changed;
}

// ---------------------------------------------------------------------------------------------- list tools
__device__ inline int cmp_score(const Site &a, const Site &b) {                              // SiteScore.compareTo :55-73
    int x = b.score - a.score; if (x) return x;
    x = b.slowScore - a.slowScore; if (x) return x;
    x = b.pairedScore - a.pairedScore; if (x) return x;
    x = b.quickScore - a.quickScore; if (x) return x;
    x = a.chrom - b.chrom; if (x) return x;
    return a.start - b.start;
}
__device__ inline int cmp_pos(const Site &a, const Site &b) {                                // PositionComparator :379-395
    if (a.chrom != b.chrom) return a.chrom - b.chrom;
    if (a.start != b.start) return a.start - b.start;
    if (a.stop != b.stop) return a.stop - b.stop;
    if (a.strand != b.strand) return a.strand - b.strand;
    if (a.score != b.score) return b.score - a.score;
    if (a.slowScore != b.slowScore) return b.slowScore - a.slowScore;
    if (a.quickScore != b.quickScore) return b.quickScore - a.quickScore;
    if (a.perfect != b.perfect) return a.perfect ? -1 : 1;
    if (a.rescued != b.rescued) return a.rescued ? 1 : -1;
    return 0;
}
// stable insertion sort (Collections.sort is a stable merge sort: same order)
template <bool BYPOS> __device__ void sort_sites(Site *s, int n) {
    for (int i = 1; i < n; i++) {
        if ((BYPOS ? cmp_pos(s[i - 1], s[i]) : cmp_score(s[i - 1], s[i])) <= 0) continue;       // already in place (the common case)
        const Site t = s[i];
        int j = i - 1;
        while (j >= 0 && (BYPOS ? cmp_pos(s[j], t) : cmp_score(s[j], t)) > 0) { s[j + 1] = s[j]; j--; }
        s[j + 1] = t;
    }
}
// Entries marked for removal (Tools.condenseStrict's nulls): the first 64 list positions in a register mask, positions beyond
// (only the overflow tier has lists that long) as a mark in the record itself (reserved[1], zero in every list entry otherwise).
struct DeadSet {
    unsigned long long lo = 0; bool hi = false;
    __device__ void mark(Site *s, int i) { if (i < 64) lo |= 1ull << i; else { s[i].reserved[1] = DEAD_MARK; hi = true; } }
    __device__ bool dead(const Site *s, int i) const { return i < 64 ? ((lo >> i) & 1) != 0 : (hi && s[i].reserved[1] == DEAD_MARK); }
    __device__ bool any() const { return lo != 0 || hi; }
};
// order-preserving removal of the marked entries
__device__ int condense(Site *s, int n, const DeadSet &dead) {
    if (!dead.any()) return n;
    int m = 0;
    for (int i = 0; i < n; i++) if (!dead.dead(s, i)) { if (m != i) s[m] = s[i]; m++; }
    return m;
}
// Tools.trimSitesBelowCutoff (Tools.java:1113-1161)
__device__ int trim_below_cutoff(Site *s, int n, int cutoff, bool retainPaired, int minRetain, int maxRetain) {
    if (n <= minRetain) return n;
    if (n > maxRetain) n = maxRetain;
    DeadSet dead;
    int removed = 0;
    const int maxToRemove = n - minRetain;
    for (int i = n - 1; i >= 0; i--) {
        if (!s[i].semiperfect && s[i].score < cutoff && (!retainPaired || s[i].pairedScore <= 0)) {       // retainSemiperfect is always true here
            dead.mark(s, i); removed++;
            if (removed >= maxToRemove) break;
        }
    }
    return condense(s, n, dead);
}
// Tools.trimSiteList (Tools.java:654-674)
__device__ int trim_site_list(Site *s, int &n, float fraction, bool retainPaired, int minRetain, int maxRetain) {
    if (n == 0) return -999999;
    if (n == 1) return s[0].score;
    int maxScore = -999999;
    if (minRetain > 1 && minRetain < n) maxScore = s[0].score;
    else for (int i = 0; i < n; i++) maxScore = imax(maxScore, s[i].score);
    n = trim_below_cutoff(s, n, (int)__fmul_rn((float)maxScore, fraction), retainPaired, minRetain, maxRetain);
    return maxScore;
}
// BBMapThread.trimList, USE_AFFINE_SCORE branch (BBMapThread.java:140-197)
__device__ void trim_list(Site *s, int &n, bool retainPaired, int maxScore, bool specialCasePerfect, int minRetain, int maxRetain) {
    if (n < 2) return;
    const int highest = trim_site_list(s, n, .6f, retainPaired, minRetain, maxRetain);
    if (highest == maxScore && specialCasePerfect) {
        trim_site_list(s, n, .94f, retainPaired, minRetain, maxRetain);
        if (n > 8) trim_site_list(s, n, .99f, retainPaired, minRetain, maxRetain);
        return;
    }
    const int mstr2 = minRetain <= 1 ? 1 : minRetain + 1;
    if (n > 4) trim_site_list(s, n, .65f, retainPaired, minRetain, maxRetain);
    if (n > 8) trim_site_list(s, n, .7f, retainPaired, minRetain, maxRetain);
    if (n > 12) trim_site_list(s, n, .75f, retainPaired, minRetain, maxRetain);
    if (n > 16) trim_site_list(s, n, .8f, retainPaired, minRetain, maxRetain);
    if (n > 20) trim_site_list(s, n, .85f, retainPaired, minRetain, maxRetain);
    if (n > 24) trim_site_list(s, n, .9f, retainPaired, minRetain, maxRetain);
    if (n > 32) trim_site_list(s, n, .95f, retainPaired, minRetain, maxRetain);
    if (n > 40) trim_site_list(s, n, .97f, retainPaired, mstr2, maxRetain);
    if (n > 48) trim_site_list(s, n, .99f, retainPaired, mstr2, maxRetain);
}
__device__ bool positional_match(const Site &a, const Site &b, bool testGaps) {              // SiteScore.java:353-365
    if (a.chrom != b.chrom || a.strand != b.strand || a.start != b.start || a.stop != b.stop) return false;
    if (!testGaps || (a.ngaps == 0 && b.ngaps == 0)) return true;
    if (a.ngaps != b.ngaps) return false;
    for (int i = 0; i < a.ngaps; i++) if (a.gaps[i] != b.gaps[i]) return false;
    return true;
}
// Tools.mergeDuplicateSites(list, true, true) (Tools.java:697-759)
__device__ int merge_duplicate_sites(Site *s, int n) {
    if (n < 2) return n;
    sort_sites<true>(s, n);
    DeadSet dead;
    int ai = 0;
    for (int i = 1; i < n; i++) {
        Site &a = s[ai];
        const Site &b = s[i];
        const bool exact = positional_match(a, b, true);
        if (exact || positional_match(a, b, false)) {
            bool takeB = false;                        // different gaps: the better of the two lends its gap array
            if (!exact) {
                if (a.score != b.score) takeB = b.score > a.score;
                else if (a.slowScore != b.slowScore) takeB = b.slowScore > a.slowScore;
                else if (a.pairedScore != b.pairedScore) takeB = b.pairedScore > a.pairedScore;
            }
            set_slow_score(a, imax(a.slowScore, b.slowScore));
            a.pairedScore = (a.pairedScore <= a.slowScore && b.pairedScore <= a.slowScore) ? 0 : imax(0, imax(a.pairedScore, b.pairedScore));
            a.score = imax(a.score, b.score);
            a.perfect = (a.perfect || b.perfect);
            a.semiperfect = (a.semiperfect || b.semiperfect);
            if (takeB) { a.ngaps = b.ngaps; for (int q = 0; q < BBMSA_MAX_GAPS; q++) a.gaps[q] = b.gaps[q]; }
            dead.mark(s, i);
        } else ai = i;
    }
    return condense(s, n, dead);
}
// Tools.removeLowQualitySitesPaired (Tools.java:934-960)
__device__ int remove_low_quality_paired(Site *s, int n, int maxSw, float multSingle, float multPaired) {
    if (n == 0) return 0;
    const int thresh = (int)__fmul_rn((float)maxSw, multSingle), threshPaired = (int)__fmul_rn((float)maxSw, multPaired);
    if (s[0].score < threshPaired) return 0;
    DeadSet dead;
    for (int i = n - 1; i >= 0; i--) {
        if (s[i].pairedScore > 0) { if (s[i].slowScore < threshPaired) dead.mark(s, i); }
        else if (s[i].slowScore < thresh) dead.mark(s, i);
    }
    return condense(s, n, dead);
}

// ---------------------------------------------------------------------------------------------- stage 1: begin
// quickMap's tail for one read: probe records -> SiteScores, removeOutOfBounds (AbstractMapThread.java:2444-2476).  SCAF: a scaffold
// table is set, and a site that spans two scaffolds goes too (the SAM_OUT branch, Data.isSingleScaffold); `dropped` counts those.
template <bool SCAF>
__device__ int load_sites_t(const Dev &D, long long r, Site *s, int &dropped) {
    const int ns = D.pnsites[r];
    if (ns < 0) return -1;                                 // the probe ran out of room (or declined the read): reported, not mapped
    const bbidx_site *ps = D.psites + r * (long long)D.maxSites;
    const int len = D.reads[r].len;
    int n = 0;
    for (int i = 0; i < ns; i++) {
        Site ss;
        ss.chrom = ps[i].chrom; ss.strand = ps[i].strand; ss.start = ps[i].start; ss.stop = ps[i].stop; ss.hits = ps[i].hits;
        ss.quickScore = ss.score = ps[i].score; ss.slowScore = 0; ss.pairedScore = 0;
        ss.perfect = ps[i].perfect; ss.semiperfect = ps[i].semiperfect; ss.rescued = 0;
        ss.ngaps = ps[i].ngaps;
        for (int q = 0; q < BBMSA_MAX_GAPS; q++) ss.gaps[q] = ps[i].gaps[q];
        ss.match_job = -1; ss.reserved[0] = ss.reserved[1] = 0;
        const int mx = D.chromArrLen[ss.chrom] - 1;
        if (ss.start < 0 || ss.stop > mx) continue;
        if (SCAF && !bbscaf::is_single_scaffold(D.scaf, ss.chrom, ss.start, ss.stop)) { dropped++; continue; }
        if (calc_gref_len(ss) >= D.S.expLimit) { set_stop(ss, ss.start + imin(len + 40, D.S.expLimit)); if (ss.ngaps) fix_gaps(ss); }
        s[n++] = ss;
    }
    return n;
}
// (a uniform branch on the kernel argument: without a table the instantiation is the plain removeOutOfBounds)
__device__ inline int load_sites(const Dev &D, long long r, Site *s, int &dropped) {
    return D.scaf.off ? load_sites_t<true>(D, r, s, dropped) : load_sites_t<false>(D, r, s, dropped);
}
// One atomic per wavefront for a per-lane count (any set of active lanes; the lanes of `m` are active, so the shuffles read live values).
__device__ inline void wave_add(unsigned *ctr, int v) {
    const unsigned long long m = __ballot(v != 0);
    if (!m) return;
    unsigned tot = 0;
    for (unsigned long long b = m; b; b &= b - 1) tot += (unsigned)__shfl(v, __builtin_ctzll(b));
    if ((int)(threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(ctr, tot);
}

// Class lists (Dev.classList).  Appends a lane's reads ra and rb (the mates of its pair; rb < 0: one read) to the long-path (class 0)
// or the short-path list (class 1), a read of class < 0 to neither.  One reservation per wavefront for both lists and both reads --
// the two counters are neighbours and take one 64-bit add -- and behind it the lanes' reads in lane order, ra before rb (as
// slow_round_kernel builds activeOut).  The class only decides which reads share a wavefront: a read on the "wrong" list is
// processed like any other.
__device__ inline void class_append(const Dev &D, long long ra, int ca, long long rb, int cb) {
    const int lane = threadIdx.x & 63;
    if (D.classSwap) { if (ca >= 0) ca ^= 1; if (cb >= 0) cb ^= 1; }
    if (rb < 0) cb = -1;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long a0 = __ballot(ca == 0), b0 = __ballot(cb == 0), a1 = __ballot(ca == 1), b1 = __ballot(cb == 1);
    const unsigned long long any = a0 | b0 | a1 | b1;
    if (!any) return;
    const int lead = __builtin_ctzll(any);
    const unsigned long long n0 = __builtin_popcountll(a0) + __builtin_popcountll(b0), n1 = __builtin_popcountll(a1) + __builtin_popcountll(b1);
    unsigned long long base = 0;
    static_assert(CNT_CLASS_SHORT == CNT_CLASS_LONG + 1 && CNT_CLASS_LONG % 2 == 0, "the two class counters are one aligned 64-bit word");
    if (lane == lead) base = atomicAdd(reinterpret_cast<unsigned long long *>(&D.counters[CNT_CLASS_LONG]), n0 | (n1 << 32));
    base = __shfl(base, lead);
    const long long at0 = (long long)(unsigned)base + __builtin_popcountll(a0 & below) + __builtin_popcountll(b0 & below);
    const long long at1 = D.nreads + (long long)(unsigned)(base >> 32) + __builtin_popcountll(a1 & below) + __builtin_popcountll(b1 & below);
    if (ca == 0) D.classList[at0] = (int)ra; else if (ca == 1) D.classList[at1] = (int)ra;
    if (cb == 0) D.classList[at0 + (ca == 0)] = (int)rb; else if (cb == 1) D.classList[at1 + (ca == 1)] = (int)rb;
}
// thread t's read in a first round that follows the class lists: the long list, then the short one; -1 beyond both
__device__ inline long long class_read(const Dev &D, long long t) {
    const long long nl = D.counters[CNT_CLASS_LONG], ns = D.counters[CNT_CLASS_SHORT];
    if (t < nl) return D.classList[t];
    if (t < nl + ns) return D.classList[D.nreads + (t - nl)];
    return -1;
}
// the state score_kernel gives a read without a site list; with class lists such a read is on neither, and begin_kernel writes it
__device__ inline SlowState slow_finished() {
    SlowState st; st.idx = 0; st.phase = 3; st.minMsaLimit = 0; st.pending = -1; st.oldJob = -1; st.expectedLen = 0; st.minscore = 0; st.seq = 0;
    return st;
}
// begin_kernel's class of a read with n sites: short path when every site is perfect (score_kernel then has no reference to read,
// scoreSlow no fill to ask for)
__device__ inline int begin_class(const Dev &D, long long r, const Site *s, int n) {
    if (n <= 0) { D.slow[r] = slow_finished(); return -1; }
    for (int i = 0; i < n; i++) if (!s[i].perfect) return 0;
    return 1;
}

// pairSiteScoresInitial (BBMapThread.java:736-940); REQUIRE_CORRECT_STRANDS_PAIRS = true, SAME_STRAND_PAIRS = false
__device__ void pair_initial(const Settings &S, Site *s1, int &n1, Site *s2, int &n2, int len1, int len2) {
    if (n1 < 1 || n2 < 1) return;
    sort_sites<true>(s1, n1); sort_sites<true>(s2, n2);
    for (int i = 0; i < n1; i++) s1[i].pairedScore = 0;
    for (int i = 0; i < n2; i++) s2[i].pairedScore = 0;
    int maxPaired1 = -1, maxPaired2 = -1, numPerfectPairs = 0;
    const int ilimit = n1 - 1, jlimit = n2 - 1, maxReadLen = imax(len1, len2);
    const int outerDistLimit = (maxReadLen * OUTER_DIST_MULT) / OUTER_DIST_DIV, innerDistLimit = S.maxPairDist;
    const int expectedFragLength = S.averagePairDist + len1 + len2;
    for (int i = 0, j = 0; i <= ilimit && j <= jlimit; i++) {
        Site &a = s1[i];
        while (j < jlimit && (s2[j].chrom < a.chrom || (s2[j].chrom == a.chrom && a.start - s2[j].stop > innerDistLimit))) j++;
        for (int k = j; k <= jlimit; k++) {
            Site &b = s2[k];
            if (b.chrom > a.chrom) break;
            if (b.start - a.stop > innerDistLimit) break;
            int innerdist, outerdist;
            if (a.strand != b.strand) {
                if (a.strand == 0) { innerdist = b.start - a.stop; outerdist = b.stop - a.start; }
                else { innerdist = a.start - b.stop; outerdist = a.stop - b.start; }
            } else if (a.start <= b.start) { innerdist = b.start - a.stop; outerdist = b.stop - a.start; }
            else { innerdist = a.start - b.stop; outerdist = a.stop - b.start; }
            if (outerdist >= outerDistLimit && innerdist <= innerDistLimit && a.strand != b.strand) {
                const int deviation = iabsdif(S.averagePairDist, innerdist);
                const int ps1 = a.score + 1 + imax(1, b.score / 2 - ((deviation * b.score) / (32 * expectedFragLength + 100)));
                const int ps2 = b.score + 1 + imax(1, a.score / 2 - ((deviation * a.score) / (32 * expectedFragLength + 100)));
                bool p1 = false, p2 = false;
                if (ps1 > a.pairedScore) { p1 = true; a.pairedScore = ps1; maxPaired1 = imax(a.score, maxPaired1); }
                if (ps2 > b.pairedScore) { p2 = true; b.pairedScore = ps2; maxPaired2 = imax(b.score, maxPaired2); }
                if (p1 && p2 && outerdist >= maxReadLen && deviation <= expectedFragLength && a.perfect && b.perfect) numPerfectPairs++;
            }
        }
    }
    for (int i = 0; i < n1; i++) if (s1[i].pairedScore > s1[i].score) s1[i].score = s1[i].pairedScore;
    for (int i = 0; i < n2; i++) if (s2[i].pairedScore > s2[i].score) s2[i].score = s2[i].pairedScore;
    if (S.trimList) {
        if (numPerfectPairs > 0) {
            n1 = trim_below_cutoff(s1, n1, (int)__fmul_rn((float)maxPaired1, .94f), false, 1, S.maxTrimSitesToRetain);
            n2 = trim_below_cutoff(s2, n2, (int)__fmul_rn((float)maxPaired2, .94f), false, 1, S.maxTrimSitesToRetain);
        } else {
            if (n1 > 4) n1 = trim_below_cutoff(s1, n1, (int)__fmul_rn((float)maxPaired1, .9f), true, 1, S.maxTrimSitesToRetain);
            if (n2 > 4) n2 = trim_below_cutoff(s2, n2, (int)__fmul_rn((float)maxPaired2, .9f), true, 1, S.maxTrimSitesToRetain);
        }
    }
}

// one thread per read (single) or per pair: BBMapThread.java:405-431 / :953-1017
__global__ __launch_bounds__(128) void begin_kernel(const Dev D) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (D.S.paired) {
        if (2 * u + 1 >= D.nreads) return;
        const long long r1 = 2 * u, r2 = r1 + 1;
        Site *s1 = D.ms + r1 * D.cap, *s2 = D.ms + r2 * D.cap;
        int drop1 = 0, drop2 = 0;
        int n1 = load_sites(D, r1, s1, drop1), n2 = load_sites(D, r2, s2, drop2);
        if (n1 < 0 || n2 < 0) {                            // one mate's probe overflowed: the pair is reported, not mapped
            atomicAdd(&D.counters[CNT_OVERFLOWED], (unsigned)((n1 < 0) + (n2 < 0)));
            D.mcount[r1] = n1 < 0 ? -1 : -2; D.mcount[r2] = n2 < 0 ? -1 : -2;
            if (D.classList) { D.slow[r1] = slow_finished(); D.slow[r2] = slow_finished(); }
            return;                                        // (the overflow tier maps the pair again and counts its removals there)
        }
        if (D.scaf.off) wave_add(&D.counters[CNT_CROSS_SCAFFOLD], drop1 + drop2);
        const int len1 = D.reads[r1].len, len2 = D.reads[r2].len;
        pair_initial(D.S, s1, n1, s2, n2, len1, len2);
        if (D.S.trimList) {
            if (n1 > MIN_TRIM_PAIRED) sort_sites<false>(s1, n1);
            if (n2 > MIN_TRIM_PAIRED) sort_sites<false>(s2, n2);
            trim_list(s1, n1, true, max_quality(D.S, len1), false, MIN_TRIM_PAIRED, D.S.maxTrimSitesToRetain);
            trim_list(s2, n2, true, max_quality(D.S, len2), false, MIN_TRIM_PAIRED, D.S.maxTrimSitesToRetain);
        }
        for (int i = 0; i < n1; i++) s1[i].score = s1[i].quickScore;
        for (int i = 0; i < n2; i++) s2[i].score = s2[i].quickScore;
        D.mcount[r1] = n1; D.mcount[r2] = n2;
        if (n1 == 0) atomicAdd(&D.counters[CNT_NO_SITE], 1u);
        if (n2 == 0) atomicAdd(&D.counters[CNT_NO_SITE], 1u);
        if (D.classList) class_append(D, r1, begin_class(D, r1, s1, n1), r2, begin_class(D, r2, s2, n2));
    } else {
        if (u >= D.nreads) return;
        Site *s = D.ms + u * D.cap;
        int drop = 0;
        int n = load_sites(D, u, s, drop);
        if (n < 0) { atomicAdd(&D.counters[CNT_OVERFLOWED], 1u); D.mcount[u] = -1; if (D.classList) D.slow[u] = slow_finished(); return; }
        if (D.scaf.off) wave_add(&D.counters[CNT_CROSS_SCAFFOLD], drop);
        if (D.S.trimList && n > 1) {
            sort_sites<false>(s, n);
            trim_list(s, n, false, max_quality(D.S, D.reads[u].len), true, MIN_TRIM_SINGLE, D.S.maxTrimSitesToRetain);
        }
        D.mcount[u] = n;
        if (n == 0) atomicAdd(&D.counters[CNT_NO_SITE], 1u);
        if (D.classList) class_append(D, u, begin_class(D, u, s, n), -1, -1);
    }
}

// ---------------------------------------------------------------------------------------------- stage 2: scoreNoIndels + sort + tip deletions
// AbstractMapThread.scoreNoIndels (:762-856), Collections.sort, findTipDeletions (:1075-1105), and scoreSlow's opening
// (BBMapThread.java:255-260).  One thread per read.
// (six waves per SIMD, as before the byte loops had chunks: the bound keeps the chunk from costing one)
#ifndef SCORE_MIN_WAVES
#define SCORE_MIN_WAVES 6
#endif
template <bool KARG> __global__ __launch_bounds__(128, SCORE_MIN_WAVES) void score_kernel(const Dev Darg) {
    const Dev &D = dev_of<KARG>(Darg);
    long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= D.nreads) return;
    if (D.classList && (r = class_read(D, r)) < 0) return;
    SlowState st = slow_finished();
    const int n = D.mcount[r];
    if (n <= 0) { D.slow[r] = st; return; }
    const bbidx_read rr = D.reads[r];
    const int len = rr.len, maxSw = max_quality(D.S, len), maxImp = max_imperfect(D.S, len);
    Site *s = D.ms + r * D.cap;
    int near = 0; bool force = false;
    for (int j = 0; j < n; j++) {
        Site &ss = s[j];                                   // in place: a site is 128 bytes, the loop touches a dozen of its fields
        const int oldScore = ss.score;
        const uint8_t *bases = D.bases + rr.bases_off + (ss.strand ? D.minusDelta : 0);
        if (ss.perfect) { near++; set_slow_score(ss, maxSw); ss.score = maxSw; ss.ngaps = 0; }
        else {
            const uint8_t *ref = D.chromArr[ss.chrom]; const int reflen = D.chromArrLen[ss.chrom];
            int sw = score_no_indels(D.S, bases, len, ref, reflen, ss.start);
            if (sw < oldScore && oldScore >= maxImp && ss.stop - ss.start + 1 != len) {            // :806-813
                const int sw2 = score_no_indels(D.S, bases, len, ref, reflen, ss.stop - len + 1);
                if (sw2 >= maxImp) { sw = sw2; set_start(ss, ss.stop - len + 1); set_perfect(D.S, ss, bases, len, ref, reflen); }
            }
            set_slow_score(ss, sw); ss.score = sw;
            if (sw >= maxImp) {
                near++;
                set_stop(ss, ss.start + len - 1); ss.ngaps = 0;
                if (sw >= maxSw) ss.perfect = ss.semiperfect = 1;
                else set_perfect(D.S, ss, bases, len, ref, reflen);
            } else if (oldScore >= maxImp) force = true;
        }
    }
    const int numNear = force ? -near : near;
    sort_sites<false>(s, n);
    if (numNear < 1 && D.S.tipSearchDist > 0) {
        for (int j = 0; j < n; j++) {
            if (!s[j].semiperfect && s[j].slowScore < maxImp) {
                Site ss = s[j];
                const uint8_t *bases = D.bases + rr.bases_off + (ss.strand ? D.minusDelta : 0);
                const uint8_t *ref = D.chromArr[ss.chrom]; const int reflen = D.chromArrLen[ss.chrom];
                if (find_tip_deletions(D.S, ss, bases, len, ref, reflen, maxImp, true, true)) {
                    ss.match_job = -1;
                    set_slow_score(ss, score_no_indels(D.S, bases, len, ref, reflen, ss.start));
                    if (ss.slowScore == maxSw) { set_stop(ss, ss.start + len - 1); ss.perfect = ss.semiperfect = 1; }
                    else { ss.perfect = 0; set_perfect(D.S, ss, bases, len, ref, reflen); }
                    s[j] = ss;
                }
            }
        }
    }
    D.nearArr[r] = numNear;
    if (D.S.paired || numNear < 1) {                       // single-ended: scoreSlow only without a near-perfect site (:466)
        st.phase = 0;
        st.minMsaLimit = -D.S.clearzone1e + (int)__fmul_rn(D.S.paired ? D.S.ratioPreRescue : D.S.minRatio, (float)maxSw);
    }
    D.slow[r] = st;
}

// ---------------------------------------------------------------------------------------------- stage 3: scoreSlow rounds
__device__ inline bbmsa_job make_job(const Dev &D, const bbidx_read &rr, const Site &ss, int pad, int minscore) {
    bbmsa_job j;
    j.read_off = rr.bases_off + (ss.strand ? D.minusDelta : 0);
    j.ref_off = (long long)(D.chromArr[ss.chrom] - D.refsBase);
    j.read_len = rr.len; j.ref_len = D.chromArrLen[ss.chrom];
    j.refStartLoc = ss.start - pad; j.refEndLoc = ss.stop + pad;
    j.minScore = minscore;
    j.flags = BBMSA_FILL_AND_SCORE_LIMITED | BBMSA_DO_TRACEBACK;
    return j;
}
// appends one fill to the plain or (sites with a gap array) the gapped log; returns its index (GAPPED_BIT marks the gapped log), or
// NO_ROOM when that log is full: the caller then leaves its state untouched and asks again in the next round, before which the host
// has grown the log (the reference's lists have no capacity; nothing may be lost or the batch refused because a log was sized too small)
constexpr int NO_ROOM = -2;
// A log slot for every lane that is here: one atomicAdd for all of them (the lanes of a wavefront that emit in the same turn of their
// loops), slots in lane order.  With the class lists a wavefront of the first round is all fills, and one add per fill on one word
// is what the round then waits for; the counter ends at the same value either way.
__device__ inline unsigned wave_slot(unsigned *ctr) {
    const unsigned long long m = __ballot(true);
    const int lane = threadIdx.x & 63, lead = __builtin_ctzll(m);
    unsigned base = 0;
    if (lane == lead) base = atomicAdd(ctr, (unsigned)__builtin_popcountll(m));
    base = __shfl(base, lead);
    return base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
}
__device__ int emit_fill(const Dev &D, long long r, const bbidx_read &rr, const Site &ss, int site, int pad, int minscore, int kind, int seq) {
    bbmap_jobinfo info; info.read = (int)r; info.seq = seq; info.kind = kind; info.site = site;
    const bbmsa_job j = make_job(D, rr, ss, pad, minscore);
    // the wide list (second DP context: BBMap's 3000 columns) takes the sites with a gap array and the windows wider than the
    // first context's column limit; a job without gaps is an ordinary job there
    if (ss.ngaps || (imin(j.ref_len - 1, j.refEndLoc) - imax(0, j.refStartLoc) + 1) > D.plainColumns) {
        const unsigned k = D.classList ? wave_slot(&D.counters[CNT_GAPPED_FILLS]) : atomicAdd(&D.counters[CNT_GAPPED_FILLS], 1u);
        if ((long long)k >= D.gjobCap) return NO_ROOM;
        D.gjobs[k] = j; D.ginfo[k] = info;
        bbmsa_gaps g; g.ngaps = ss.ngaps;
        for (int q = 0; q < BBMSA_MAX_GAPS; q++) g.gaps[q] = q < ss.ngaps ? ss.gaps[q] : 0;
        D.ggaps[k] = g;
        return (int)k | GAPPED_BIT;
    }
    const unsigned k = D.classList ? wave_slot(&D.counters[CNT_FILLS]) : atomicAdd(&D.counters[CNT_FILLS], 1u);
    if ((long long)k >= D.jobCap) return NO_ROOM;
    D.jobs[k] = j; D.jinfo[k] = info;
    return (int)k;
}
__device__ inline const bbmsa_result &fill_result(const Dev &D, int job) {
    return (job & GAPPED_BIT) ? D.gresults[job & ~GAPPED_BIT] : D.results[job];
}
// the tail of scoreSlow's loop body (BBMapThread.java:361-381); job < 0: no (successful) fill
__device__ void finish_site(const Dev &D, SlowState &st, Site &ss, int job, const uint8_t *bases, int len, int maxSw) {
    if (job >= 0) {
        const bbmsa_result &res = fill_result(D, job);
        set_slow_score(ss, res.score[0]); set_limits(ss, res.score[1], res.score[2]); ss.match_job = job;
    }
    ss.reserved[0] = ss.reserved[1] = 0;
    ss.score = ss.slowScore;
    st.minMsaLimit = imax(st.minMsaLimit, ss.slowScore - D.S.clearzone3);
    ss.perfect = (ss.slowScore == maxSw);
    if (ss.perfect) ss.semiperfect = 1;
    else if (!ss.semiperfect) set_perfect(D.S, ss, bases, len, D.chromArr[ss.chrom], D.chromArrLen[ss.chrom]);
}

// scoreSlow's per-site opening (BBMapThread.java:278-303): a site whose span differs from the read length loses its ungapped
// score and flags; an over-long expected window is cut.  Depends on nothing but the site itself, so it gives the same answer
// whether it is evaluated ahead of time (on a copy) or when the loop reaches the site.
__device__ inline int prepare_site(const Settings &S, Site &ss, int len, int &expectedLen, bool &needsFill) {
    if (ss.stop - ss.start != len - 1) { set_slow_score(ss, 0); ss.semiperfect = 0; ss.perfect = 0; }
    const int sw = ss.slowScore;
    needsFill = sw < max_imperfect(S, len) && !ss.semiperfect;
    expectedLen = 0;
    if (needsFill) {
        expectedLen = calc_gref_len(ss);
        if (expectedLen >= S.expLimit) set_stop(ss, ss.start + imin(len + 40, S.expLimit));
    }
    return sw;
}
__device__ inline bbmap_jobinfo &job_info(const Dev &D, int job) { return (job & GAPPED_BIT) ? D.ginfo[job & ~GAPPED_BIT] : D.jinfo[job]; }

// One round: every active read consumes the result of its fill in flight and moves on to its next fill (or finishes).
// activeIn == nullptr: every read of the batch (round 1), in the class lists' order when there are lists.
//
// Fills ahead of time.  Strictly one fill per read and round would make a read with m candidate sites take m rounds, and a
// round costs the latency of a whole DP launch sequence however few jobs it holds.  A site's fill depends on the sites before
// it through ONE number, the running minMsaLimit = max(initial, best slowScore so far - CLEARZONE3) (:376), and once a read's
// first site is done that number rarely moves (the list is sorted by score, best first).  So while site idx >= 1 is in
// flight, the sites behind it are filled too, with the limit as it stands (Site.reserved[0] = 1 + job, reserved[1] = the
// minScore used).  When the loop reaches such a site it recomputes the minScore the reference would use: equal -> the finished
// fill IS the reference's fill and is adopted (numbered in the read's sequence at that moment); different -> it is dropped
// (its log entry keeps seq = -1) and the site is filled again.  Results are those of the sequential loop in every case.
// (five waves per SIMD, as before the byte loops had chunks)
#ifndef SLOW_ROUND_MIN_WAVES
#define SLOW_ROUND_MIN_WAVES 5
#endif
__global__ __launch_bounds__(128, SLOW_ROUND_MIN_WAVES) void slow_round_kernel(const Dev D) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long count = D.activeIn ? D.nActiveIn : D.nreads;
    bool stillActive = false;
    long long r = -1;
    if (t < count) r = D.activeIn ? D.activeIn[t] : (D.classList ? class_read(D, t) : t);
    if (r >= 0) {
        SlowState st = D.slow[r];
        if (st.phase != 3) {
            const bbidx_read rr = D.reads[r];
            const int len = rr.len, maxSw = max_quality(D.S, len);
            const int n = D.mcount[r];
            Site *s = D.ms + r * D.cap;
            while (st.idx < n) {
                Site ss = s[st.idx];
                const uint8_t *bases = D.bases + rr.bases_off + (ss.strand ? D.minusDelta : 0);
                if (st.phase == 1) {                                               // first fill came back (:312-335)
                    const bbmsa_result &res = fill_result(D, st.pending);
                    const int nsc = res.score_len;
                    if (nsc > 6 && (res.score[3] + res.score[4] + st.expectedLen < D.S.expLimit)) {
                        set_limits(ss, ss.start - res.score[6], ss.stop + res.score[7]);
                        const int job = emit_fill(D, r, rr, ss, st.idx, D.S.slowAlignPadding + D.S.extraPadding, st.minscore, 1, st.seq);
                        stillActive = true;
                        if (job == NO_ROOM) break;                                     // log full: the same step again next round
                        st.seq++; st.oldJob = st.pending; st.pending = job;
                        atomicAdd(&D.counters[CNT_REFILLS], 1u);
                        st.phase = 2; s[st.idx] = ss;
                        break;
                    }
                    finish_site(D, st, ss, nsc > 0 ? st.pending : -1, bases, len, maxSw);
                    s[st.idx] = ss; st.idx++; st.phase = 0;
                    continue;
                }
                if (st.phase == 2) {                                               // the wider refill came back: keep the better one
                    const bbmsa_result &res = fill_result(D, st.pending), &old = fill_result(D, st.oldJob);
                    const int job = (res.score_len == 0 || res.score[0] < old.score[0]) ? st.oldJob : st.pending;
                    finish_site(D, st, ss, job, bases, len, maxSw);
                    s[st.idx] = ss; st.idx++; st.phase = 0;
                    continue;
                }
                // phase 0: look at site idx (:267-309)
                bool needsFill;
                const int early = ss.reserved[0], earlyMin = ss.reserved[1];
                const int sw = prepare_site(D.S, ss, len, st.expectedLen, needsFill);
                if (needsFill) {
                    st.minscore = imax(sw, st.minMsaLimit);
                    if (early && earlyMin == st.minscore) {                        // filled ahead of time with the very same bound: adopt
                        st.pending = early - 1;
                        bbmap_jobinfo &ji = job_info(D, st.pending);
                        ji.seq = st.seq++; ji.site = st.idx;
                        st.phase = 1; s[st.idx] = ss;
                        continue;                                                  // its result is there already
                    }
                    const int job = emit_fill(D, r, rr, ss, st.idx, D.S.slowAlignPadding, st.minscore, 0, st.seq);
                    stillActive = true;
                    if (job == NO_ROOM) break;                                         // log full: this site again next round
                    if (early) atomicAdd(&D.counters[CNT_FILLS_DROPPED], 1u);                      // a fill ahead of time that the sequence does not contain
                    st.seq++; st.pending = job;
                    st.phase = 1; s[st.idx] = ss;
                    break;
                }
                if (early) atomicAdd(&D.counters[CNT_FILLS_DROPPED], 1u);
                finish_site(D, st, ss, -1, bases, len, maxSw);
                s[st.idx] = ss; st.idx++;
            }
            if (!stillActive) st.phase = 3;
            else if (st.idx >= 1 && D.fillAhead && (st.phase == 1 || st.phase == 2)) {
                for (int j = st.idx + 1; j < n; j++) {
                    Site tmp = s[j];
                    bool needsFill; int expectedLen;
                    const int sw = prepare_site(D.S, tmp, len, expectedLen, needsFill);
                    if (!needsFill) continue;
                    const int minscore = imax(sw, st.minMsaLimit);
                    if (tmp.reserved[0] && tmp.reserved[1] == minscore) continue;  // already in the log with this bound
                    const int job = emit_fill(D, r, rr, tmp, j, D.S.slowAlignPadding, minscore, 0, -1);
                    if (job == NO_ROOM) break;                                         // no room for fills ahead of time this round
                    if (tmp.reserved[0]) atomicAdd(&D.counters[CNT_FILLS_DROPPED], 1u);
                    s[j].reserved[0] = job + 1; s[j].reserved[1] = minscore;
                }
            }
            D.slow[r] = st;
        }
    }
    // next round's read list: one reservation per wavefront
    const unsigned long long m = __ballot(stillActive);
    if (m) {
        const int lane = threadIdx.x & 63;
        unsigned base = 0;
        if (lane == __builtin_ctzll(m)) base = atomicAdd(&D.counters[CNT_NEXT_ACTIVE], (unsigned)__builtin_popcountll(m));
        base = __shfl(base, __builtin_ctzll(m));
        if (stillActive) D.activeOut[base + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (int)r;
    }
}

// ---------------------------------------------------------------------------------------------- stage 4: after scoreSlow
// Tools.mergeDuplicateSites (+ Collections.sort for single-ended reads, BBMapThread.java:483-489 / :1042, :1058)
__global__ __launch_bounds__(128) void finish_kernel(const Dev D) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= D.nreads) return;
    int n = D.mcount[r];
    if (n <= 0) return;
    Site *s = D.ms + r * D.cap;
    n = merge_duplicate_sites(s, n);
    if (!D.S.paired) sort_sites<false>(s, n);
    D.mcount[r] = n;
}

// ---------------------------------------------------------------------------------------------- stage 5: rescue
// processReadPair :1065-1095 + rescue() up to the quickRescue call (AbstractMapThread.java:1144-1220).  One thread per pair.
__global__ __launch_bounds__(128) void rescue_plan_kernel(const Dev D) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * p + 1 >= D.nreads) return;
    PairResc pr = D.pres[p];
    pr.first = 0; pr.count = 0; pr.ran = 0;
    const long long ra = 2 * p + D.pass, rl = 2 * p + (1 - D.pass);             // anchor read, loose read
    int na = D.mcount[ra], nl = D.mcount[rl];
    if (na < 0 || nl < 0) { D.pres[p] = pr; return; }                            // overflowed pair
    Site *sa = D.ms + ra * D.cap;
    const Site *sl = D.ms + rl * D.cap;
    int unpairedA;
    if (D.pass == 0) {
        int u1 = 0, u2 = 0;
        for (int i = 0; i < na; i++) if (sa[i].pairedScore == 0) u1++;
        for (int i = 0; i < nl; i++) if (sl[i].pairedScore == 0) u2++;
        pr.unpaired2 = u2; unpairedA = u1;
    } else unpairedA = pr.unpaired2;
    if (!(unpairedA > 0 && na > 0)) { D.pres[p] = pr; return; }
    pr.ran = 1;
    const int lenA = D.reads[ra].len, L = D.reads[rl].len;
    sort_sites<false>(sa, na);
    na = remove_low_quality_paired(sa, na, max_quality(D.S, lenA), D.S.ratioPreRescue, D.S.ratioPreRescue);
    D.mcount[ra] = na;
    const int searchDist = imin(D.S.maxPairDist, 2 * D.S.averagePairDist + 100);
    if (D.S.rescueSkip || searchDist > D.S.maxRescueDist || na == 0) { D.pres[p] = pr; return; }        // :1146-1151
    const int maxLooseSw = max_quality(D.S, L), maxAnchorSw = max_quality(D.S, lenA), maxImp = max_imperfect(D.S, L);
    const int bestLoose = nl == 0 ? 0 : sl[0].slowScore, bestAnchor = sa[0].slowScore;
    if (bestLoose == maxLooseSw && bestAnchor == maxAnchorSw && sa[0].pairedScore > 0) { D.pres[p] = pr; return; }
    const int rescueScoreLimit = (int)__fmul_rn(0.95f, (float)bestAnchor);
    pr.retainLimit = imax((int)__fmul_rn(0.68f, (float)bestLoose), (int)__fmul_rn(0.4f, (float)maxLooseSw));
    pr.retainLimit2 = imax((int)__fmul_rn(0.95f, (float)bestLoose), (int)__fmul_rn(0.55f, (float)maxLooseSw));
    pr.maxMismatches = bestLoose > maxImp ? 5 : imin(D.S.maxRescueMismatches, (int)__fsub_rn(__fmul_rn(0.60f, (float)L), 1.0f));
    pr.findTip = (D.S.tipSearchDist > 0 && bestLoose < maxImp) ? 1 : 0;
    int cnt = 0;
    for (int i = 0; i < na; i++) { if (sa[i].slowScore < rescueScoreLimit) break; if (sa[i].pairedScore == 0 && !sa[i].rescued) cnt++; }
    if (cnt == 0) { D.pres[p] = pr; return; }
    const unsigned first = atomicAdd(&D.counters[CNT_RESCUE_SEARCHES], (unsigned)cnt);
    pr.first = (int)first; pr.count = cnt;
    if ((long long)first + cnt <= D.rescCap) {
        const bbidx_read rrl = D.reads[rl];
        int k = 0;
        for (int i = 0; i < na; i++) {
            const Site &ssa = sa[i];
            if (ssa.slowScore < rescueScoreLimit) break;
            if (!(ssa.pairedScore == 0 && !ssa.rescued)) continue;
            const int searchIntoAnchor = ssa.stop - ssa.start - 1 + (lenA * 11 / 16);
            const int strand = ssa.strand ^ 1;
            bbresc_job j;
            j.read_off = rrl.bases_off + (strand ? D.minusDelta : 0);              // the loose read on the strand to search
            j.read_len = L; j.chrom = ssa.chrom;
            if (ssa.strand == 0) { j.loc = ssa.stop - searchIntoAnchor; j.idealStart = ssa.stop + D.S.averagePairDist; }
            else { j.loc = ssa.start + searchIntoAnchor; j.idealStart = ssa.start - D.S.averagePairDist; }
            j.searchDist = searchDist + searchIntoAnchor; j.maxAllowedMismatches = pr.maxMismatches;
            j.flags = strand == 1 ? 1 : 0; j.reserved = 0;
            D.rjobs[first + k] = j;
            RescInfo ri; ri.pair = (int)p; ri.anchorSite = i; ri.strand = strand; ri.job = -1;
            D.rinfo[first + k] = ri;
            k++;
        }
    }
    D.pres[p] = pr;
}

// rescue()'s body after quickRescue + slowRescue up to its fill (AbstractMapThread.java:1222-1226, :1246-1265).  One thread per
// pair, its searches in anchor order (a read's fills are numbered in the order the reference issues them).
template <bool KARG> __global__ __launch_bounds__(128, 5) void rescue_prep_kernel(const Dev Darg) {
    const Dev &D = dev_of<KARG>(Darg);
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * p + 1 >= D.nreads) return;
    const PairResc pr = D.pres[p];
    if (pr.count == 0 || (long long)pr.first + pr.count > D.rescCap) return;
    const long long rl = 2 * p + (1 - D.pass);
    const bbidx_read rrl = D.reads[rl];
    const int L = rrl.len, maxImp = max_imperfect(D.S, L), maxScore = max_quality(D.S, L);
    int seq = D.slow[rl].seq;
    for (int k = 0; k < pr.count; k++) {
        const long long q = pr.first + k;
        RescInfo ri = D.rinfo[q];
        const bbresc_result res = D.rres[q];
        const bbresc_job rj = D.rjobs[q];
        Site ss;
        ss.chrom = rj.chrom; ss.strand = ri.strand; ss.start = res.start; ss.stop = res.stop; ss.hits = 0;
        ss.quickScore = ss.score = res.score; ss.slowScore = 0; ss.pairedScore = 0;
        ss.perfect = res.perfect; ss.semiperfect = res.semiperfect; ss.rescued = 1; ss.ngaps = 0;
        for (int i = 0; i < BBMSA_MAX_GAPS; i++) ss.gaps[i] = 0;
        ss.match_job = -1; ss.reserved[0] = 0; ss.reserved[1] = 0;
        ri.job = -1;
        const int reflen = D.chromArrLen[rj.chrom];
        // reserved[0]: 0 = dropped, 1 = slowRescue finished without a fill, 2 = fill in flight; reserved[1] = ungapped score
        if (res.found == 1 && ss.start >= 0 && ss.stop <= reflen - 1 && res.mismatches <= pr.maxMismatches) {
            const uint8_t *bases = D.bases + rj.read_off;
            const uint8_t *ref = D.chromArr[rj.chrom];
            int sw = score_no_indels(D.S, bases, L, ref, reflen, ss.start);
            if (sw < maxImp && D.S.maxIndel > 0) {
                set_slow_score(ss, sw);
                if (pr.findTip && find_tip_deletions(D.S, ss, bases, L, ref, reflen, maxImp, true, true)) sw = score_no_indels(D.S, bases, L, ref, reflen, ss.start);
                const int minMsaLimit = -D.S.clearzone1e + (int)__fmul_rn(D.S.ratioPaired, (float)maxScore);
                ri.job = emit_fill(D, rl, rrl, ss, -1, D.S.slowRescuePadding, imax(sw, minMsaLimit), 2, seq++);
                atomicAdd(&D.counters[CNT_RESCUE_FILLS], 1u);
                ss.reserved[0] = 2; ss.reserved[1] = sw;
            } else {
                set_slow_score(ss, sw); ss.score = ss.slowScore; set_stop(ss, ss.start + L - 1);
                ss.reserved[0] = 1; ss.reserved[1] = sw;
            }
        }
        D.rsite[q] = ss;
        D.rinfo[q] = ri;
    }
    D.slow[rl].seq = seq;
}

// slowRescue's tail (:1267-1305), rescue()'s retain / pair logic (:1227-1236) and mergeDuplicateSites of the loose list
// (BBMapThread.java:1087 / :1094).  One thread per pair.
__global__ __launch_bounds__(128) void rescue_finish_kernel(const Dev D) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * p + 1 >= D.nreads) return;
    const PairResc pr = D.pres[p];
    if (!pr.ran) return;
    const long long ra = 2 * p + D.pass, rl = 2 * p + (1 - D.pass);
    Site *sa = D.ms + ra * D.cap, *sl = D.ms + rl * D.cap;
    int nl = D.mcount[rl];
    const int nsearch = ((long long)pr.first + pr.count > D.rescCap) ? 0 : pr.count;
    const bbidx_read rrl = D.reads[rl];
    const int L = rrl.len, maxScore = max_quality(D.S, L);
    bool overflow = false;
    for (int k = 0; k < nsearch; k++) {
        const long long q = pr.first + k;
        Site ss = D.rsite[q];
        if (ss.reserved[0] == 0) continue;
        const RescInfo ri = D.rinfo[q];
        const uint8_t *bases = D.bases + D.rjobs[q].read_off;
        const uint8_t *ref = D.chromArr[ss.chrom]; const int reflen = D.chromArrLen[ss.chrom];
        if (ss.reserved[0] == 2) {
            const bbmsa_result &res = fill_result(D, ri.job);
            if (res.score_len > 0) { set_slow_score(ss, res.score[0]); ss.score = ss.slowScore; set_start(ss, res.score[1]); set_stop(ss, res.score[2]); ss.match_job = ri.job; }
            else { const int oldStart = D.rres[q].start; set_slow_score(ss, ss.reserved[1]); ss.score = ss.slowScore; set_start(ss, oldStart); set_stop(ss, ss.start + L - 1); }
        }
        ss.reserved[0] = ss.reserved[1] = 0;
        ss.pairedScore = ss.score + 1;
        ss.perfect = (ss.slowScore == maxScore);
        if (ss.perfect) ss.semiperfect = 1; else set_perfect(D.S, ss, bases, L, ref, reflen);
        if (ss.score > pr.retainLimit && ss.start >= 0 && ss.stop <= reflen - 1) {
            Site &ssa = sa[ri.anchorSite];
            if (ss.score > pr.retainLimit2) {
                ss.pairedScore = imax(ss.pairedScore, ss.slowScore + ssa.slowScore / 4);
                ssa.pairedScore = imax(ssa.pairedScore, ssa.slowScore + ss.slowScore / 4);
            }
            if (nl < D.cap) sl[nl++] = ss; else overflow = true;
        }
    }
    if (overflow) { atomicAdd(&D.counters[CNT_OVERFLOWED], 1u); D.mcount[rl] = -1; return; }
    D.mcount[rl] = merge_duplicate_sites(sl, nl);
}

#include "mapper_final.h"

// both builds of the kernels that come in two (the host picks one per context, DEV_KERNEL)
#define DEV_KERNEL_BUILDS(name) template __global__ void name<false>(const Dev); template __global__ void name<true>(const Dev);
DEV_KERNEL_BUILDS(score_kernel) DEV_KERNEL_BUILDS(rescue_prep_kernel) DEV_KERNEL_BUILDS(final_round_kernel)
#undef DEV_KERNEL_BUILDS

// ---------------------------------------------------------------------------------------------- reads the probe leaves alone
// The probe writes the reverse complement of the reads it probes.  A read shorter than k or without a key is not probed (quickMap's
// `basesP.length < KEYLEN` return, current/align2/AbstractMapThread.java:646), but its mate may anchor a rescue that searches for it
// on either strand (basesM1 / basesM2 exist for every read, :501-503).  One thread per read: such reads are few and, as a rule, short.
__global__ __launch_bounds__(128) void revcomp_unprobed_kernel(const bbidx_read *reads, long long n, int k, const uint8_t *in, uint8_t *out) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const bbidx_read rr = reads[r];
    if (rr.nkeys >= 1 && rr.len >= k) return;
    for (int i = 0; i < rr.len; i++) out[rr.bases_off + i] = (uint8_t)bbidx::complement_extended(in[rr.bases_off + rr.len - 1 - i]);
}

// ---------------------------------------------------------------------------------------------- overflow tier
// units (reads, or pairs in paired mode) whose site list did not fit: appended in any order, sorted on the host
__global__ __launch_bounds__(128) void collect_overflow_kernel(const int *mcount, long long nunits, int paired, int *ids, unsigned *count) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nunits) return;
    const bool over = paired ? (mcount[2 * u] < 0 || mcount[2 * u + 1] < 0) : mcount[u] < 0;
    if (over) ids[atomicAdd(count, 1u)] = (int)u;
}
__global__ __launch_bounds__(128) void gather_reads_kernel(const bbidx_read *reads, const int *ids, int nunits, int paired, bbidx_read *sub, int *readIds) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nunits) return;
    if (paired) {
        const int r = 2 * ids[i];
        sub[2 * i] = reads[r]; sub[2 * i + 1] = reads[r + 1]; readIds[2 * i] = r; readIds[2 * i + 1] = r + 1;
    } else { sub[i] = reads[ids[i]]; readIds[i] = ids[i]; }
}
// a read the tier mapped is marked in the main list (BBMAP_NSITES_IN_TIER); counts the reads that had overflowed and now have a list
__global__ __launch_bounds__(128) void mark_tier_kernel(int *mcount, const int *tierCount, const int *readIds, int n, unsigned *resolved) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || tierCount[i] < 0) return;
    const int r = readIds[i];
    if (mcount[r] == -1) atomicAdd(resolved, 1u);
    mcount[r] = BBMAP_NSITES_IN_TIER;
}

// ---------------------------------------------------------------------------------------------- packed output
__global__ __launch_bounds__(256) void pack_counts_kernel(const int *mcount, long long n, int *counts) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) { const int m = mcount[r]; counts[r] = m > 0 ? m : 0; }
}
// one 16-byte piece of a 128-byte site record per thread: eight consecutive lanes move one record
__global__ __launch_bounds__(256) void pack_sites_kernel(const Site *ms, const int *mcount, const long long *offsets, long long n, int cap, long long packedCap, Site *packed) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long slot = t >> 3; const int piece = (int)(t & 7);
    const long long r = slot / cap; const int j = (int)(slot - r * cap);
    if (r >= n || j >= mcount[r]) return;
    const long long dst = offsets[r] + j;
    if (dst >= packedCap) return;
    ((uint4 *)(packed + dst))[piece] = ((const uint4 *)(ms + r * cap + j))[piece];
}


// ---------------------------------------------------------------------------------------------- scaffold coordinates (on demand)
// SamLine's coordinate block (current/stream/SamLine.java:120-187) over the final records, bbmap_get_scaffold_records.  One
// wavefront per read, or per pair (the mates unpair each other); every value below is wave-uniform.
struct ScafMate { int mapped, single, gscaf, a1, b1, scaflen, pos0, pos1; };

__device__ ScafMate scaf_mate(const bbscaf::Table &T, const bbmap_final &f, const uint8_t *m) {
    const int lane = threadIdx.x & 63;
    ScafMate o;
    o.mapped = f.mapped != 0; o.single = 1; o.gscaf = -1; o.a1 = o.b1 = o.scaflen = o.pos0 = o.pos1 = 0;
    const int chrom = f.chrom;
    if (!o.mapped || chrom < 1 || chrom > T.nchroms) { o.mapped = 0; return o; }
    const int start = f.start, stop = f.stop;
    const int b = T.off[chrom], n = T.off[chrom + 1] - b;
    const int *a = T.loc + b;
    if (n >= 2) {                                           // Data.isSingleScaffold (Data.java:1112-1140)
        const int scaf = bbscaf::wave_last_at_or_below(a, n, start + T.pad);
        if (scaf != n - 1) {
            const int lowerBound = a[scaf] - T.pad, upperBound = a[scaf + 1];
            o.single = !(stop < lowerBound || start > upperBound) && stop < upperBound;
        }
    }
    if (!o.single) { o.mapped = 0; return o; }              // :134-140 / :154-160: r.setMapped(false)
    const int idx = n < 2 ? 0 : bbscaf::wave_last_at_or_below(a, n, (start + stop) / 2 + T.pad / 2);    // Data.scaffoldIndex
    o.gscaf = b + idx; o.scaflen = T.len[b + idx];
    o.a1 = start - a[idx];                                  // scaffoldRelativeLoc
    o.b1 = o.a1 - start + stop;
    // the match string is in long format (one symbol per column, no digits), 64 symbols per ballot
    const int ml = f.match_len > 0 ? f.match_len : 0;
    int clip = 0, tclip = 0, clippedIndels = 0;
    if (ml > 0 && m[0] == 'C') {                            // countLeadingClip (:924-945)
        for (int base = 0; base < ml; base += 64) {
            const int i = base + lane;
            const unsigned long long x = __ballot(i < ml && m[i] != 'C');
            if (x) { clip += __builtin_ctzll(x); break; }
            clip += min(64, ml - base);
        }
    }
    for (int end = ml; end > 0; end -= 64) {                // countTrailingClip (:959-972)
        const int i = end - 1 - lane;
        const unsigned long long x = __ballot(i >= 0 && m[i] != 'C');
        if (x) { tclip += __builtin_ctzll(x); break; }
        tclip += min(64, end);
    }
    if (o.a1 < 0) {                                         // countLeadingIndels (:975-996): walk until rloc reaches 0
        int rloc = o.a1, dels = 0, inss = 0;
        for (int base = 0; base < ml && rloc < 0; base += 64) {
            const int i = base + lane;
            const bool v = i < ml;
            const uint8_t ch = v ? m[i] : 0;
            const unsigned long long adv = __ballot(v && ch != 'I');             // symbols that move rloc
            const bool inc = v && __popcll(adv & ((1ull << lane) - 1)) < -rloc;  // rloc < 0 still holds when the loop reaches it
            dels += __popcll(__ballot(inc && ch == 'D'));
            inss += __popcll(__ballot(inc && ch == 'I'));
            rloc += __popcll(__ballot(inc && ch != 'I'));
        }
        clippedIndels = dels - inss;
    }
    // countTrailingIndels(b1, scaflen, match) (:999-1020) returns 0 whenever b1 >= 0, and for b1 < 0 its loop condition
    // rloc >= rlen is false at once: it is 0 for every record.
    o.pos0 = (o.a1 + 1) + clip + clippedIndels;
    o.pos1 = (o.b1 + 1) - tclip;
    if (o.pos1 > o.scaflen) o.pos1 = o.scaflen;
    if (o.pos0 < 1) o.pos0 = 1;
    return o;
}

__device__ inline void put_scafrec(bbmap_scafrec *out, const ScafMate &q, int paired, int sameScaf) {
    bbmap_scafrec w;
    w.scaffold = q.mapped ? q.gscaf : -1;
    w.start = q.a1; w.stop = q.b1; w.pos = q.pos0; w.end = q.pos1; w.scaflen = q.scaflen;
    const int inbounds = q.mapped && q.a1 >= 0 && q.b1 < q.scaflen;         // :267-268
    w.flags = (q.mapped ? BBMAP_SCAF_MAPPED : 0) | (paired ? BBMAP_SCAF_PAIRED : 0) | (inbounds ? BBMAP_SCAF_INBOUNDS : 0) |
              (sameScaf ? BBMAP_SCAF_SAME_SCAFFOLD : 0);
    w.reserved = 0;
    *out = w;
}

__global__ __launch_bounds__(256) void scaffold_coords_kernel(const bbscaf::Table T, const BatchView V, bbmap_scafrec *out) {
    const long long u = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (u >= (V.paired ? V.n / 2 : V.n)) return;
    const bool lead = (threadIdx.x & 63) == 0;
    if (!V.paired) {
        const ReadRec R = record_of<TierRule::ByRecord>(V, u);
        const ScafMate q = scaf_mate(T, *R.f, R.m);
        if (lead) put_scafrec(out + u, q, R.f->paired != 0, 0);
        return;
    }
    const ReadRec R1 = record_of<TierRule::ByRecord>(V, 2 * u), R2 = record_of<TierRule::ByRecord>(V, 2 * u + 1);
    const ScafMate q1 = scaf_mate(T, *R1.f, R1.m), q2 = scaf_mate(T, *R2.f, R2.m);
    const bool both = q1.single && q2.single;               // a mate that spans two scaffolds unpairs the other (:137-138, :157-158)
    const int same = q1.mapped && q2.mapped && q1.gscaf == q2.gscaf;       // sameScaf (:160): idx1 == idx2 on the same chromosome
    if (lead) {
        put_scafrec(out + 2 * u, q1, both && R1.f->paired != 0, same);
        put_scafrec(out + 2 * u + 1, q2, both && R2.f->paired != 0, same);
    }
}
__global__ __launch_bounds__(256) void tier_index_kernel(const int *ids, long long n, long long nreads, int *tierIdx) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = ids[i];
    if (r >= 0 && r < nreads) tierIdx[r] = (int)i;
}

}  // namespace bbmapper
