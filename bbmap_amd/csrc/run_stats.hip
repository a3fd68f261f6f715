// Run statistics on the device: AbstractMapThread.calcStatistics1 / calcStatistics2 (current/align2/AbstractMapThread.java:1478-1641,
// :1644-1770) with calcCorrectness (:2615-2689), Read.countErrors (current/stream/Read.java:2189-2240) and the insert-size histogram
// (AbstractMapThread.java:524, ReadStats.addToInsertHistogram current/align2/ReadStats.java:578-592, Read.insertSizeMapped
// current/stream/Read.java:2618-2670) -- the counters behind the table BBMap prints at the end of a run.
//
// One wavefront per read on a persistent grid, every control value wave-uniform.  The match string is consumed 64 symbols per step and
// the site list 64 sites per step, both with ballots and popcounts; the carries from one step to the next (previous score, groups so
// far, first correct site) are scalars.  Mate 1's wavefront also does the pair-level part of calcStatistics1 and takes what it needs
// of mate 2 (mapped, start, stop, strand, chrom, length) from mate 2's record.  What a read adds to the counters is laid out one
// counter per lane and added to the wave's own row of LDS accumulators (64-bit; about 80 wave-uniform 64-bit values do not fit the SGPR
// file, and in LDS they cannot be spilled); a block adds its four rows to the global counters once, at its end, with one 64-bit atomic
// per counter that moved.  The histogram is device atomics into its HBM array.  Everything is an integer: the result does not depend
// on the order of the adds.
//
// Fixed at the reference's defaults: AMBIGUOUS_TOSS = false, OUTPUT_PAIRED_ONLY = false, SAME_STRAND_PAIRS = false and
// REQUIRE_CORRECT_STRANDS_PAIRS = true (the histogram's ignoreStrand is false), MIN_PAIR_DIST = -160.  The splice counter
// (countErrors' errors[5], readCountSplice) is left out: SamLine.INTRON_LIMIT stays at Integer.MAX_VALUE, so no run of `D` ever has that
// length and the counter cannot move.  perfectHit and lowQualityReadsDiscarded need quickMap's return value (maxPossibleQuickScore),
// which the mapper does not keep: they stay with the host, and an unmapped read always counts as noHit.
#include "run_stats.h"

#include <climits>

#include "host_common.h"
#include "insert_size.h"
#include "wave_prims.h"

namespace bbrunstats {
using wavep::u64;
using wavep::lt_mask;
using wavep::popc;
using wavep::uni;

constexpr int MIN_PAIR_DIST = -160;                         // AbstractMapThread.java:2974
constexpr int MAXINSERTLEN = BBMAP_INSERT_HIST_BINS - 1;    // ReadStats.java:1313

// per-mate counters, in bbmap_runstats' order
enum { C_mappedRetained, C_mappedRetainedBases, C_ambiguousBestAlignment, C_ambiguousBestAlignmentBases, C_matchCountM, C_matchCountS,
       C_matchCountD, C_matchCountI, C_matchCountN, C_readCountS, C_readCountD, C_readCountI, C_readCountN, C_readCountE, C_rescuedP,
       C_rescuedM, C_perfectMatch, C_perfectMatchBases, C_perfectHitCount, C_semiPerfectHitCount, C_semiperfectMatch,
       C_semiperfectMatchBases, C_siteSum, C_topSiteSum, C_uniqueHit, C_noHit, C_firstSiteCorrectP, C_firstSiteCorrectM,
       C_firstSiteCorrectPaired, C_firstSiteCorrectSolo, C_firstSiteCorrectRescued, C_firstSiteIncorrect, C_firstSiteCorrectLoose,
       C_firstSiteIncorrectLoose, C_truePositiveP, C_truePositiveM, C_totalCorrectSites, C_correctUniqueHit, C_correctMultiHit,
       C_correctLowHit, C_falsePositive, C_readsUsed, C_basesUsed, C_PER_MATE };
static_assert(C_PER_MATE == PER_MATE, "per-mate counters");
// pair-level counters, as lanes PER_MATE.. of mate 1's wavefront
enum { P_bothUnmapped = PER_MATE, P_bothUnmappedBases, P_numMated, P_numMatedBases, P_badPairs, P_badPairBases, P_innerLengthSum,
       P_outerLengthSum, P_insertSizeSum, P_END };
static_assert(P_END - PER_MATE == PAIR_LEVEL, "pair-level counters");

// Read.countErrors {M, S, D, I, N}: `X`, `Y` and `I` all count as insertions, `C` counts with `N`
struct Errors { int m, s, d, i, n; };
__device__ inline Errors count_errors(const uint8_t *m, int ml, int lane) {
    Errors E = {0, 0, 0, 0, 0};
    for (int base = 0; base < ml; base += 64) {
        const int ch = base + lane < ml ? m[base + lane] : 0;
        E.m += popc(__ballot(ch == 'm'));
        E.s += popc(__ballot(ch == 'S'));
        E.d += popc(__ballot(ch == 'D'));
        E.i += popc(__ballot(ch == 'I' || ch == 'X' || ch == 'Y'));
        E.n += popc(__ballot(ch == 'N' || ch == 'C'));
    }
    return E;
}

__device__ inline int absdif(int a, int b) { return a > b ? a - b : b - a; }        // Tools.absdif

// calcCorrectness {correctGroup, sizeOfTopGroup, numCorrect, firstElementCorrect, firstElementCorrectLoose} and the perfect /
// semiperfect site counts of calcStatistics' own loop over r.sites (:1572-1582), in one pass over the list
struct Sites { int correctGroup, topGroup, numCorrect, firstCorrect, firstLoose, perfect, semiperfect; };
__device__ inline Sites walk_sites(const bbmap_msite *s, int n, const bbmap_truth *truth, int thresh, int lane) {
    Sites R = {-1, 0, 0, 0, 0, 0, 0};
    if (n <= 0) return R;
    // `original` is the truth record when the read has one, else site 0 (:2623-2627)
    const bool given = truth && truth->chrom >= 0;
    const int oc = given ? truth->chrom : s[0].chrom, os = given ? truth->strand : s[0].strand;
    const int oa = given ? truth->start : s[0].start, ob = given ? truth->stop : s[0].stop;
    const int score0 = s[0].score;
    int prevScore = INT_MAX, group = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool valid = i < n;
        const bbmap_msite *ss = s + (valid ? i : 0);
        const int score = ss->score;
        const bool same = valid && ss->chrom == oc && ss->strand == os;
        // (a lane past the list's end reads site 0 again; `same` keeps it out of every ballot.  absdif is int arithmetic and wraps for
        // coordinates further than 2^31 apart, as Tools.absdif(int, int) does)
        const int da = absdif(ss->start, oa), db = absdif(ss->stop, ob);
        const u64 correct = __ballot(same && da <= thresh && db <= thresh);                     // isCorrectHit (:2692-2700)
        const u64 loose = __ballot(same && (da <= thresh + 20 || db <= thresh + 20));           // isCorrectHitLoose (:2712-2719)
        R.perfect += popc(__ballot(valid && ss->perfect != 0));
        R.semiperfect += popc(__ballot(valid && ss->semiperfect != 0));
        R.topGroup += popc(__ballot(valid && score == score0));
        int before = __shfl_up(score, 1, 64);
        if (lane == 0) before = prevScore;
        const u64 changes = __ballot(valid && before != score);                                  // `if(prevScore!=ss.score)`: a group begins
        if (correct && R.correctGroup < 0) {
            const int fl = __builtin_ctzll(correct);
            R.correctGroup = group + popc(changes & (lt_mask(fl) | (1ull << fl)));               // score changes at or before it
        }
        if (base == 0) { R.firstCorrect = (int)(correct & 1); R.firstLoose = (int)(loose & 1); }
        R.numCorrect += popc(correct);
        group += popc(changes);
        prevScore = __shfl(score, min(63, n - base - 1), 64);
    }
    return R;
}

using bbinsert::Mate;                                      // Read.insertSizeMapped(r1, r2, false) for two mapped mates (insert_size.h)
using bbinsert::insert_size_mapped;

#define SET(k, v) mine = lane == (k) ? (long long)(v) : mine

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK) void run_stats_kernel(const Args A, u64 *counters, u64 *ihist) {
    __shared__ u64 acc[WAVES_PER_BLOCK][N_COUNTERS];
    const int lane = threadIdx.x & 63, wid = uni((int)(threadIdx.x >> 6));
    for (int k = lane; k < N_COUNTERS; k += 64) acc[wid][k] = 0;           // a wave touches its own row only, until the block's flush
    __syncthreads();
    const long long nwaves = (long long)gridDim.x * WAVES_PER_BLOCK;
    for (long long r = (long long)blockIdx.x * WAVES_PER_BLOCK + wid; r < A.V.n; r += nwaves) {
        const int mate = A.V.paired ? (int)(r & 1) : 0;
        const ReadRec R = record_of<TierRule::ByList, true>(A.V, r);         // one read as calcStatistics sees it, wave-uniform
        const bbmap_final &f = *R.f;
        const int len = A.V.reads[r].len, elements = R.n;                    // elements: r.sites
        const bool mapped = f.mapped != 0, paired = f.paired != 0, rescued = f.rescued != 0, plus = f.strand == 0;
        long long mine = 0;
        SET(C_readsUsed, 1); SET(C_basesUsed, len);
        if (f.ambiguous && mapped) { SET(C_ambiguousBestAlignment, 1); SET(C_ambiguousBestAlignmentBases, len); }      // :1484 / :1647
        if (elements > 0) {
            if (R.m) {                                                      // `if(r.match!=null)` (:1515 / :1667)
                const Errors E = count_errors(R.m, R.ml, lane);
                SET(C_matchCountM, E.m); SET(C_matchCountS, E.s); SET(C_matchCountD, E.d); SET(C_matchCountI, E.i); SET(C_matchCountN, E.n);
                SET(C_readCountS, E.s > 0); SET(C_readCountD, E.d > 0); SET(C_readCountI, E.i > 0); SET(C_readCountN, E.n > 0);
                SET(C_readCountE, E.s > 0 || E.d > 0 || E.i > 0);
            }
            const Sites T = walk_sites(R.s, elements, A.truth ? A.truth + r : nullptr, A.thresh, lane);
            SET(C_mappedRetained, 1); SET(C_mappedRetainedBases, len);
            if (rescued) { SET(C_rescuedP, plus); SET(C_rescuedM, !plus); }
            const int maxSw = A.ptsMatch + (len - 1) * A.ptsMatch2;         // maxSwScore = msa.maxQuality(len)
            if (f.perfect || (maxSw > 0 && R.s[0].slowScore == maxSw)) { SET(C_perfectMatch, 1); SET(C_perfectMatchBases, len); }      // :1565 / :1693
            SET(C_perfectHitCount, T.perfect); SET(C_semiPerfectHitCount, T.semiperfect);
            if (T.semiperfect > 0) { SET(C_semiperfectMatch, 1); SET(C_semiperfectMatchBases, len); }
            if (T.firstCorrect) {
                SET(C_firstSiteCorrectP, plus); SET(C_firstSiteCorrectM, !plus);
                SET(C_firstSiteCorrectPaired, paired); SET(C_firstSiteCorrectSolo, !paired);
                SET(C_firstSiteCorrectRescued, rescued);
            } else SET(C_firstSiteIncorrect, 1);
            SET(C_firstSiteCorrectLoose, T.firstLoose); SET(C_firstSiteIncorrectLoose, !T.firstLoose);
            SET(C_siteSum, elements); SET(C_topSiteSum, T.topGroup);
            SET(C_uniqueHit, T.topGroup == 1);
            if (T.correctGroup > 0) {
                SET(C_truePositiveP, plus); SET(C_truePositiveM, !plus);
                SET(C_totalCorrectSites, T.numCorrect);
                if (T.correctGroup == 1) { SET(C_correctUniqueHit, T.topGroup == 1); SET(C_correctMultiHit, T.topGroup != 1); }
                else SET(C_correctLowHit, 1);
            } else SET(C_falsePositive, 1);
        } else SET(C_noHit, 1);
        // the pair-level part of calcStatistics1: mate 1's wavefront, or every read of a single-ended run (r2 == null)
        if (mate == 0) {
            const bool hasMate = A.V.paired != 0;
            bool mateMapped = false;
            Mate m2 = {0, 0, 0, 0, 0};
            if (hasMate) {
                const ReadRec Q = record_of<TierRule::ByList>(A.V, r + 1);
                mateMapped = Q.f->mapped != 0;
                m2.strand = Q.f->strand; m2.start = Q.f->start; m2.stop = Q.f->stop; m2.chrom = Q.f->chrom; m2.len = A.V.reads[r + 1].len;
            }
            const int len2 = hasMate ? len : 0;                             // `len2=(r2==null ? 0 : r.length())` (:1481): mate 1's length
            if (!mapped && !mateMapped) {                                   // :1489-1496
                SET(P_bothUnmapped, hasMate ? 2 : 1); SET(P_bothUnmappedBases, len + (hasMate ? m2.len : 0));
            }
            if (elements > 0) {
                if (paired) {                                               // :1542-1559
                    int inner, outer;
                    if (f.start <= m2.start) { inner = m2.start - f.stop; outer = m2.stop - f.start; }
                    else { inner = f.start - m2.stop; outer = f.stop - m2.start; }
                    inner = min(A.maxPairDist, inner);
                    inner = max(MIN_PAIR_DIST, inner);
                    SET(P_numMated, 1); SET(P_numMatedBases, len + len2);
                    SET(P_innerLengthSum, inner); SET(P_outerLengthSum, outer); SET(P_insertSizeSum, inner + len + m2.len);
                } else if (hasMate && mateMapped) { SET(P_badPairs, 1); SET(P_badPairBases, len + len2); }
            }
            // AbstractMapThread.java:524 `if(MAKE_INSERT_HISTOGRAM && r.paired())` and ReadStats.addToInsertHistogram's own conditions
            if (ihist && hasMate && paired && mapped && mateMapped) {
                const Mate m1 = {f.strand, f.start, f.stop, f.chrom, len};
                const int x = min(MAXINSERTLEN, insert_size_mapped(m1, m2));
                if (x > 0 && lane == 0) atomicAdd(&ihist[x], 1ull);
            }
        }
        if (lane < P_END) acc[wid][lane < PER_MATE ? mate * PER_MATE + lane : PAIR_BASE + (lane - PER_MATE)] += (u64)mine;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < N_COUNTERS; k += blockDim.x) {
        u64 sum = 0;
        for (int w = 0; w < WAVES_PER_BLOCK; w++) sum += acc[w][k];
        if (sum) atomicAdd(&counters[k], sum);
    }
}
#undef SET

hipError_t launch(const Args &a, unsigned long long *counters, unsigned long long *ihist, hipStream_t stream) {
    if (a.V.n <= 0) return hipSuccess;
    const long long want = (a.V.n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const unsigned blocks = (unsigned)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    hipLaunchKernelGGL(run_stats_kernel, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, stream, a, counters, ihist);
    return hipGetLastError();
}

}  // namespace bbrunstats

// The raw form over arrays the caller owns (include/bbmap_amd.h).
extern "C" int bbpipe_run_stats_device(void *stream, int64_t n_reads, int32_t paired, int32_t scheme, int32_t thresh, const bbidx_read *reads,
                                       const bbmap_final *finals, const uint8_t *pool, const bbmap_msite *sites, const int32_t *nsites,
                                       int32_t cap, const bbmap_truth *truth, bbmap_runstats *counters, int64_t *ihist) {
    if (n_reads < 0 || (paired && (n_reads & 1)) || thresh < 0 || cap < 1 || cap > BBMAP_MAX_SITES_LIMIT ||
        (scheme != BBMSA_SCHEME_11TS && scheme != BBMSA_SCHEME_9PACBIO)) return bbfail(BBMAP_E_ARG, "bbpipe_run_stats_device: bad argument");
    if (n_reads == 0) return BBMAP_OK;
    if (!reads || !finals || !pool || !sites || !nsites || !counters) return bbfail(BBMAP_E_ARG, "bbpipe_run_stats_device: null buffer");
    bbrunstats::Args a = {};
    a.V.reads = reads; a.V.fin = finals; a.V.pool = pool; a.V.sites = sites; a.V.nsites = nsites; a.V.cap = cap;      // (no tier)
    a.truth = truth; a.V.n = n_reads; a.V.paired = paired ? 1 : 0;
    a.ptsMatch = scheme == BBMSA_SCHEME_9PACBIO ? 90 : 70; a.ptsMatch2 = 100;     // POINTS_MATCH / POINTS_MATCH2 of the two aligner classes
    a.thresh = thresh; a.maxPairDist = 32000;                                      // MAX_PAIR_DIST (AbstractMapThread.java:2975)
    BBHIP(bbrunstats::launch(a, (unsigned long long *)counters, (unsigned long long *)ihist, (hipStream_t)stream));
    return BBMAP_OK;
}
