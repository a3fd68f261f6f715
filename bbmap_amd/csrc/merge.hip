// The merge stage: BBMerge's ratio-mode overlap search (BBMerge.mateByOverlap_ratioMode, current/jgi/BBMerge.java:1615-1639, over the
// natives of jni/BBMergeOverlapper.c) and Read.joinRead's overlapped branch (current/stream/Read.java:2804-2840) over a batch of
// pairs.  Mate 2 comes as it was sequenced and is reverse-complemented while it is read.  The arithmetic is in merge_shared.h and is
// the same code for both forms; this file holds what differs: where a pair's bases and per-insert sums live and who computes them.
//
// Overlap kernel: one wavefront (one 64-thread workgroup) per pair.  Both mates go to LDS as (base, probCorrect[q]) columns, mate 2
// complemented and reversed on the way.  Lanes take inserts, 64 consecutive ones at a time, and one lane owns the whole column loop
// of its insert: consecutive lanes read consecutive LDS columns of one mate and the same column of the other (a broadcast).  The
// overlap length is a triangle over the inserts, but 64 neighbours have nearly the same length, so consecutive assignment wastes
// little (2 x 150, defaults: 485 wave steps for 340 steps' worth of columns); pairing long with short inserts per lane was not
// better at this granularity.  (good, bad, ratio) per insert go to LDS, and every lane then runs the two decision walks in step
// (the state is wave-uniform), visiting only the inserts a wave-wide test leaves (merge_shared.h: decide).  Lengths pick the
// kernel: pairs whose mates fit 192 bases run with 7.7 KB of LDS per wavefront, longer ones (up to 512) with 20.5 KB, so the usual
// short pairs keep about 20 wavefronts per CU; each pair is skipped by the launch of the other class.
// Join kernel: one wavefront per pair, one lane per output base; every position of joinRead's right-to-left loop is independent.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <mutex>
#include <vector>

#include "bbmap_amd.h"
#include "complement.h"
#include "host_common.h"
#include "merge_shared.h"

namespace bbmerge {

static const float h_probCorrect[MAX_QUALITY + 1] = {BBMERGE_PROB_CORRECT};
__device__ const float d_probCorrect[MAX_QUALITY + 1] = {BBMERGE_PROB_CORRECT};

constexpr int SHORT_LEN = 192;                 // the short class: both mates at most this long

struct Col { int base; float p; };
// a mate as column_sums reads it
struct Cols {
    const Col *c;
    __host__ __device__ int base(int i) const { return c[i].base; }
    __host__ __device__ float prob(int i) const { return c[i].p; }
};
// the per-insert triples as decide() reads them
struct Triples {
    const float *g, *b, *r;
    __host__ __device__ float good(int k) const { return g[k]; }
    __host__ __device__ float bad(int k) const { return b[k]; }
    __host__ __device__ float ratio(int k) const { return r[k]; }
};

struct HostWave {
    template <class F> LaneMask ballot(F f) const {
        LaneMask m = 0;
        for (int lane = 0; lane < 64; lane++) if (f(lane)) m |= 1ull << lane;
        return m;
    }
};
struct DeviceWave {
    template <class F> __device__ LaneMask ballot(F f) const { return __ballot(f((int)threadIdx.x)); }
};

static const bbmerge_rec SKIPPED = {-1, 0, 0, BBMERGE_INFO_SKIPPED};

template <int MAXLEN> struct PairLds {
    Col a[MAXLEN], b[MAXLEN];
    float good[2 * MAXLEN], bad[2 * MAXLEN], ratio[2 * MAXLEN];      // inserts 0 .. alen + blen - 4 at the most
};

// One native for the pair in LDS.  Called by the whole wavefront in uniform control flow.
template <bool Q, int MAXLEN> __device__ void search(PairLds<MAXLEN> &S, const Params &p, int alen, int blen, bbmerge_rec &r) {
    const Range range = insert_range(p, alen, blen);
    const Cols A{S.a}, B{S.b};
    __syncthreads();                            // the mates are in LDS; the previous form's walks have read its triples
    for (int k0 = 0; k0 <= range.hi - range.lo; k0 += 64) {
        const int k = k0 + (int)threadIdx.x;
        if (k <= range.hi - range.lo) {
            const Span s = span_of(range.hi - k, alen, blen);
            float good, bad;
            column_sums<Q>(A, B, s, p.gIncr, p.bIncr, good, bad);
            S.good[k] = good; S.bad[k] = bad; S.ratio[k] = ratio_of(bad, p.offset, s.len);
        }
    }
    __syncthreads();
    decide<Q>(DeviceWave(), Triples{S.good, S.bad, S.ratio}, p, range, alen, blen, r);
}

// Pairs whose longer mate has MINLEN < length <= MAXLEN; the launch with MAXLEN == BBMERGE_MAX_READ_LEN also reports longer pairs.
template <int MINLEN, int MAXLEN>
__global__ void __launch_bounds__(64) bbmerge_overlap_kernel(bbmerge_config cfg, const bbidx_read *reads1, const bbidx_read *reads2,
                                                             const uint8_t *bases, const uint8_t *quality, bbmerge_rec *recs) {
    __shared__ PairLds<MAXLEN> S;
    const long long pair = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const bbidx_read r1 = reads1[pair], r2 = reads2[pair];
    const int alen = imax(r1.len, 0), blen = imax(r2.len, 0);
    const int longer = imax(alen, blen);
    if (longer <= MINLEN) return;
    if (longer > MAXLEN) {
        if (MAXLEN == BBMERGE_MAX_READ_LEN && lane == 0) recs[pair] = bbmerge_rec{-1, 0, 0, BBMERGE_INFO_SKIPPED};
        return;
    }
    const bool quality_form = runs_quality_form(cfg, quality != nullptr);
    bool outside = false;
    for (int i = lane; i < alen; i += 64) {
        Col c;
        c.base = (int8_t)bases[r1.bases_off + i]; c.p = 0;
        if (quality_form) {
            const int q = quality[r1.bases_off + i];
            outside |= q > MAX_QUALITY;
            c.p = d_probCorrect[imin(q, MAX_QUALITY)];
        }
        S.a[i] = c;
    }
    for (int i = lane; i < blen; i += 64) {      // Read.reverseComplement: base i of b is the complement of mate 2's base blen - 1 - i
        Col c;
        c.base = (int8_t)bbpipe::complement_extended(bases[r2.bases_off + blen - 1 - i]); c.p = 0;
        if (quality_form) {
            const int q = quality[r2.bases_off + blen - 1 - i];
            outside |= q > MAX_QUALITY;
            c.p = d_probCorrect[imin(q, MAX_QUALITY)];
        }
        S.b[i] = c;
    }
    if (__any(outside)) {
        if (lane == 0) recs[pair] = bbmerge_rec{-1, 0, 0, BBMERGE_INFO_SKIPPED};
        return;
    }
    const Params p = params_of(cfg);
    bbmerge_rec r = {-1, 0, 0, 0};               // (rvector[4] = 0)
    if (quality_form) {
        search<true>(S, p, alen, blen, r);
        r.info |= BBMERGE_INFO_QUALITY;
    }
    if (runs_flat_form(cfg, quality_form, r)) {
        search<false>(S, p, alen, blen, r);
        r.info |= BBMERGE_INFO_FLAT;
    }
    if (lane == 0) recs[pair] = r;
}

// b's column j and its quality, from mate 2 as it was sequenced
template <class Bytes> __host__ __device__ inline void join_pair_column(const Bytes &bases, const Bytes &quality, bool with_quality, const bbidx_read &r1,
                                                                       const bbidx_read &r2, int alen, int blen, int insert, int i, int maxq,
                                                                       uint8_t &base, uint8_t &qual) {
    const int8_t ca = i < alen ? (int8_t)bases[r1.bases_off + i] : (int8_t)0;
    const int8_t qa = with_quality && i < alen ? (int8_t)quality[r1.bases_off + i] : (int8_t)0;
    const int j = blen - insert + i;
    int8_t cb = 0, qb = 0;
    if (j >= 0) {
        cb = (int8_t)bbpipe::complement_extended(bases[r2.bases_off + blen - 1 - j]);
        if (with_quality) qb = (int8_t)quality[r2.bases_off + blen - 1 - j];
    }
    join_column(with_quality, ca, qa, j >= 0, cb, qb, maxq, base, qual);
}

// the length joinRead's overlapped branch gives, 0 where it does not apply
__host__ __device__ inline int joined_length(int insert, int alen, int blen) { return insert > 0 && insert < alen + blen ? insert : 0; }

__global__ void __launch_bounds__(256) bbmerge_join_kernel(int maxq, long long n, const bbidx_read *reads1, const bbidx_read *reads2, const uint8_t *bases,
                                                           const uint8_t *quality, const int32_t *insert, bbidx_read *merged, uint8_t *out_bases,
                                                           uint8_t *out_quality) {
    const long long pair = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (pair >= n) return;
    const int lane = threadIdx.x & 63;
    const bbidx_read r1 = reads1[pair], r2 = reads2[pair];
    const int alen = imax(r1.len, 0), blen = imax(r2.len, 0);
    const int len = joined_length(insert[pair], alen, blen);
    const long long out = merged[pair].bases_off;
    for (int i = lane; i < len; i += 64) {
        uint8_t base, qual;
        join_pair_column(bases, quality, quality != nullptr, r1, r2, alen, blen, len, i, maxq, base, qual);
        out_bases[out + i] = base;
        if (quality) out_quality[out + i] = qual;
    }
    if (lane == 0) merged[pair].len = len;
}

static int check_config(const char *who, const bbmerge_config *cfg, int64_t n_pairs) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "%s: null config", who);
    if (n_pairs < 0 || n_pairs >= 0x7fffffff) return bbfail(BBMAP_E_ARG, "%s: bad pair count", who);
    if (!good_config(*cfg))
        return bbfail(BBMAP_E_ARG, "%s: bad config (no NaN, ratioMargin >= 1, gIncr and bIncr >= 0, minInsert0 and minInsert >= 0, maxMergeQuality 0..127)", who);
    return BBMAP_OK;
}

static int check_overlap_args(const char *who, const bbmerge_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                              const uint8_t *bases, const bbmerge_rec *recs) {
    BBTRY(check_config(who, cfg, n_pairs));
    if (n_pairs > 0 && (!reads1 || !reads2 || !bases || !recs)) return bbfail(BBMAP_E_ARG, "%s: null buffer", who);
    return BBMAP_OK;
}

static int check_join_args(const char *who, const bbmerge_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                           const uint8_t *bases, const uint8_t *quality, const int32_t *insert, const bbidx_read *merged, const uint8_t *out_bases,
                           const uint8_t *out_quality) {
    BBTRY(check_config(who, cfg, n_pairs));
    if (n_pairs > 0 && (!reads1 || !reads2 || !bases || !insert || !merged || !out_bases || (quality && !out_quality)))
        return bbfail(BBMAP_E_ARG, "%s: null buffer", who);
    return BBMAP_OK;
}

// once per process and device: the gfx950 check
static int prepare_device(const char *who) {
    static std::mutex mu;
    static bool ready[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;       // (a machine without a device: the check below says so)
    if (dev < 0 || dev >= 64) return bbfail(BBMAP_E_ARG, "%s: device ordinal beyond 63", who);
    std::lock_guard<std::mutex> lock(mu);
    if (!ready[dev]) {
        BBTRY(bb_use_gfx950(who, dev));
        ready[dev] = true;
    }
    return BBMAP_OK;
}

// one native on the host: the same column sums and the same walks, the triples in plain arrays
template <bool Q> static void host_search(const std::vector<Col> &a, const std::vector<Col> &b, const Params &p, int alen, int blen,
                                          std::vector<float> &g, std::vector<float> &bd, std::vector<float> &rt, bbmerge_rec &r) {
    const Range range = insert_range(p, alen, blen);
    const Cols A{a.data()}, B{b.data()};
    for (int k = 0; k <= range.hi - range.lo; k++) {
        const Span s = span_of(range.hi - k, alen, blen);
        column_sums<Q>(A, B, s, p.gIncr, p.bIncr, g[k], bd[k]);
        rt[k] = ratio_of(bd[k], p.offset, s.len);
    }
    decide<Q>(HostWave(), Triples{g.data(), bd.data(), rt.data()}, p, range, alen, blen, r);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The verdict (merge_shared.h: verdict_of).  Same geometry as the overlap kernel: one wavefront per pair, the mates in LDS, now with
// their qualities beside them for the filters.  bbmerge_stats is counted from the records by a kernel of its own, below.
// The entropy scans are one lane's work: under the defaults a scan ends after about a dozen bases, and only a low-complexity mate is
// walked to its end.  The normal mode's counts go lane per overlap like the ratio sums, into the same LDS arrays (a count is at most
// 512 and exact as a float).  The filters look at one insert per pair: 64 lanes work out 64 columns' terms, then the terms are folded
// in column order.
static const float h_probCorrect2[MAX_FILTER_QUALITY + 1] = {BBMERGE_PROB_CORRECT2};
__device__ const float d_probCorrect2[MAX_FILTER_QUALITY + 1] = {BBMERGE_PROB_CORRECT2};

// a mate with its qualities, as the filters read it
struct QCols {
    const Col *c; const uint8_t *q;
    __host__ __device__ int base(int i) const { return c[i].base; }
    __host__ __device__ float prob(int i) const { return c[i].p; }
    __host__ __device__ int qual(int i) const { return q[i]; }
};
// the normal mode's per-overlap counts as normal_decide() reads them
struct Counts {
    const float *g, *b;
    __host__ __device__ float good(int k) const { return g[k]; }
    __host__ __device__ float bad(int k) const { return b[k]; }
};

template <int MAXLEN> struct VerdictLds {
    PairLds<MAXLEN> pair;
    uint8_t qa[MAXLEN], qb[MAXLEN];
    // The entropy scans' k-mer counts (4^k of them) live in the per-insert arrays, which nobody needs before the first search: the
    // short class keeps the overlap kernel's 20 wavefronts per CU.
    // For k = 5 the 2 KB of counts run from good[] on into bad[]: the three arrays must follow each other in this order.
    static_assert(offsetof(PairLds<MAXLEN>, bad) == offsetof(PairLds<MAXLEN>, good) + sizeof(float) * 2 * MAXLEN &&
                  offsetof(PairLds<MAXLEN>, ratio) == offsetof(PairLds<MAXLEN>, bad) + sizeof(float) * 2 * MAXLEN &&
                  sizeof(PairLds<MAXLEN>) == offsetof(PairLds<MAXLEN>, ratio) + sizeof(float) * 2 * MAXLEN, "good, bad, ratio are one run of floats");
    static_assert(sizeof(float) * 3 * 2 * MAXLEN >= sizeof(uint16_t) << (2 * MAX_ENTROPY_K), "the counts fit good, bad and ratio");
    __device__ uint16_t *counts() { return reinterpret_cast<uint16_t *>(pair.good); }
};

// the pair in LDS; every method is called by the whole wavefront in uniform control flow
template <int MAXLEN> struct DevicePair {
    VerdictLds<MAXLEN> &S;
    const bbmerge_verdict_config &c;
    int alen, blen;
    __device__ int entropy(bool tail) {
        __syncthreads();                        // the mates are in LDS; the scan before this one is over
        uint16_t *counts = S.counts();
        for (int i = (int)threadIdx.x; i < (1 << (2 * c.entropyK)); i += 64) counts[i] = 0;
        __syncthreads();
        int r = 0;
        if (threadIdx.x == 0)
            r = tail ? entropy_scan(FromEnd<Cols>{Cols{S.pair.a}, alen}, alen, c.entropyK, c.minEntropyScore, counts)
                     : entropy_scan(Cols{S.pair.b}, blen, c.entropyK, c.minEntropyScore, counts);
        return __shfl(r, 0);
    }
    __device__ int entropy_a() { return entropy(true); }
    __device__ int entropy_b() { return entropy(false); }
    template <bool Q> __device__ void ratio(const Params &p, bbmerge_rec &r) { search<Q>(S.pair, p, alen, blen, r); }
    template <bool Q> __device__ int normal(const NormalParams &p, int &bad, int &ambig) {
        const Cols A{S.pair.a}, B{S.pair.b};
        const float minprob = d_probCorrect[p.minq];
        const int n = p.maxOverlap - p.first;
        __syncthreads();                        // the walks before this pass have read their triples
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + (int)threadIdx.x;
            if (k < n) {
                int g, b;
                normal_counts<Q>(A, B, p.first + k, alen, blen, minprob, g, b);
                S.pair.good[k] = (float)g; S.pair.bad[k] = (float)b;
            }
        }
        __syncthreads();
        return normal_decide(DeviceWave(), Counts{S.pair.good, S.pair.bad}, p, alen, blen, bad, ambig);
    }
    // the filters: 64 lanes work out the terms of 64 columns, then every lane folds them in column order (lane l's term comes
    // through a scalar register), so the table lookups of a chunk are in flight together and the order of the float operations is
    // the reference's
    static __device__ float lane_value(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
    __device__ float expected(int insert) {
        const QCols A{S.pair.a, S.qa}, B{S.pair.b, S.qb};
        const FilterSpan s = expected_span(alen, blen, __builtin_amdgcn_readfirstlane(insert));
        float expected = 0;
        for (int c0 = 0; c0 < s.n; c0 += 64) {
            const int col = c0 + (int)threadIdx.x;
            const float t = col < s.n ? expected_term(A, B, s.istart + col, s.jstart + col, d_probCorrect2) : 0.0f;
            for (int l = 0, cnt = imin(64, s.n - c0); l < cnt; l++) expected += lane_value(t, l);
        }
        return expected;
    }
    __device__ float probability(int insert) {
        const QCols A{S.pair.a, S.qa}, B{S.pair.b, S.qb};
        const FilterSpan s = probability_span(alen, blen, __builtin_amdgcn_readfirstlane(insert));
        float probActual = 1, probCommon = 1;
        for (int c0 = 0; c0 < s.n; c0 += 64) {
            const int col = c0 + (int)threadIdx.x;
            float common = 1, actual = 1;
            if (col < s.n) probability_terms(A, B, s.istart + col, s.jstart + col, d_probCorrect2, common, actual);
            for (int l = 0, cnt = imin(64, s.n - c0); l < cnt; l++) {
                probCommon *= lane_value(common, l); probActual *= lane_value(actual, l);
            }
        }
        return probability_of(probActual, probCommon);
    }
};

// Pairs whose longer mate has MINLEN < length <= MAXLEN; the launch with MAXLEN == BBMERGE_MAX_READ_LEN also reports longer pairs.
template <int MINLEN, int MAXLEN>
__global__ void __launch_bounds__(64) bbmerge_verdict_kernel(bbmerge_verdict_config cfg, const bbidx_read *reads1, const bbidx_read *reads2,
                                                             const uint8_t *bases, const uint8_t *quality, bbmerge_verdict_rec *recs) {
    __shared__ VerdictLds<MAXLEN> S;
    const long long pair = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const bbidx_read r1 = reads1[pair], r2 = reads2[pair];
    const int alen = imax(r1.len, 0), blen = imax(r2.len, 0);
    const int longer = imax(alen, blen);
    if (longer <= MINLEN || (longer > MAXLEN && MAXLEN != BBMERGE_MAX_READ_LEN)) return;
    const bool have_quality = cfg.useQuality != 0 && quality != nullptr;
    const bool prob_read = reads_prob_correct(cfg, have_quality), filtered = filters_on(cfg, have_quality);
    bbmerge_verdict_rec v;
    bool outside = longer > MAXLEN;
    if (!outside) {
        for (int i = lane; i < alen; i += 64) {
            Col c;
            c.base = (int8_t)bases[r1.bases_off + i]; c.p = 0;
            if (have_quality) {
                const int q = quality[r1.bases_off + i];
                outside |= (prob_read && q > MAX_QUALITY) || (filtered && q > MAX_FILTER_QUALITY);
                if (prob_read) c.p = d_probCorrect[imin(q, MAX_QUALITY)];
                S.qa[i] = (uint8_t)imin(q, MAX_FILTER_QUALITY);
            }
            S.pair.a[i] = c;
        }
        for (int i = lane; i < blen; i += 64) {      // Read.reverseComplement: base i of b is the complement of mate 2's base blen - 1 - i
            Col c;
            c.base = (int8_t)bbpipe::complement_extended(bases[r2.bases_off + blen - 1 - i]); c.p = 0;
            if (have_quality) {
                const int q = quality[r2.bases_off + blen - 1 - i];
                outside |= (prob_read && q > MAX_QUALITY) || (filtered && q > MAX_FILTER_QUALITY);
                if (prob_read) c.p = d_probCorrect[imin(q, MAX_QUALITY)];
                S.qb[i] = (uint8_t)imin(q, MAX_FILTER_QUALITY);
            }
            S.pair.b[i] = c;
        }
        outside = __any(outside);
    }
    if (outside) {
        skipped_verdict(v);
    } else {
        DevicePair<MAXLEN> e{S, cfg, alen, blen};
        verdict_of(e, cfg, alen, blen, have_quality, v);
    }
    if (lane == 0) recs[pair] = v;
}

// bbmerge_stats from the records.  One pair's wavefront adding its own counts would send a million atomics to the same few
// addresses (measured: 87 ms for 1 M pairs beside 9 ms for the verdicts themselves), so the counting is a pass of its own over the
// 48-byte records: a workgroup takes 8192 consecutive records, its threads stride through them by 256 and count in registers, the
// workgroup sums in LDS (its own histogram included), and one thread per counter or bin adds to memory what the workgroup holds.
constexpr int STATS_THREADS = 256, STATS_RECORDS_PER_BLOCK = 8192;
__global__ void __launch_bounds__(STATS_THREADS) bbmerge_stats_kernel(long long n, const bbmerge_verdict_rec *recs, bbmerge_stats *stats) {
    typedef unsigned long long U;               // (every counter is >= 0)
    __shared__ unsigned hist[BBMERGE_HIST_LEN];
    __shared__ U sums[8];                       // pairs, merged, ambiguous, tooShort, tooLong, noSolution, skipped, insertSum
    __shared__ int lo, hi;
    for (int i = (int)threadIdx.x; i < BBMERGE_HIST_LEN; i += STATS_THREADS) hist[i] = 0;
    if (threadIdx.x < 8) sums[threadIdx.x] = 0;
    if (threadIdx.x == 0) { lo = 999999999; hi = 0; }
    __syncthreads();
    StatsDelta d;
    d.clear();
    const long long first = (long long)blockIdx.x * STATS_RECORDS_PER_BLOCK;
    for (long long i = first + threadIdx.x; i < first + STATS_RECORDS_PER_BLOCK && i < n; i += STATS_THREADS) {
        bbmerge_verdict_rec v;
        v.code = recs[i].code; v.info = recs[i].info;
        d.count(v);
        if (v.code > 0 && !(v.info & BBMERGE_INFO_SKIPPED)) atomicAdd(&hist[imin(v.code, BBMERGE_HIST_LEN - 1)], 1u);
    }
    const int part[7] = {d.pairs, d.merged, d.ambiguous, d.tooShort, d.tooLong, d.noSolution, d.skipped};
    for (int k = 0; k < 7; k++) if (part[k]) atomicAdd(&sums[k], (U)part[k]);
    if (d.merged) {
        atomicAdd(&sums[7], (U)d.insertSum);
        atomicMin(&lo, d.insertMin);
        atomicMax(&hi, d.insertMax);
    }
    __syncthreads();
    U *const out[8] = {(U *)&stats->pairs, (U *)&stats->merged, (U *)&stats->ambiguous, (U *)&stats->tooShort, (U *)&stats->tooLong,
                       (U *)&stats->noSolution, (U *)&stats->skipped, (U *)&stats->insertSum};
    if (threadIdx.x < 8 && sums[threadIdx.x]) atomicAdd(out[threadIdx.x], sums[threadIdx.x]);
    if (threadIdx.x == 8 && sums[1]) { atomicMin((U *)&stats->insertMin, (U)lo); atomicMax((U *)&stats->insertMax, (U)hi); }
    for (int i = (int)threadIdx.x; i < BBMERGE_HIST_LEN; i += STATS_THREADS) if (hist[i]) atomicAdd((U *)&stats->hist[i], (U)hist[i]);
}

// the pair in plain arrays: the same functions, the wavefront a loop
struct HostPair {
    const bbmerge_verdict_config &c;
    int alen, blen;
    std::vector<Col> &a, &b;
    std::vector<uint8_t> &qa, &qb;
    std::vector<uint16_t> &counts;
    std::vector<float> &g, &bd, &rt;
    int entropy_a() {
        std::fill(counts.begin(), counts.end(), (uint16_t)0);
        return entropy_scan(FromEnd<Cols>{Cols{a.data()}, alen}, alen, c.entropyK, c.minEntropyScore, counts.data());
    }
    int entropy_b() {
        std::fill(counts.begin(), counts.end(), (uint16_t)0);
        return entropy_scan(Cols{b.data()}, blen, c.entropyK, c.minEntropyScore, counts.data());
    }
    template <bool Q> void ratio(const Params &p, bbmerge_rec &r) { host_search<Q>(a, b, p, alen, blen, g, bd, rt, r); }
    template <bool Q> int normal(const NormalParams &p, int &bad, int &ambig) {
        const Cols A{a.data()}, B{b.data()};
        for (int k = 0; k < p.maxOverlap - p.first; k++) {
            int gk, bk;
            normal_counts<Q>(A, B, p.first + k, alen, blen, h_probCorrect[p.minq], gk, bk);
            g[k] = (float)gk; bd[k] = (float)bk;
        }
        return normal_decide(HostWave(), Counts{g.data(), bd.data()}, p, alen, blen, bad, ambig);
    }
    float expected(int insert) { return expected_mismatches(QCols{a.data(), qa.data()}, QCols{b.data(), qb.data()}, alen, blen, insert, h_probCorrect2); }
    float probability(int insert) { return merge_probability(QCols{a.data(), qa.data()}, QCols{b.data(), qb.data()}, alen, blen, insert, h_probCorrect2); }
};

static int check_verdict_args(const char *who, const bbmerge_verdict_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                              const uint8_t *bases, const bbmerge_verdict_rec *recs) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "%s: null config", who);
    BBTRY(check_config(who, &cfg->ratio, n_pairs));
    if (!good_verdict_config(*cfg))
        return bbfail(BBMAP_E_ARG, "%s: bad config (entropyK 1..5, qualIters >= 1, 0 <= maxMismatches0 >= maxMismatches >= margin, a mode on, no NaN)", who);
    if (n_pairs > 0 && (!reads1 || !reads2 || !bases || !recs)) return bbfail(BBMAP_E_ARG, "%s: null buffer", who);
    return BBMAP_OK;
}

}  // namespace bbmerge

extern "C" int bbmerge_default_verdict_config(bbmerge_verdict_config *cfg) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "bbmerge_default_verdict_config: null argument");
    BBTRY(bbmerge_default_config(&cfg->ratio));
    cfg->useEntropy = 1; cfg->entropyK = 3; cfg->minEntropyScore = 39;                       // BBMerge.java: useEntropy, entropyK, minEntropyScore
    cfg->minOverlapBases = 11; cfg->minOverlapBases0 = 8; cfg->ratioReduction = 3;
    cfg->useRatioMode = 1; cfg->useNormalMode = 0; cfg->requireRatioMatch = 0; cfg->maxMismatchesR = 20;
    cfg->margin = 2; cfg->maxMismatches = 3; cfg->maxMismatches0 = 3; cfg->minQuality = 10; cfg->qualIters = 3;
    cfg->useQuality = 1; cfg->useEfilter = 1;
    cfg->efilterRatio = 6.0f; cfg->efilterOffset = 0.05f; cfg->pfilterRatio = 0.00004f;
    cfg->maxLength = 0; cfg->reserved = 0;
    return BBMAP_OK;
}

extern "C" int bbmerge_verdict_batch(const bbmerge_verdict_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                                     const uint8_t *bases, const uint8_t *quality, bbmerge_verdict_rec *recs, bbmerge_stats *stats) {
    using namespace bbmerge;
    BBTRY(check_verdict_args("bbmerge_verdict_batch", cfg, n_pairs, reads1, reads2, bases, recs));
    const bool have_quality = cfg->useQuality != 0 && quality != nullptr;
    const bool prob_read = reads_prob_correct(*cfg, have_quality), filtered = filters_on(*cfg, have_quality);
    std::vector<Col> a(BBMERGE_MAX_READ_LEN), b(BBMERGE_MAX_READ_LEN);
    std::vector<uint8_t> qa(BBMERGE_MAX_READ_LEN), qb(BBMERGE_MAX_READ_LEN);
    std::vector<uint16_t> counts(1 << (2 * cfg->entropyK));
    std::vector<float> g(2 * BBMERGE_MAX_READ_LEN), bd(2 * BBMERGE_MAX_READ_LEN), rt(2 * BBMERGE_MAX_READ_LEN);
    StatsDelta delta;
    delta.clear();
    for (int64_t pair = 0; pair < n_pairs; pair++) {
        const bbidx_read r1 = reads1[pair], r2 = reads2[pair];
        const int alen = imax(r1.len, 0), blen = imax(r2.len, 0);
        bbmerge_verdict_rec v;
        bool outside = imax(alen, blen) > BBMERGE_MAX_READ_LEN;
        for (int i = 0; i < alen && !outside; i++) {
            a[i].base = (int8_t)bases[r1.bases_off + i]; a[i].p = 0;
            if (have_quality) {
                const int q = quality[r1.bases_off + i];
                outside |= (prob_read && q > MAX_QUALITY) || (filtered && q > MAX_FILTER_QUALITY);
                if (prob_read) a[i].p = h_probCorrect[imin(q, MAX_QUALITY)];
                qa[i] = (uint8_t)imin(q, MAX_FILTER_QUALITY);
            }
        }
        for (int i = 0; i < blen && !outside; i++) {
            b[i].base = (int8_t)bbpipe::complement_extended(bases[r2.bases_off + blen - 1 - i]); b[i].p = 0;
            if (have_quality) {
                const int q = quality[r2.bases_off + blen - 1 - i];
                outside |= (prob_read && q > MAX_QUALITY) || (filtered && q > MAX_FILTER_QUALITY);
                if (prob_read) b[i].p = h_probCorrect[imin(q, MAX_QUALITY)];
                qb[i] = (uint8_t)imin(q, MAX_FILTER_QUALITY);
            }
        }
        if (outside) {
            skipped_verdict(v);
        } else {
            HostPair e{*cfg, alen, blen, a, b, qa, qb, counts, g, bd, rt};
            verdict_of(e, *cfg, alen, blen, have_quality, v);
        }
        recs[pair] = v;
        delta.count(v);
        if (stats && v.code > 0 && !(v.info & BBMERGE_INFO_SKIPPED)) stats->hist[imin(v.code, BBMERGE_HIST_LEN - 1)]++;
    }
    if (stats) {
        stats->pairs += delta.pairs; stats->merged += delta.merged; stats->ambiguous += delta.ambiguous; stats->tooShort += delta.tooShort;
        stats->tooLong += delta.tooLong; stats->noSolution += delta.noSolution; stats->skipped += delta.skipped;
        stats->insertSum += delta.insertSum;
        if (delta.merged) {
            if (delta.insertMin < stats->insertMin) stats->insertMin = delta.insertMin;
            if (delta.insertMax > stats->insertMax) stats->insertMax = delta.insertMax;
        }
    }
    return BBMAP_OK;
}

extern "C" int bbmerge_verdict_batch_device(const bbmerge_verdict_config *cfg, void *stream, int64_t n_pairs, const bbidx_read *reads1,
                                            const bbidx_read *reads2, const uint8_t *bases, const uint8_t *quality, bbmerge_verdict_rec *recs,
                                            bbmerge_stats *stats) {
    using namespace bbmerge;
    BBTRY(check_verdict_args("bbmerge_verdict_batch_device", cfg, n_pairs, reads1, reads2, bases, recs));
    if (n_pairs == 0) return BBMAP_OK;
    BBTRY(prepare_device("bbmerge_verdict_batch_device"));
    const int64_t chunk = 1 << 24;              // (a grid holds fewer than 2^32 threads)
    for (int64_t at = 0; at < n_pairs; at += chunk) {
        const unsigned blocks = (unsigned)(n_pairs - at < chunk ? n_pairs - at : chunk);
        hipLaunchKernelGGL((bbmerge_verdict_kernel<-1, SHORT_LEN>), dim3(blocks), dim3(64), 0, (hipStream_t)stream, *cfg, reads1 + at, reads2 + at, bases,
                           quality, recs + at);
        BBHIP(hipGetLastError());
        hipLaunchKernelGGL((bbmerge_verdict_kernel<SHORT_LEN, BBMERGE_MAX_READ_LEN>), dim3(blocks), dim3(64), 0, (hipStream_t)stream, *cfg, reads1 + at,
                           reads2 + at, bases, quality, recs + at);
        BBHIP(hipGetLastError());
    }
    if (stats) {
        const unsigned blocks = (unsigned)((n_pairs + STATS_RECORDS_PER_BLOCK - 1) / STATS_RECORDS_PER_BLOCK);
        hipLaunchKernelGGL(bbmerge_stats_kernel, dim3(blocks), dim3(STATS_THREADS), 0, (hipStream_t)stream, (long long)n_pairs, recs, stats);
        BBHIP(hipGetLastError());
    }
    return BBMAP_OK;
}

extern "C" int bbmerge_default_config(bbmerge_config *cfg) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "bbmerge_default_config: null argument");
    cfg->minOverlap0 = 8 - 3; cfg->minOverlap = 11 - 3;          // MIN_OVERLAPPING_BASES_0, MIN_OVERLAPPING_BASES, less the ratio reduction
    cfg->minInsert = 35; cfg->minInsert0 = 26;                   // min(35, max((int)(35 * 0.75), 5, 8)), BBMerge.java:605-611
    cfg->maxRatio = 0.09f; cfg->ratioMargin = 5.5f; cfg->ratioOffset = 0.55f; cfg->gIncr = 0.95f; cfg->bIncr = 0.95f;
    cfg->useQuality = 0; cfg->withoutQuality = 1;
    cfg->maxMergeQuality = 41;
    return BBMAP_OK;
}

extern "C" int bbmerge_overlap_batch(const bbmerge_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                                     const uint8_t *bases, const uint8_t *quality, bbmerge_rec *recs) {
    using namespace bbmerge;
    BBTRY(check_overlap_args("bbmerge_overlap_batch", cfg, n_pairs, reads1, reads2, bases, recs));
    const Params p = params_of(*cfg);
    const bool quality_form = runs_quality_form(*cfg, quality != nullptr);
    std::vector<Col> a(BBMERGE_MAX_READ_LEN), b(BBMERGE_MAX_READ_LEN);
    std::vector<float> g(2 * BBMERGE_MAX_READ_LEN), bd(2 * BBMERGE_MAX_READ_LEN), rt(2 * BBMERGE_MAX_READ_LEN);
    for (int64_t pair = 0; pair < n_pairs; pair++) {
        const bbidx_read r1 = reads1[pair], r2 = reads2[pair];
        const int alen = imax(r1.len, 0), blen = imax(r2.len, 0);
        recs[pair] = SKIPPED;
        if (imax(alen, blen) > BBMERGE_MAX_READ_LEN) continue;
        bool outside = false;
        for (int i = 0; i < alen; i++) {
            a[i].base = (int8_t)bases[r1.bases_off + i]; a[i].p = 0;
            if (quality_form) {
                const int q = quality[r1.bases_off + i];
                outside |= q > MAX_QUALITY;
                a[i].p = h_probCorrect[imin(q, MAX_QUALITY)];
            }
        }
        for (int i = 0; i < blen; i++) {
            b[i].base = (int8_t)bbpipe::complement_extended(bases[r2.bases_off + blen - 1 - i]); b[i].p = 0;
            if (quality_form) {
                const int q = quality[r2.bases_off + blen - 1 - i];
                outside |= q > MAX_QUALITY;
                b[i].p = h_probCorrect[imin(q, MAX_QUALITY)];
            }
        }
        if (outside) continue;
        bbmerge_rec r = {-1, 0, 0, 0};
        if (quality_form) {
            host_search<true>(a, b, p, alen, blen, g, bd, rt, r);
            r.info |= BBMERGE_INFO_QUALITY;
        }
        if (runs_flat_form(*cfg, quality_form, r)) {
            host_search<false>(a, b, p, alen, blen, g, bd, rt, r);
            r.info |= BBMERGE_INFO_FLAT;
        }
        recs[pair] = r;
    }
    return BBMAP_OK;
}

extern "C" int bbmerge_overlap_batch_device(const bbmerge_config *cfg, void *stream, int64_t n_pairs, const bbidx_read *reads1,
                                            const bbidx_read *reads2, const uint8_t *bases, const uint8_t *quality, bbmerge_rec *recs) {
    using namespace bbmerge;
    BBTRY(check_overlap_args("bbmerge_overlap_batch_device", cfg, n_pairs, reads1, reads2, bases, recs));
    if (n_pairs == 0) return BBMAP_OK;
    BBTRY(prepare_device("bbmerge_overlap_batch_device"));
    const int64_t chunk = 1 << 24;              // (a grid holds fewer than 2^32 threads)
    for (int64_t at = 0; at < n_pairs; at += chunk) {
        const unsigned blocks = (unsigned)(n_pairs - at < chunk ? n_pairs - at : chunk);
        hipLaunchKernelGGL((bbmerge_overlap_kernel<-1, SHORT_LEN>), dim3(blocks), dim3(64), 0, (hipStream_t)stream, *cfg, reads1 + at, reads2 + at, bases,
                           quality, recs + at);
        BBHIP(hipGetLastError());
        hipLaunchKernelGGL((bbmerge_overlap_kernel<SHORT_LEN, BBMERGE_MAX_READ_LEN>), dim3(blocks), dim3(64), 0, (hipStream_t)stream, *cfg, reads1 + at,
                           reads2 + at, bases, quality, recs + at);
        BBHIP(hipGetLastError());
    }
    return BBMAP_OK;
}

extern "C" int bbmerge_join_batch(const bbmerge_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                                  const uint8_t *bases, const uint8_t *quality, const int32_t *insert, bbidx_read *merged,
                                  uint8_t *out_bases, uint8_t *out_quality) {
    using namespace bbmerge;
    BBTRY(check_join_args("bbmerge_join_batch", cfg, n_pairs, reads1, reads2, bases, quality, insert, merged, out_bases, out_quality));
    for (int64_t pair = 0; pair < n_pairs; pair++) {
        const bbidx_read r1 = reads1[pair], r2 = reads2[pair];
        const int alen = imax(r1.len, 0), blen = imax(r2.len, 0);
        const int len = joined_length(insert[pair], alen, blen);
        const int64_t out = merged[pair].bases_off;
        for (int i = 0; i < len; i++) {
            uint8_t base, qual;
            join_pair_column(bases, quality, quality != nullptr, r1, r2, alen, blen, len, i, cfg->maxMergeQuality, base, qual);
            out_bases[out + i] = base;
            if (quality) out_quality[out + i] = qual;
        }
        merged[pair].len = len;
    }
    return BBMAP_OK;
}

extern "C" int bbmerge_join_batch_device(const bbmerge_config *cfg, void *stream, int64_t n_pairs, const bbidx_read *reads1,
                                         const bbidx_read *reads2, const uint8_t *bases, const uint8_t *quality, const int32_t *insert,
                                         bbidx_read *merged, uint8_t *out_bases, uint8_t *out_quality) {
    using namespace bbmerge;
    BBTRY(check_join_args("bbmerge_join_batch_device", cfg, n_pairs, reads1, reads2, bases, quality, insert, merged, out_bases, out_quality));
    if (n_pairs == 0) return BBMAP_OK;
    BBTRY(prepare_device("bbmerge_join_batch_device"));
    const int64_t chunk = 1 << 24;              // (a grid holds fewer than 2^32 threads)
    for (int64_t at = 0; at < n_pairs; at += chunk) {
        const int64_t n = n_pairs - at < chunk ? n_pairs - at : chunk;
        BBTRY(launch<256>(bbmerge_join_kernel, n * 64, (hipStream_t)stream, (int)cfg->maxMergeQuality, (long long)n, reads1 + at, reads2 + at, bases,
                          quality, insert + at, merged + at, out_bases, out_quality));
    }
    return BBMAP_OK;
}
