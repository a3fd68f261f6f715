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

}  // namespace bbmerge

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
