// The width sort in front of the first pass: a counting sort of the launch's jobs by (class, columns / 8 descending) into one list
// per class.  Classes: unlimited fills (the wavefront kernel's prune-free build takes them), band candidates (msa_fill_band.hip; only
// when the launch runs the band kernel over a list, bbmsa_sort_with_band), everything else (the general build).
#include <hip/hip_runtime.h>

#include "host_common.h"
#include "msa_common.h"
#include "msa_ctx.h"

namespace bbmsa {
constexpr int WIDTH_PER_CLASS = 512;           // columns / 8.  Only 11ts contexts sort, and bbmsa_create refuses one of more than 4,096
                                               // columns, so only a window of exactly 4,096 shares its bucket (with 4,088..4,095)
constexpr int WIDTH_CLASSES = 3;
constexpr int WIDTH_BUCKETS = WIDTH_CLASSES * WIDTH_PER_CLASS;
enum { CLASS_UNLIMITED = 0, CLASS_CANDIDATE = 1, CLASS_GENERAL = 2 };
constexpr int SORT_THREADS = 256, SORT_JOBS_PER_THREAD = 4;     // a block of the histogram / scatter kernels takes 1,024 jobs
struct SortKey { int maxRows, maxColumns, bandwidth; float bandwidthRatio; int byKind, band, bandRows, maxSlack; };
// byKind: the unlimited fills get their own list (else they are general jobs); band: so do the band kernel's candidates, by the
// kernel's own rule (band_is_candidate, msa_common.h).
__device__ inline int job_width_bucket(const bbmsa_job &t, const SortKey k) {
    int a = t.refStartLoc, b = t.refEndLoc;
    if (t.flags & BBMSA_CLAMP_WINDOW) { a = max(0, a); b = min(t.ref_len - 1, b); if (b - a >= k.maxColumns) b = min(t.ref_len - 1, a + k.maxColumns - 1); }
    const int cols = max(0, b - a + 1);
    int cls = CLASS_GENERAL;
    if (k.band && band_is_candidate(t.flags, t.minScore, t.read_len, b - a + 1, k.maxRows, k.maxColumns, k.bandRows, k.maxSlack)) cls = CLASS_CANDIDATE;
    else if (k.byKind && !fill_is_limited(t.flags, t.minScore, t.read_len, b - a + 1, fill_halfband(t.read_len, b - a + 1, k.bandwidth, k.bandwidthRatio))) cls = CLASS_UNLIMITED;
    constexpr int W = WIDTH_PER_CLASS;
    return cls * W + W - 1 - min(W - 1, cols >> 3);            // bucket 0 of a class = its widest windows
}
// Both kernels count in an LDS copy of the histogram first: a launch's windows crowd into a few buckets (half of the plain context's
// fills have one width), and one global atomic per job on those few words is what the kernels then wait for.  A block adds each bucket
// it met to the global word once.
__global__ __launch_bounds__(SORT_THREADS) void width_hist_kernel(const bbmsa_job *jobs, long long n, SortKey key, unsigned *hist) {
    __shared__ unsigned s[WIDTH_BUCKETS];
    for (int i = threadIdx.x; i < WIDTH_BUCKETS; i += SORT_THREADS) s[i] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * (SORT_THREADS * SORT_JOBS_PER_THREAD) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < SORT_JOBS_PER_THREAD; k++) {
        const long long i = base + (long long)k * SORT_THREADS;
        if (i < n) atomicAdd(&s[job_width_bucket(jobs[i], key)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < WIDTH_BUCKETS; i += SORT_THREADS) { const unsigned v = s[i]; if (v) atomicAdd(&hist[i], v); }
}
// one block of WIDTH_PER_CLASS threads: exclusive prefix sums in place, each class's from 0 (the scatter's cursors), and the lengths of
// the three lists.  The general list's length goes to two words: `listCount`, which the band kernel then appends its hand-overs
// through, and `sortedCount`, which keeps it.
__global__ void width_scan_kernel(unsigned *hist, unsigned *listCount, unsigned *sortedCount, unsigned *unlCount, unsigned *candCount) {
    __shared__ unsigned s[WIDTH_PER_CLASS];
    const int t = threadIdx.x;
    for (int cls = 0; cls < WIDTH_CLASSES; cls++) {
        const unsigned own = hist[cls * WIDTH_PER_CLASS + t];
        s[t] = own;
        __syncthreads();
        for (int d = 1; d < WIDTH_PER_CLASS; d <<= 1) { const unsigned v = t >= d ? s[t - d] : 0u; __syncthreads(); s[t] += v; __syncthreads(); }
        hist[cls * WIDTH_PER_CLASS + t] = s[t] - own;
        if (t == WIDTH_PER_CLASS - 1) {
            if (cls == CLASS_UNLIMITED) *unlCount = s[t];
            else if (cls == CLASS_CANDIDATE) *candCount = s[t];
            else { *listCount = s[t]; *sortedCount = s[t]; }
        }
        __syncthreads();
    }
}
// every list has room for all n jobs; a job's place is its bucket's cursor + the block's share of the bucket + its rank in the block
__global__ __launch_bounds__(SORT_THREADS) void width_scatter_kernel(const bbmsa_job *jobs, long long n, SortKey key, unsigned *cursor, int *list, int *unlList, int *candList) {
    __shared__ unsigned s[WIDTH_BUCKETS];
    for (int i = threadIdx.x; i < WIDTH_BUCKETS; i += SORT_THREADS) s[i] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * (SORT_THREADS * SORT_JOBS_PER_THREAD) + threadIdx.x;
    int bucket[SORT_JOBS_PER_THREAD]; unsigned rank[SORT_JOBS_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SORT_JOBS_PER_THREAD; k++) {
        const long long i = base + (long long)k * SORT_THREADS;
        bucket[k] = -1; rank[k] = 0;
        if (i < n) { bucket[k] = job_width_bucket(jobs[i], key); rank[k] = atomicAdd(&s[bucket[k]], 1u); }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < WIDTH_BUCKETS; i += SORT_THREADS) { const unsigned v = s[i]; if (v) s[i] = atomicAdd(&cursor[i], v); }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SORT_JOBS_PER_THREAD; k++) {
        if (bucket[k] < 0) continue;
        const long long i = base + (long long)k * SORT_THREADS;
        const unsigned pos = s[bucket[k]] + rank[k];
        if ((long long)pos >= n) continue;                      // (cannot happen: a class holds at most n jobs)
        const int cls = bucket[k] / WIDTH_PER_CLASS;
        (cls == CLASS_UNLIMITED ? unlList : (cls == CLASS_CANDIDATE ? candList : list))[pos] = (int)i;
    }
}
}  // namespace bbmsa

int bbmsa_width_sort(bbmsa_ctx *c, hipStream_t stream, const bbmsa_job *jobs, int64_t n_jobs, bool band) {
    using namespace bbmsa;
    if (!c->d_widthHist) BBHIP(hipMalloc(&c->d_widthHist, WIDTH_BUCKETS * 4));
    BBHIP(hipMemsetAsync(c->d_widthHist, 0, WIDTH_BUCKETS * 4, stream));
    const int perBlock = SORT_THREADS * SORT_JOBS_PER_THREAD;
    const unsigned sb = (unsigned)((n_jobs + perBlock - 1) / perBlock);
    const SortKey key = {c->cfg.maxRows, c->cfg.maxColumns, c->cfg.bandwidth, c->cfg.bandwidthRatio, c->sw.unlimitedLoop ? 1 : 0,
                         band ? 1 : 0, c->bandRows, c->narrowSlack};
    int *const list = c->fastList.as<int>();
    unsigned *const cnt = c->d_counters;
    hipLaunchKernelGGL(width_hist_kernel, dim3(sb), dim3(SORT_THREADS), 0, stream, jobs, (long long)n_jobs, key, c->d_widthHist);
    hipLaunchKernelGGL(width_scan_kernel, dim3(1), dim3(WIDTH_PER_CLASS), 0, stream, c->d_widthHist, cnt + CNT_LIST_COUNT, cnt + CNT_SORTED_COUNT,
                       cnt + CNT_UNL_LIST_COUNT, cnt + CNT_CAND_COUNT);
    hipLaunchKernelGGL(width_scatter_kernel, dim3(sb), dim3(SORT_THREADS), 0, stream, jobs, (long long)n_jobs, key, c->d_widthHist,
                       list, list + n_jobs, list + 2 * n_jobs);
    BBHIP(hipGetLastError());
    return BBMAP_OK;
}
