// Host side of the MultiStateAligner11ts C ABI (include/bbmap_amd.h): context, scratch sizing,
// launch geometry and the two launches (wavefront kernel, then the generic kernel over the jobs
// it handed back).  No CPU compute path exists here: without a HIP device every entry fails.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <new>

#include "host_common.h"
#include "msa_common.h"
#include "msa_ctx.h"

namespace bbmsa {
struct StripParams {            // msa_fill_strip.hip
    const bbmsa_job *jobs; const uint8_t *reads; const uint8_t *refs; bbmsa_result *results; uint8_t *match;
    long long njobs; const unsigned int *njobs_dev; unsigned int *queue; unsigned int *dirbuf;
    long long dir_slot_dwords, dir_strip_dwords; int *boundary; uint8_t *tmpbuf; int *slow_list; unsigned int *slow_count;
    int match_stride; int maxRows, maxColumns; int bandwidth; float bandwidthRatio;
    int pipeK, pipeSlots; int *pipeBoundary; int *pipeSync; int pipeSpinLimit;
};
int strip_rows_per_lane();
const void *strip_kernel_pacbio();
const void *strip_kernel_pacbio_pipelined();
int strip_pipe_sync_ints(int K);
const void *fast_kernel_for(int R, bool banded);
const void *fast_kernel_unl_for(int R);
const void *fast_kernel_both_for(int R);                       // both step loops, chosen per job (64 lanes per job only); null: no such build
constexpr int kCounterWords = 32, kCounterBytes = kCounterWords * 4;      // d_counters of every context (bbmsa_align_impl has the list)
template <class S> __global__ void msa_fill_generic_kernel(const GenericParams p);
const void *band_kernel();                                     // msa_fill_band.hip
int band_lds_bytes(int tableLen, int bandRows);
}  // namespace bbmsa

namespace bbmsa {
// The width sort in front of the first pass: a counting sort of the launch's jobs by (class, columns / 8 descending) into one list
// per class.  Classes: unlimited fills (the wavefront kernel's prune-free build takes them), band candidates (msa_fill_band.hip; only
// when the launch runs the band kernel over a list, bbmsa_sort_with_band), everything else (the general build).
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

// The wavefront kernel's second geometry: 64 lanes per job, one job per 64-thread block, an LDS column buffer as wide as maxColumns.
// It takes the windows wider than the first pass's buffer (the wide pass) and, at the caller's request, whole launches that hold
// too few jobs to be anything but a wavefront's latency (bbmsa_set_latency_jobs).
static int setup_wide_pass(bbmsa_ctx *c) {
    if (c->wideBlocks > 0) return BBMAP_OK;
    c->wideR = (c->cfg.maxRows + 63) / 64;
    c->wideCols = c->cfg.maxColumns;
    c->wideTmpBytes = ((64 * c->wideR + c->wideCols + 8) + 3) & ~3;
    const int perJob = bbmsa::lds_job_ints(c->wideCols, c->wideTmpBytes);
    c->wideLdsBytes = (bbmsa::lds_table_ints(c->wideTableLen) + perJob) * 4;
    const void *wfn = bbmsa::fast_kernel_for(c->wideR, c->banded);
    if (wfn && c->wideLdsBytes <= 160 * 1024) {
        if (c->wideLdsBytes > 64 * 1024) BBHIP(hipFuncSetAttribute(wfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->wideLdsBytes));
        const void *bfn = c->banded ? nullptr : bbmsa::fast_kernel_both_for(c->wideR);      // (bbmsa_set_wide_unlimited)
        if (bfn && c->wideLdsBytes > 64 * 1024) BBHIP(hipFuncSetAttribute(bfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->wideLdsBytes));
        int per = 0;
        BBHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, wfn, 64, c->wideLdsBytes));
        if (per < 1) per = 1;
        if (per > 8) per = 8;
        const long long slotDwords = (long long)(((c->wideCols + 64 - 1) >> 3) + 1) * c->wideR * 64;
        BBHIP(hipMalloc(&c->d_wideDir, (size_t)((long long)c->numCUs * per * slotDwords * 4)));
        c->wideDirSlotDwords = slotDwords;
        c->wideBlocks = c->numCUs * per;
    }
    return BBMAP_OK;
}

extern "C" int bbmsa_create(const bbmsa_config *cfg, bbmsa_ctx **out) {
    if (!cfg || !out) return bbfail(BBMAP_E_ARG, "bbmsa_create: null argument");
    *out = nullptr;
    const int scheme = cfg->reserved[2] & 0xFF;
    const bool legacyOnly = (cfg->reserved[2] & BBMSA_LEGACY_ONLY) != 0;
    if (scheme != BBMSA_SCHEME_11TS && scheme != BBMSA_SCHEME_9PACBIO) return bbfail(BBMAP_E_ARG, "bbmsa_create: unknown scoring scheme");
    if (scheme == BBMSA_SCHEME_11TS && (cfg->maxRows < 1 || cfg->maxRows > 640 || cfg->maxColumns < 1 || cfg->maxColumns > 4096))
        return bbfail(BBMAP_E_ARG, "bbmsa_create: maxRows must be 1..640 and maxColumns 1..4096");
    if (scheme == BBMSA_SCHEME_9PACBIO && (cfg->maxRows < 1 || cfg->maxRows > 6100 || cfg->maxColumns < 1 || cfg->maxColumns > 8192))
        return bbfail(BBMAP_E_ARG, "bbmsa_create: the PacBio scheme takes maxRows 1..6100 and maxColumns 1..8192");
    hipDeviceProp_t prop;
    BBTRY(bb_use_gfx950("bbmsa_create", cfg->device, &prop));

    bbmsa_ctx *c = new (std::nothrow) bbmsa_ctx();
    if (!c) return bbfail(BBMAP_E_NOMEM, "bbmsa_create: out of host memory");
    c->cfg = *cfg;
    c->device = cfg->device;
    c->numCUs = prop.multiProcessorCount;

    c->scheme = scheme;
    c->legacyOnly = legacyOnly;
    // every failure below leaves through bbmsa_destroy(c): nothing allocated so far is leaked
    struct Guard { bbmsa_ctx *c; ~Guard() { if (c) bbmsa_destroy(c); } } guard{c};
    if (legacyOnly) {
        // a context for bbmsa_fill_packed only (the per-call JNI shape): one scratch matrix, no batch buffers
        BBHIP(hipMalloc(&c->d_counters, bbmsa::kCounterBytes));
        BBHIP(hipMemset(c->d_counters, 0, bbmsa::kCounterBytes));
        const long long planeInts = (long long)(cfg->maxRows + 1) * (cfg->maxColumns + 2);
        c->genThreads = 1;
        BBHIP(hipMalloc(&c->d_matrix, (size_t)(3 * planeInts * 4)));
        BBHIP(hipMalloc(&c->d_limits, (size_t)((cfg->maxRows + cfg->maxColumns + 4) * 4)));
        for (int i = 0; i < 4; i++) BBHIP(hipEventCreate(&c->ev[i]));
        BBTRY(bbmsa_legacy_create(c));
        guard.c = nullptr;
        *out = c;
        return BBMAP_OK;
    }
    if (scheme != BBMSA_SCHEME_11TS) {
        // 9PacBio: the strip-tiled wavefront kernel (msa_fill_strip.hip), one alignment per wavefront; banded fills and windows
        // narrower than the read are handed to the one-job-per-thread kernel
        BBHIP(hipMalloc(&c->d_counters, bbmsa::kCounterBytes));
        BBHIP(hipMemset(c->d_counters, 0, bbmsa::kCounterBytes));
        const long long planeInts = (long long)(cfg->maxRows + 1) * (cfg->maxColumns + 2);
        const long long perThread = 3 * planeInts * 4;
        long long budget = (long long)env_int("BBMSA_GENERIC_SCRATCH_MB", 40960) << 20;   // 6019 x 7600 (mapPacBio) needs 35 GB for one wavefront of matrices
        long long threads = budget / perThread;
        if (threads > 4096) threads = 4096;
        threads = (threads / 64) * 64;
        if (threads < 64) return bbfail(BBMAP_E_NOMEM, "bbmsa_create: BBMSA_GENERIC_SCRATCH_MB cannot hold one wavefront of scratch matrices for this maxRows x maxColumns");
        c->genThreads = (int)threads;
        BBHIP(hipMalloc(&c->d_matrix, (size_t)(threads * perThread)));
        BBHIP(hipMalloc(&c->d_limits, (size_t)(threads * (cfg->maxRows + cfg->maxColumns + 4) * 4)));
        {
            const int R = bbmsa::strip_rows_per_lane();
            c->stripLds = (cfg->maxColumns + 2) * 4 + ((cfg->maxColumns + 2 + 7) & ~7);     // horizLimit ints + reference bytes
            const void *kfn = bbmsa::strip_kernel_pacbio();
            if (c->stripLds > 64 * 1024) BBHIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->stripLds));
            // Resident wavefronts per CU, from the LDS a wavefront takes (160 KB per CU; the kernel holds ~128 VGPRs, up to 4 waves per
            // SIMD, so LDS is what limits it).  Not asked of hipOccupancyMaxActiveBlocksPerMultiprocessor: that query was seen to fail with
            // hipErrorUnknown depending on what the process had done before (after the CPU oracle had run in it), for reasons the
            // runtime's log does not give; nothing here depends on the exact figure (the pipelined form no longer assumes co-residency).
            int per = (160 * 1024) / (c->stripLds + 512);
            if (per < 1) per = 1;
            if (per > 8) per = 8;
            c->stripBlocks = c->numCUs * per;
            const int strips = (cfg->maxRows + 64 * R - 1) / (64 * R);
            c->stripDwords = (long long)(((cfg->maxColumns + 64) >> 3) + 1) * R * 64;
            c->stripSlotDwords = c->stripDwords * strips;
            // traceback records: 4 bits per cell of every resident job (23 MB per 6,000 x 7,600 job)
            long long dirBudget = (long long)env_int("BBMSA_STRIP_DIR_MB", 32768) << 20;
            while (c->stripBlocks > c->numCUs && (long long)c->stripBlocks * c->stripSlotDwords * 4 > dirBudget) c->stripBlocks -= c->numCUs;
            while (c->stripBlocks > 1 && (long long)c->stripBlocks * c->stripSlotDwords * 4 > dirBudget) c->stripBlocks /= 2;
            {   // the pipelined form for launches with few jobs: the strips of one job in `strips` wavefronts
                const void *kp = bbmsa::strip_kernel_pacbio_pipelined();
                if (c->stripLds > 64 * 1024) BBHIP(hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, c->stripLds));
                int perP = (160 * 1024) / (c->stripLds + 512);
                if (perP < 1) perP = 1;
                if (perP > 8) perP = 8;
                c->pipeK = strips;
                c->pipeSlots = (c->numCUs * perP) / strips;                  // every wavefront of every slot is resident: the hand-shakes need it
                if (c->pipeSlots > c->stripBlocks) c->pipeSlots = c->stripBlocks;
                if (c->pipeSlots > 256) c->pipeSlots = 256;
                c->pipeJobsMax = env_int("BBMSA_STRIP_PIPE_JOBS", 512);      // launches with at most this many jobs take the pipelined form
                if (strips < 2 || c->pipeSlots < 1) c->pipeJobsMax = 0;
                if (c->pipeJobsMax > 0) {
                    BBHIP(hipMalloc(&c->d_pipeBoundary, (size_t)((long long)c->pipeSlots * strips * 3 * (cfg->maxColumns + 2) * 4)));
                    BBHIP(hipMalloc(&c->d_pipeSync, (size_t)((long long)c->pipeSlots * bbmsa::strip_pipe_sync_ints(strips) * 4)));
                }
            }
            BBHIP(hipMalloc(&c->d_dir, (size_t)((long long)c->stripBlocks * c->stripSlotDwords * 4)));
            BBHIP(hipMalloc(&c->d_stripBoundary, (size_t)((long long)c->stripBlocks * 6 * (cfg->maxColumns + 2) * 4)));
            BBHIP(hipMalloc(&c->d_stripTmp, (size_t)((long long)c->stripBlocks * (cfg->maxRows + cfg->maxColumns + 8))));
        }
        for (int i = 0; i < 4; i++) BBHIP(hipEventCreate(&c->ev[i]));
        guard.c = nullptr;
        *out = c;
        return BBMAP_OK;
    }
    // lanes per job / rows per lane: smallest lane group whose <=10 rows per lane cover maxRows
    int G = cfg->reserved[0];
    if (G != 16 && G != 32 && G != 64) {
        G = env_int("BBMSA_LANES_PER_JOB", 0);
        if (G != 16 && G != 32 && G != 64) G = (cfg->maxRows <= 320) ? 32 : 64;
    }
    while (G < 64 && (cfg->maxRows + G - 1) / G > 10) G *= 2;
    c->G = G;
    c->R = (cfg->maxRows + G - 1) / G;
    int fastCols = cfg->reserved[1] > 0 ? cfg->reserved[1] : env_int("BBMSA_FAST_COLS", 0);
    if (fastCols <= 0) fastCols = cfg->maxColumns < 640 ? cfg->maxColumns : 640;
    if (fastCols > cfg->maxColumns) fastCols = cfg->maxColumns;
    c->fastCols = fastCols;
    c->tmpBytes = ((G * c->R + fastCols + 8) + 3) & ~3;
    const int jobsPerWave = 64 / G;
    const int perJobInts = bbmsa::lds_job_ints(fastCols, c->tmpBytes);
    {   // index = time + needed: time <= min(longer side + 1, 2047 (clamped)), needed <= rows.  The first pass only takes windows of
        // up to fastCols columns, so its tables are sized for those; the wide pass has its own (wideTableLen).
        const int side = (cfg->maxColumns > cfg->maxRows ? cfg->maxColumns : cfg->maxRows) + 2;
        c->wideTableLen = (side < 2048 ? side : 2048) + cfg->maxRows + 8;
        const int sideF = (fastCols > cfg->maxRows ? fastCols : cfg->maxRows) + 2;
        c->tableLen = (sideF < 2048 ? sideF : 2048) + cfg->maxRows + 8;
    }
    if (c->tableLen > bbmsa::kTableLen) c->tableLen = bbmsa::kTableLen;
    if (c->wideTableLen > bbmsa::kTableLen) c->wideTableLen = bbmsa::kTableLen;
    c->tableLen = (c->tableLen + 3) & ~3; c->wideTableLen = (c->wideTableLen + 3) & ~3;
    c->ldsBytes = (bbmsa::lds_table_ints(c->tableLen) + 4 * jobsPerWave * perJobInts) * 4;
    if (c->ldsBytes > 160 * 1024) return bbfail(BBMAP_E_ARG, "bbmsa_create: fast-path LDS budget exceeded; lower reserved[1] (fastCols)");

    c->banded = !(cfg->bandwidth < 1 && cfg->bandwidthRatio <= 0.0f);
    const void *kfn = bbmsa::fast_kernel_for(c->R, c->banded);
    if (!kfn) return bbfail(BBMAP_E_ARG, "bbmsa_create: no kernel for this rows-per-lane");
    if (c->ldsBytes > 64 * 1024) {
        BBHIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->ldsBytes));
        BBHIP(hipFuncSetAttribute(bbmsa::fast_kernel_unl_for(c->R), hipFuncAttributeMaxDynamicSharedMemorySize, c->ldsBytes));
    }
    int blocksPerCU = 0;
    BBHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocksPerCU, kfn, 256, c->ldsBytes));
    if (blocksPerCU < 1) blocksPerCU = 1;
    const int capBlocks = env_int("BBMSA_BLOCKS_PER_CU", 0);
    if (capBlocks > 0 && capBlocks < blocksPerCU) blocksPerCU = capBlocks;
    c->blocks = c->numCUs * blocksPerCU;

    const int maxSteps = fastCols + G - 1;
    c->dirSlotDwords = (long long)((maxSteps >> 3) + 1) * c->R * G;
    const long long slots = (long long)c->blocks * 4 * jobsPerWave;
    BBHIP(hipMalloc(&c->d_dir, (size_t)(slots * c->dirSlotDwords * 4)));
    BBHIP(hipMalloc(&c->d_counters, bbmsa::kCounterBytes));
    BBHIP(hipMemset(c->d_counters, 0, bbmsa::kCounterBytes));

    // generic kernel scratch: as many threads as a 2 GiB matrix budget allows (at least one wave)
    const long long planeInts = (long long)(cfg->maxRows + 1) * (cfg->maxColumns + 2);
    const long long perThread = 3 * planeInts * 4;
    long long budget = (long long)env_int("BBMSA_GENERIC_SCRATCH_MB", 2048) << 20;
    long long threads = budget / perThread;
    if (threads > 16384) threads = 16384;
    threads = (threads / 64) * 64;
    if (threads < 64) return bbfail(BBMAP_E_NOMEM, "bbmsa_create: BBMSA_GENERIC_SCRATCH_MB cannot hold one wavefront of scratch matrices for this maxRows x maxColumns");
    c->genThreads = (int)threads;
    BBHIP(hipMalloc(&c->d_matrix, (size_t)(threads * perThread)));
    BBHIP(hipMalloc(&c->d_limits, (size_t)(threads * (cfg->maxRows + cfg->maxColumns + 4) * 4)));
    // wide pass geometry (only when some windows can exceed the first pass's column buffer)
    if (cfg->maxColumns > fastCols) BBTRY(setup_wide_pass(c));
    // band kernel (msa_fill_band.hip) in front of the first pass: only without a band (a band changes the window rule);
    // BBMSA_NARROW=0 disables it (the switches keep the name of its predecessor, the one-job-per-lane narrow-window kernel)
    c->narrowSlack = env_int("BBMSA_NARROW_SLACK", 2000);
    if (!c->banded && env_int("BBMSA_NARROW", 1) != 0) {
        int perCU = 0;
        c->bandRows = cfg->maxRows < 256 ? cfg->maxRows : 256;
        c->bandLds = bbmsa::band_lds_bytes(c->tableLen, c->bandRows);
        if (c->bandLds > 64 * 1024) BBHIP(hipFuncSetAttribute(bbmsa::band_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, c->bandLds));
        BBHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, bbmsa::band_kernel(), 256, c->bandLds));
        if (perCU < 1) perCU = 1;
        if (perCU > 4) perCU = 4;
        c->narrowBlocks = c->numCUs * perCU;
        BBHIP(hipMalloc(&c->d_bandDir, (size_t)c->narrowBlocks * 4 * (size_t)(c->bandRows + 1) * 128 * 4));
    }
    // route switches of the environment (msa_ctx.h): defaults off, as the functions they mirror leave a context
    c->sortByWidth = env_int("BBMSA_SORT_BY_WIDTH", 0) != 0;
    c->sortWithBand = env_int("BBMSA_SORT_WITH_BAND", 0) != 0;
    c->wideUnlimited = env_int("BBMSA_WIDE_UNLIMITED", 0) != 0;
    c->unlimitedLoop = env_int("BBMSA_UNLIMITED_LOOP", 1) != 0;         // 0: the general build of the wavefront kernel takes every job
    // bbmsa_last_unlimited's counters cost every fill two or three atomics on the same few words: only on request
    c->unlimitedStats = env_int("BBMSA_UNLIMITED_STATS", 0) != 0 || getenv("BBMAP_DP_COUNTS") != nullptr;
    { const int lat = env_int("BBMSA_LATENCY_JOBS", 0); if (lat > 0) BBTRY(bbmsa_set_latency_jobs(c, lat)); }
    for (int i = 0; i < 4; i++) BBHIP(hipEventCreate(&c->ev[i]));
    guard.c = nullptr;
    *out = c;
    return BBMAP_OK;
}

extern "C" void bbmsa_destroy(bbmsa_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    bbmsa_legacy_destroy(c);
    if (c->d_dir) (void)hipFree(c->d_dir);
    if (c->d_counters) (void)hipFree(c->d_counters);
    if (c->d_widthHist) (void)hipFree(c->d_widthHist);
    for (DevBuf *b : {&c->slowList, &c->slowList2, &c->fastList, &c->gref, &c->gaux, &c->gjobs}) b->release();
    if (c->d_matrix) (void)hipFree(c->d_matrix);
    if (c->d_limits) (void)hipFree(c->d_limits);
    if (c->d_wideDir) (void)hipFree(c->d_wideDir);
    if (c->d_bandDir) (void)hipFree(c->d_bandDir);
    if (c->d_stripBoundary) (void)hipFree(c->d_stripBoundary);
    if (c->d_stripTmp) (void)hipFree(c->d_stripTmp);
    if (c->d_pipeBoundary) (void)hipFree(c->d_pipeBoundary);
    if (c->d_pipeSync) (void)hipFree(c->d_pipeSync);
    for (int i = 0; i < 4; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    delete c;
}

extern "C" int bbmsa_align_batch_device(bbmsa_ctx *c, void *stream_, int64_t n_jobs,
                                        const bbmsa_job *jobs, const uint8_t *reads, const uint8_t *refs,
                                        bbmsa_result *results, uint8_t *match, int32_t match_stride) {
    return bbmsa_align_impl(c, stream_, n_jobs, nullptr, jobs, reads, refs, results, match, match_stride);
}

extern "C" int bbmsa_align_batch_device_indirect(bbmsa_ctx *c, void *stream_, const uint32_t *n_jobs_dev, int64_t max_jobs,
                                                 const bbmsa_job *jobs, const uint8_t *reads, const uint8_t *refs,
                                                 bbmsa_result *results, uint8_t *match, int32_t match_stride) {
    if (!n_jobs_dev) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch_device_indirect: null counter");
    return bbmsa_align_impl(c, stream_, max_jobs, n_jobs_dev, jobs, reads, refs, results, match, match_stride);
}

namespace {
// the caller's arguments of one launch
struct Batch {
    int64_t n_jobs; const uint32_t *n_jobs_dev; const bbmsa_job *jobs; const uint8_t *reads, *refs; bbmsa_result *results; uint8_t *match;
    int32_t match_stride;
};
// what every kernel's parameter struct takes from the batch and the context
template <class P> void set_batch(P &p, const bbmsa_ctx *c, const Batch &B) {
    p.jobs = B.jobs; p.reads = B.reads; p.refs = B.refs; p.results = B.results; p.match = B.match;
    p.njobs = B.n_jobs; p.njobs_dev = B.n_jobs_dev; p.match_stride = B.match_stride;
    p.maxRows = c->cfg.maxRows; p.maxColumns = c->cfg.maxColumns; p.bandwidth = c->cfg.bandwidth; p.bandwidthRatio = c->cfg.bandwidthRatio;
}
// the last kernel of every launch: the one-job-per-thread kernel over the jobs the passes before it handed on
template <class S> int launch_generic(bbmsa_ctx *c, const Batch &B, hipStream_t stream, const int *list, const unsigned int *count) {
    bbmsa::GenericParams gp;
    set_batch(gp, c, B);
    gp.list = list; gp.list_count = count;
    gp.matrix = c->d_matrix; gp.limits = c->d_limits; gp.queue = c->d_counters + 2;
    hipLaunchKernelGGL(bbmsa::msa_fill_generic_kernel<S>, dim3(c->genThreads / 64), dim3(64), 0, stream, gp);
    BBHIP(hipGetLastError());
    BBHIP(hipEventRecord(c->ev[2], stream));
    c->timed = true;
    return BBMAP_OK;
}
}  // namespace

int bbmsa_align_impl(bbmsa_ctx *c, void *stream_, int64_t n_jobs, const uint32_t *n_jobs_dev,
                     const bbmsa_job *jobs, const uint8_t *reads, const uint8_t *refs,
                     bbmsa_result *results, uint8_t *match, int32_t match_stride) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch_device: null context");
    if (n_jobs < 0 || n_jobs > 0x7fffffffLL) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch_device: n_jobs out of range");
    if (n_jobs == 0) return BBMAP_OK;
    if (!jobs || !reads || !refs || !results) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch_device: null buffer");
    if (match && match_stride < 1) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch_device: match_stride must be positive");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->device));
    if (c->legacyOnly) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch_device: this context was created for bbmsa_fill_packed only (BBMSA_LEGACY_ONLY)");
    const Batch B = {n_jobs, n_jobs_dev, jobs, reads, refs, results, match, match_stride};
    const size_t listBytes = (size_t)n_jobs * 4;
    BBHIP(c->slowList.grow(listBytes, 0, &stream));
    int *const slowList = c->slowList.as<int>();
    if (c->scheme != BBMSA_SCHEME_11TS) {
        BBHIP(hipMemsetAsync(c->d_counters, 0, bbmsa::kCounterBytes, stream));
        c->narrowUsed = false; c->lastSorted = false; c->lastLatency = false; c->lastIndirect = n_jobs_dev != nullptr;
        BBHIP(hipEventRecord(c->ev[0], stream));
        BBHIP(hipEventRecord(c->ev[3], stream));
        bbmsa::StripParams sp;
        set_batch(sp, c, B);
        sp.queue = c->d_counters; sp.dirbuf = c->d_dir; sp.dir_slot_dwords = c->stripSlotDwords; sp.dir_strip_dwords = c->stripDwords;
        sp.boundary = c->d_stripBoundary; sp.tmpbuf = c->d_stripTmp; sp.slow_list = slowList; sp.slow_count = c->d_counters + 1;
        long long sblocks = n_jobs < c->stripBlocks ? n_jobs : c->stripBlocks;
        sp.pipeK = 0; sp.pipeSlots = 0; sp.pipeBoundary = nullptr; sp.pipeSync = nullptr;
        sp.pipeSpinLimit = env_int("BBMSA_PIPE_SPIN_LIMIT", 1 << 21);          // polls before a wave of the pipelined form gives up (~3 s; tests force timeouts)
        if (sp.pipeSpinLimit < 1) sp.pipeSpinLimit = 1;
        void *sargs[] = {&sp};
        if (!n_jobs_dev && c->pipeJobsMax > 0 && n_jobs <= c->pipeJobsMax) {
            // few jobs (the late scoreSlow rounds of mapPacBio): a lone 6,000 x 6,100 fill is one wavefront's dependent chain, 370 ms;
            // with its strips pipelined over `pipeK` wavefronts it is ~50
            const long long slots = n_jobs < c->pipeSlots ? n_jobs : c->pipeSlots;
            sp.pipeK = c->pipeK; sp.pipeSlots = (int)slots; sp.pipeBoundary = c->d_pipeBoundary; sp.pipeSync = c->d_pipeSync;
            BBHIP(hipMemsetAsync(c->d_pipeSync, 0, (size_t)(slots * bbmsa::strip_pipe_sync_ints(c->pipeK) * 4), stream));
            BBHIP(hipLaunchKernel(bbmsa::strip_kernel_pacbio_pipelined(), dim3((unsigned)(slots * c->pipeK)), dim3(64), sargs, (size_t)c->stripLds, stream));
        } else
        BBHIP(hipLaunchKernel(bbmsa::strip_kernel_pacbio(), dim3((unsigned)sblocks), dim3(64), sargs, (size_t)c->stripLds, stream));
        BBHIP(hipEventRecord(c->ev[1], stream));
        return launch_generic<bbmsa::Scheme9PacBio>(c, B, stream, slowList, c->d_counters + 1);
    }
    if (c->wideBlocks > 0) BBHIP(c->slowList2.grow(listBytes, 0, &stream));
    const bool useNarrow = c->narrowBlocks > 0 && !c->narrowOff;
    // Both the band kernel and the sort write the wavefront kernel's list.  Together only on request (bbmsa_sort_with_band): the sort
    // then gives the band kernel a list of its candidates, and the band kernel appends what it hands on behind the sorted list.
    const bool sortJobs = c->sortByWidth && !n_jobs_dev && n_jobs >= 256 && n_jobs > c->latencyJobs && (!useNarrow || c->sortWithBand);
    // (sorted: the general list with room for the band kernel's hand-overs, then the unlimited fills' list, then the candidates')
    if (c->narrowBlocks > 0 || sortJobs) BBHIP(c->fastList.grow(sortJobs ? 3 * listBytes : listBytes, 0, &stream));
    int *const fastList = c->fastList.as<int>();
    // counters: [0] fast queue, [1] slow count, [2] generic queue, [3] narrow queue, [4] fast-list count,
    //           [5] jobs finished by the band kernel (the "narrow" slots), [6] candidates it handed on, [7] wide pass's slow count,
    //           [8] wide queue, [9] jobs the wavefront kernel's prune-free loop ran, [10] unlimited jobs its general loop ran,
    //           [11] length of a width-sorted launch's list of unlimited jobs, [12] the unlimited build's queue,
    //           [13] / [14] wavefront steps of the unlimited jobs / of all jobs (bbmsa_last_unlimited),
    //           [15] length of a width-sorted launch's list of band candidates, [16] of its general list as the sort left it
    //           (before the band kernel's hand-overs), [17] steps the wavefronts ran (a wavefront steps as its longest job)
    BBHIP(hipMemsetAsync(c->d_counters, 0, bbmsa::kCounterBytes, stream));
    BBHIP(hipEventRecord(c->ev[0], stream));
    c->narrowUsed = useNarrow;
    if (sortJobs) {
        if (!c->d_widthHist) BBHIP(hipMalloc(&c->d_widthHist, bbmsa::WIDTH_BUCKETS * 4));
        BBHIP(hipMemsetAsync(c->d_widthHist, 0, bbmsa::WIDTH_BUCKETS * 4, stream));
        const int perBlock = bbmsa::SORT_THREADS * bbmsa::SORT_JOBS_PER_THREAD;
        const unsigned sb = (unsigned)((n_jobs + perBlock - 1) / perBlock);
        const bbmsa::SortKey key = {c->cfg.maxRows, c->cfg.maxColumns, c->cfg.bandwidth, c->cfg.bandwidthRatio, c->unlimitedLoop ? 1 : 0,
                                    useNarrow ? 1 : 0, c->bandRows, c->narrowSlack};
        hipLaunchKernelGGL(bbmsa::width_hist_kernel, dim3(sb), dim3(bbmsa::SORT_THREADS), 0, stream, jobs, (long long)n_jobs, key, c->d_widthHist);
        hipLaunchKernelGGL(bbmsa::width_scan_kernel, dim3(1), dim3(bbmsa::WIDTH_PER_CLASS), 0, stream, c->d_widthHist, c->d_counters + 4, c->d_counters + 16,
                           c->d_counters + 11, c->d_counters + 15);
        hipLaunchKernelGGL(bbmsa::width_scatter_kernel, dim3(sb), dim3(bbmsa::SORT_THREADS), 0, stream, jobs, (long long)n_jobs, key, c->d_widthHist,
                           fastList, fastList + n_jobs, fastList + 2 * n_jobs);
        BBHIP(hipGetLastError());
    }
    if (useNarrow) {
        bbmsa::NarrowParams np;
        set_batch(np, c, B);
        np.queue = c->d_counters + 3; np.fast_list = fastList; np.fast_count = c->d_counters + 4;
        np.stats = c->d_counters + 5; np.maxSlack = c->narrowSlack;
        np.dirbuf32 = c->d_bandDir; np.tableLen = c->tableLen; np.bandRows = c->bandRows;
        np.list = sortJobs ? fastList + 2 * n_jobs : nullptr; np.list_count = sortJobs ? c->d_counters + 15 : nullptr;
        long long nb = (n_jobs + 63) / 64;
        if (nb > c->narrowBlocks) nb = c->narrowBlocks;
        void *nargs[] = {&np};
        BBHIP(hipLaunchKernel(bbmsa::band_kernel(), dim3((unsigned)nb), dim3(256), nargs, (size_t)c->bandLds, stream));
    }
    BBHIP(hipEventRecord(c->ev[3], stream));

    bbmsa::FillParams fp = {};
    set_batch(fp, c, B);
    fp.queue = c->d_counters; fp.dirbuf = c->d_dir; fp.dir_slot_dwords = c->dirSlotDwords;
    fp.list = (useNarrow || sortJobs) ? fastList : nullptr; fp.list_count = c->d_counters + 4; fp.priority = 0;
    fp.slow_list = slowList; fp.slow_count = c->d_counters + 1;
    fp.lanesPerJob = c->G; fp.fastCols = c->fastCols; fp.tmpBytes = c->tmpBytes; fp.tableLen = c->tableLen;
    fp.unl_stats = c->unlimitedStats ? c->d_counters + 9 : nullptr;

    // A launch with few jobs is a wavefront's latency, not throughput: (columns + lanes - 1) steps of one dependent chain.  The wide
    // pass's geometry (64 lanes x 3 rows, one job per block) has the shorter chain per step (3 rows instead of 5: ~450 instead of
    // ~740 instructions), so such launches go to it directly (bbmsa_set_latency_jobs; the mapper's late rounds hold a few hundred fills).
    const bool latency = c->wideBlocks > 0 && !n_jobs_dev && !useNarrow && n_jobs <= c->latencyJobs;
    c->lastSorted = sortJobs; c->lastLatency = latency; c->lastIndirect = n_jobs_dev != nullptr; c->lastJobs = n_jobs;
    const int jobsPerBlock = 4 * (64 / c->G);
    long long blocks = (n_jobs + jobsPerBlock - 1) / jobsPerBlock;
    if (blocks > c->blocks) blocks = c->blocks;
    if (sortJobs && c->unlimitedLoop) {
        // the sort made a list of the unlimited fills: the build without limits and prune tests takes them, the general build the rest
        bbmsa::FillParams up = fp;
        up.queue = c->d_counters + 12; up.list = fastList + n_jobs; up.list_count = c->d_counters + 11;
        void *uargs[] = {&up};
        BBHIP(hipLaunchKernel(bbmsa::fast_kernel_unl_for(c->R), dim3((unsigned)blocks), dim3(256), uargs, (size_t)c->ldsBytes, stream));
    }
    void *args[] = {&fp};
    if (!latency)
        BBHIP(hipLaunchKernel(bbmsa::fast_kernel_for(c->R, c->banded), dim3((unsigned)blocks), dim3(256), args, (size_t)c->ldsBytes, stream));
    const int *genList = slowList;
    const unsigned int *genCount = c->d_counters + 1;
    if (c->wideBlocks > 0) {
        // wide pass over the first pass's hand-overs; what it cannot take either (banded rows with holes) goes on to the
        // generic kernel through the second list ([7] = its count, [8] = wide queue)
        bbmsa::FillParams wp = fp;
        wp.queue = c->d_counters + 8; wp.dirbuf = c->d_wideDir; wp.dir_slot_dwords = c->wideDirSlotDwords;
        wp.list = slowList; wp.list_count = c->d_counters + 1;
        if (latency) { wp.list = nullptr; wp.list_count = nullptr; }          // every job of the launch
        wp.slow_list = c->slowList2.as<int>(); wp.slow_count = c->d_counters + 7;
        wp.lanesPerJob = 64; wp.fastCols = c->wideCols; wp.tmpBytes = c->wideTmpBytes; wp.tableLen = c->wideTableLen;
        static const int widePrio = env_int("BBMSA_WIDE_PRIORITY", 2);
        wp.priority = widePrio;
        void *wargs[] = {&wp};
        const long long wblocks = latency && n_jobs < c->wideBlocks ? n_jobs : c->wideBlocks;
        // one job per wavefront: which step loop runs is wave-uniform, so one build can hold both and give an unlimited fill the
        // prune-free one (bbmsa_set_wide_unlimited; a banded context has no such build)
        const void *bothFn = (c->wideUnlimited && !c->banded) ? bbmsa::fast_kernel_both_for(c->wideR) : nullptr;
        BBHIP(hipLaunchKernel(bothFn ? bothFn : bbmsa::fast_kernel_for(c->wideR, c->banded), dim3((unsigned)wblocks), dim3(64), wargs, (size_t)c->wideLdsBytes, stream));
        genList = wp.slow_list; genCount = c->d_counters + 7;
    }
    BBHIP(hipEventRecord(c->ev[1], stream));
    return launch_generic<bbmsa::Scheme11ts>(c, B, stream, genList, genCount);
}

void bbmsa_use_narrow(bbmsa_ctx *c, bool on) { if (c) c->narrowOff = !on; }
void bbmsa_sort_by_width(bbmsa_ctx *c, bool on) { if (c) c->sortByWidth = on; }
void bbmsa_sort_with_band(bbmsa_ctx *c, bool on) { if (c) c->sortWithBand = on; }
void bbmsa_set_wide_unlimited(bbmsa_ctx *c, bool on) { if (c) c->wideUnlimited = on; }
int bbmsa_set_latency_jobs(bbmsa_ctx *c, int64_t n) {
    if (!c || c->scheme != BBMSA_SCHEME_11TS || c->legacyOnly) return BBMAP_OK;
    BBHIP(hipSetDevice(c->device));
    if (n > 0) BBTRY(setup_wide_pass(c));
    if (n > 0 && !c->slowList2.p) BBHIP(c->slowList2.grow(c->slowList.cap));   // (its hand-over list, late: as long as the first)
    c->latencyJobs = c->wideBlocks > 0 ? n : 0;
    return BBMAP_OK;
}
int bbmsa_wait_first_pass(bbmsa_ctx *c, void *waiter) {
    if (!c || !c->timed) return BBMAP_OK;
    BBHIP(hipStreamWaitEvent((hipStream_t)waiter, c->ev[3], 0));       // recorded right in front of the last launch's first pass
    return BBMAP_OK;
}

extern "C" int bbmsa_last_kernel_ms(bbmsa_ctx *c, float *ms_fast, float *ms_slow) {
    if (!c || !c->timed) return bbfail(BBMAP_E_ARG, "bbmsa_last_kernel_ms: nothing launched yet");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    float a = 0, b = 0;
    BBHIP(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    BBHIP(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    if (ms_fast) *ms_fast = a;
    if (ms_slow) *ms_slow = b;
    return BBMAP_OK;
}

extern "C" int bbmsa_last_kernel_ms3(bbmsa_ctx *c, float *ms3) {
    if (!c || !c->timed || !ms3) return bbfail(BBMAP_E_ARG, "bbmsa_last_kernel_ms3: nothing launched yet");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    BBHIP(hipEventElapsedTime(&ms3[0], c->ev[0], c->ev[3]));
    BBHIP(hipEventElapsedTime(&ms3[1], c->ev[3], c->ev[1]));
    BBHIP(hipEventElapsedTime(&ms3[2], c->ev[1], c->ev[2]));
    return BBMAP_OK;
}

extern "C" int bbmsa_last_counts(bbmsa_ctx *c, int64_t *counts4) {
    if (!c || !c->timed || !counts4) return bbfail(BBMAP_E_ARG, "bbmsa_last_counts: nothing launched yet");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    unsigned h[bbmsa::kCounterWords];
    BBHIP(hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    // the wavefront list: what the band kernel left to the wavefront kernel without trying it, plus what it handed on -- on a sorted
    // launch the sort's general and unlimited lists, which hold no candidate (finished + handed on + this = the launch's jobs)
    counts4[0] = h[5]; counts4[1] = h[6]; counts4[2] = c->narrowUsed ? (c->lastSorted ? h[16] + h[11] : h[4]) : 0; counts4[3] = c->wideBlocks > 0 ? h[7] : h[1];
    if (getenv("BBMAP_DP_COUNTS")) {
        if (c->wideBlocks > 0) fprintf(stderr, "   (first pass handed %u jobs to the wide pass)\n", h[1]);
        if (c->lastSorted) fprintf(stderr, "   (sorted: %u general, %u unlimited, %u band candidates)\n", h[16], h[11], h[15]);
        fprintf(stderr, "   (the wavefronts ran %u steps)\n", h[17]);
    }
    return BBMAP_OK;
}

// Test hook: the three lists the last launch's width sort made, as `n_jobs` ints each in lists3 (general, unlimited, band candidates;
// entries past a list's length are not written) and their lengths in lens3.  Fails when the last launch was not sorted.
extern "C" int bbmsa_debug_sorted_lists(bbmsa_ctx *c, int64_t n_jobs, int32_t *lists3, int64_t *lens3) {
    if (!c || !c->timed || !lists3 || !lens3) return bbfail(BBMAP_E_ARG, "bbmsa_debug_sorted_lists: nothing launched yet");
    if (!c->lastSorted || n_jobs != c->lastJobs) return bbfail(BBMAP_E_ARG, "bbmsa_debug_sorted_lists: the last launch was not a sorted launch of n_jobs jobs");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    unsigned h[bbmsa::kCounterWords];
    BBHIP(hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    const unsigned len[3] = {h[16], h[11], h[15]};
    for (int k = 0; k < 3; k++) {
        if ((int64_t)len[k] > n_jobs) return bbfail(BBMAP_E_HIP, "bbmsa_debug_sorted_lists: a list is longer than the launch");
        lens3[k] = len[k];
        if (len[k]) BBHIP(hipMemcpy(lists3 + (size_t)k * (size_t)n_jobs, c->fastList.as<int>() + (size_t)k * (size_t)n_jobs, (size_t)len[k] * 4, hipMemcpyDeviceToHost));
    }
    return BBMAP_OK;
}

extern "C" int bbmsa_last_unlimited(bbmsa_ctx *c, int64_t *counts4) {
    if (!c || !c->timed || !counts4) return bbfail(BBMAP_E_ARG, "bbmsa_last_unlimited: nothing launched yet");
    if (c->scheme == BBMSA_SCHEME_11TS && !c->legacyOnly && !c->unlimitedStats) return bbfail(BBMAP_E_ARG, "bbmsa_last_unlimited: the context does not count (create it with BBMSA_UNLIMITED_STATS=1 in the environment)");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    unsigned h[16];
    BBHIP(hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    const bool wave = c->scheme == BBMSA_SCHEME_11TS && !c->legacyOnly;
    counts4[0] = wave ? h[9] : 0; counts4[1] = wave ? h[10] : 0; counts4[2] = wave ? h[13] : 0; counts4[3] = wave ? h[14] : 0;
    return BBMAP_OK;
}

int bbmsa_last_route_flags(const bbmsa_ctx *c) {
    if (!c || !c->timed) return 0;
    return (c->narrowUsed ? BBMSA_ROUTE_NARROW : 0) | (c->lastSorted ? BBMSA_ROUTE_SORTED : 0) | (c->lastLatency ? BBMSA_ROUTE_LATENCY : 0);
}

extern "C" int bbmsa_last_route(bbmsa_ctx *c, int64_t *route8) {
    if (!c || !c->timed || !route8) return bbfail(BBMAP_E_ARG, "bbmsa_last_route: nothing launched yet");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    unsigned h[16];
    BBHIP(hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    const bool wide = c->scheme == BBMSA_SCHEME_11TS && c->wideBlocks > 0;
    route8[0] = c->narrowUsed; route8[1] = c->lastSorted; route8[2] = c->lastLatency; route8[3] = wide; route8[4] = c->lastIndirect;
    route8[5] = h[1]; route8[6] = wide ? h[7] : 0; route8[7] = c->narrowUsed ? h[5] : 0;
    return BBMAP_OK;
}

extern "C" int bbmsa_geometry(bbmsa_ctx *c, int32_t *geo4) {
    if (!c || !geo4) return bbfail(BBMAP_E_ARG, "bbmsa_geometry: null argument");
    geo4[0] = geo4[1] = geo4[2] = geo4[3] = 0;
    if (c->legacy) {
        int last = 0, mask = 0;
        bbmsa_legacy_rows_per_lane(c, &last, &mask);
        geo4[0] = 64; geo4[1] = last; geo4[2] = c->cfg.maxColumns; geo4[3] = mask;
    } else if (c->scheme == BBMSA_SCHEME_11TS) {
        geo4[0] = c->G; geo4[1] = c->R; geo4[2] = c->fastCols; geo4[3] = c->wideBlocks > 0 ? c->wideR : 0;
    }
    return BBMAP_OK;
}

extern "C" int bbmsa_align_batch(bbmsa_ctx *c, int64_t n_jobs, const bbmsa_job *jobs,
                                 const uint8_t *reads, int64_t reads_bytes,
                                 const uint8_t *refs, int64_t refs_bytes,
                                 bbmsa_result *results, uint8_t *match, int32_t match_stride) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmsa_align_batch: null context");
    if (n_jobs == 0) return BBMAP_OK;
    if (n_jobs < 0 || !jobs || !reads || !refs || !results || reads_bytes < 0 || refs_bytes < 0)
        return bbfail(BBMAP_E_ARG, "bbmsa_align_batch: bad argument");
    BBHIP(hipSetDevice(c->device));
    // every job must stay inside the buffers it was given
    for (int64_t i = 0; i < n_jobs; i++) {
        const bbmsa_job &j = jobs[i];
        if (j.read_len < 0 || j.read_off < 0 || j.read_off + j.read_len > reads_bytes)
            return bbfail(BBMAP_E_ARG, "bbmsa_align_batch: a read lies outside the reads buffer");
        if (j.ref_len < 0 || j.ref_off < 0 || j.ref_off + j.ref_len > refs_bytes)
            return bbfail(BBMAP_E_ARG, "bbmsa_align_batch: a reference array lies outside the refs buffer");
        if (!(j.flags & BBMSA_CLAMP_WINDOW) && (j.refStartLoc < 0 || j.refEndLoc >= j.ref_len))
            return bbfail(BBMAP_E_ARG, "bbmsa_align_batch: window outside its reference array (set BBMSA_CLAMP_WINDOW to clamp)");
    }
    DevTmp<bbmsa_job> d_jobs; DevTmp<uint8_t> d_reads, d_refs, d_match; DevTmp<bbmsa_result> d_res;
    BBTRY(d_jobs.upload(jobs, (size_t)n_jobs));
    BBTRY(d_reads.upload(reads, (size_t)reads_bytes));
    BBTRY(d_refs.upload(refs, (size_t)refs_bytes));
    BBTRY(d_res.alloc((size_t)n_jobs));
    if (match) BBTRY(d_match.alloc((size_t)n_jobs * (size_t)match_stride));
    BBHIP(hipMemset(d_res, 0xff, (size_t)n_jobs * sizeof(bbmsa_result)));
    BBTRY(bbmsa_align_batch_device(c, nullptr, n_jobs, d_jobs, d_reads, d_refs, d_res, d_match, match_stride));
    BBHIP(hipStreamSynchronize(nullptr));
    BBHIP(hipMemcpy(results, d_res, (size_t)n_jobs * sizeof(bbmsa_result), hipMemcpyDeviceToHost));
    if (match) BBHIP(hipMemcpy(match, d_match, (size_t)n_jobs * (size_t)match_stride, hipMemcpyDeviceToHost));
    return BBMAP_OK;
}
