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
template <class S> __global__ void msa_fill_generic_kernel(const GenericParams p);
const void *band_kernel();                                     // msa_fill_band.hip
int band_lds_bytes(int tableLen, int bandRows);
}  // namespace bbmsa

static int clamp_occupancy(int per, int most) { return per < 1 ? 1 : (per > most ? most : per); }

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
    const void *wfn = bbmsa::fast_kernel_for(c->wideR, c->sw.banded);
    if (wfn && c->wideLdsBytes <= 160 * 1024) {
        if (c->wideLdsBytes > 64 * 1024) BBHIP(hipFuncSetAttribute(wfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->wideLdsBytes));
        const void *bfn = c->sw.banded ? nullptr : bbmsa::fast_kernel_both_for(c->wideR);      // (bbmsa_set_wide_unlimited)
        if (bfn && c->wideLdsBytes > 64 * 1024) BBHIP(hipFuncSetAttribute(bfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->wideLdsBytes));
        int per = 0;
        BBHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, wfn, 64, c->wideLdsBytes));
        per = clamp_occupancy(per, 8);
        const long long slotDwords = (long long)(((c->wideCols + 64 - 1) >> 3) + 1) * c->wideR * 64;
        BBHIP(hipMalloc(&c->d_wideDir, (size_t)((long long)c->numCUs * per * slotDwords * 4)));
        c->wideDirSlotDwords = slotDwords;
        c->wideBlocks = c->numCUs * per;
        c->sw.widePresent = true;
    }
    return BBMAP_OK;
}

// The generic kernel's scratch, one slot per thread (three score planes and the two limit arrays).  Threads: as many as the matrix
// budget allows (BBMSA_GENERIC_SCRATCH_MB, `defaultMB` without it), whole wavefronts, at most `mostThreads`.
static int generic_threads(const bbmsa_config &cfg, int defaultMB, long long mostThreads, int *out) {
    const long long perThread = 3LL * (cfg.maxRows + 1) * (cfg.maxColumns + 2) * 4;
    long long threads = ((long long)env_int("BBMSA_GENERIC_SCRATCH_MB", defaultMB) << 20) / perThread;
    if (threads > mostThreads) threads = mostThreads;
    threads = (threads / 64) * 64;
    if (threads < 64) return bbfail(BBMAP_E_NOMEM, "bbmsa_create: BBMSA_GENERIC_SCRATCH_MB cannot hold one wavefront of scratch matrices for this maxRows x maxColumns");
    *out = (int)threads;
    return BBMAP_OK;
}
static int alloc_generic_scratch(bbmsa_ctx *c, int threads) {
    c->genThreads = threads;
    BBHIP(hipMalloc(&c->d_matrix, (size_t)threads * 3 * (size_t)(c->cfg.maxRows + 1) * (size_t)(c->cfg.maxColumns + 2) * 4));
    BBHIP(hipMalloc(&c->d_limits, (size_t)threads * (size_t)(c->cfg.maxRows + c->cfg.maxColumns + 4) * 4));
    return BBMAP_OK;
}

// a context for bbmsa_fill_packed only (the per-call JNI shape): one scratch matrix, no batch buffers
static int create_legacy_only(bbmsa_ctx *c) {
    BBTRY(alloc_generic_scratch(c, 1));
    return bbmsa_legacy_create(c);
}

// 9PacBio: the strip-tiled wavefront kernel (msa_fill_strip.hip), one alignment per wavefront; banded fills and windows narrower
// than the read are handed to the one-job-per-thread kernel
static int create_pacbio(bbmsa_ctx *c) {
    const bbmsa_config *cfg = &c->cfg;
    int threads = 0;
    BBTRY(generic_threads(*cfg, 40960, 4096, &threads));          // 6019 x 7600 (mapPacBio) needs 35 GB for one wavefront of matrices
    BBTRY(alloc_generic_scratch(c, threads));
    const int R = bbmsa::strip_rows_per_lane();
    c->stripLds = (cfg->maxColumns + 2) * 4 + ((cfg->maxColumns + 2 + 7) & ~7);     // horizLimit ints + reference bytes
    const void *kfn = bbmsa::strip_kernel_pacbio();
    if (c->stripLds > 64 * 1024) BBHIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, c->stripLds));
    // Resident wavefronts per CU, from the LDS a wavefront takes (160 KB per CU; the kernel holds ~128 VGPRs, up to 4 waves per
    // SIMD, so LDS is what limits it).  Not asked of hipOccupancyMaxActiveBlocksPerMultiprocessor: that query was seen to fail with
    // hipErrorUnknown depending on what the process had done before (after the CPU oracle had run in it), for reasons the
    // runtime's log does not give; nothing here depends on the exact figure (the pipelined form no longer assumes co-residency).
    const int per = clamp_occupancy((160 * 1024) / (c->stripLds + 512), 8);
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
        c->pipeK = strips;
        c->pipeSlots = (c->numCUs * per) / strips;                  // every wavefront of every slot is resident: the hand-shakes need it
        if (c->pipeSlots > c->stripBlocks) c->pipeSlots = c->stripBlocks;
        if (c->pipeSlots > 256) c->pipeSlots = 256;
        c->sw.pipeJobsMax = env_int("BBMSA_STRIP_PIPE_JOBS", 512);  // launches with at most this many jobs take the pipelined form
        if (strips < 2 || c->pipeSlots < 1) c->sw.pipeJobsMax = 0;
        if (c->sw.pipeJobsMax > 0) {
            BBHIP(hipMalloc(&c->d_pipeBoundary, (size_t)((long long)c->pipeSlots * strips * 3 * (cfg->maxColumns + 2) * 4)));
            BBHIP(hipMalloc(&c->d_pipeSync, (size_t)((long long)c->pipeSlots * bbmsa::strip_pipe_sync_ints(strips) * 4)));
        }
    }
    BBHIP(hipMalloc(&c->d_dir, (size_t)((long long)c->stripBlocks * c->stripSlotDwords * 4)));
    BBHIP(hipMalloc(&c->d_stripBoundary, (size_t)((long long)c->stripBlocks * 6 * (cfg->maxColumns + 2) * 4)));
    BBHIP(hipMalloc(&c->d_stripTmp, (size_t)((long long)c->stripBlocks * (cfg->maxRows + cfg->maxColumns + 8))));
    return BBMAP_OK;
}

// 11ts: the wavefront kernel's first pass, the wide pass behind it where windows can exceed its buffer, the band kernel in front
static int create_11ts(bbmsa_ctx *c) {
    const bbmsa_config *cfg = &c->cfg;
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

    c->sw.banded = !(cfg->bandwidth < 1 && cfg->bandwidthRatio <= 0.0f);
    const void *kfn = bbmsa::fast_kernel_for(c->R, c->sw.banded);
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

    int threads = 0;
    BBTRY(generic_threads(*cfg, 2048, 16384, &threads));
    BBTRY(alloc_generic_scratch(c, threads));
    // wide pass geometry (only when some windows can exceed the first pass's column buffer)
    if (cfg->maxColumns > fastCols) BBTRY(setup_wide_pass(c));
    // band kernel (msa_fill_band.hip) in front of the first pass: only without a band (a band changes the window rule);
    // BBMSA_NARROW=0 disables it (the switches keep the name of its predecessor, the one-job-per-lane narrow-window kernel)
    c->narrowSlack = env_int("BBMSA_NARROW_SLACK", 2000);
    if (!c->sw.banded && env_int("BBMSA_NARROW", 1) != 0) {
        int perCU = 0;
        c->bandRows = cfg->maxRows < 256 ? cfg->maxRows : 256;
        c->bandLds = bbmsa::band_lds_bytes(c->tableLen, c->bandRows);
        if (c->bandLds > 64 * 1024) BBHIP(hipFuncSetAttribute(bbmsa::band_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, c->bandLds));
        BBHIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, bbmsa::band_kernel(), 256, c->bandLds));
        c->narrowBlocks = c->numCUs * clamp_occupancy(perCU, 4);
        c->sw.bandPresent = true;
        BBHIP(hipMalloc(&c->d_bandDir, (size_t)c->narrowBlocks * 4 * (size_t)(c->bandRows + 1) * 128 * 4));
    }
    // route switches of the environment (msa_ctx.h): defaults off, as the functions they mirror leave a context
    c->sw.sortByWidth = env_int("BBMSA_SORT_BY_WIDTH", 0) != 0;
    c->sw.sortWithBand = env_int("BBMSA_SORT_WITH_BAND", 0) != 0;
    c->sw.wideUnlimited = env_int("BBMSA_WIDE_UNLIMITED", 0) != 0;
    c->sw.unlimitedLoop = env_int("BBMSA_UNLIMITED_LOOP", 1) != 0;      // 0: the general build of the wavefront kernel takes every job
    // bbmsa_last_unlimited's counters cost every fill two or three atomics on the same few words: only on request
    c->unlimitedStats = env_int("BBMSA_UNLIMITED_STATS", 0) != 0 || getenv("BBMAP_DP_COUNTS") != nullptr;
    { const int lat = env_int("BBMSA_LATENCY_JOBS", 0); if (lat > 0) BBTRY(bbmsa_set_latency_jobs(c, lat)); }
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
    c->sw.scheme = scheme;
    c->legacyOnly = legacyOnly;
    // every failure below leaves through bbmsa_destroy(c): nothing allocated so far is leaked
    struct Guard { bbmsa_ctx *c; ~Guard() { if (c) bbmsa_destroy(c); } } guard{c};
    BBTRY(legacyOnly ? create_legacy_only(c) : scheme != BBMSA_SCHEME_11TS ? create_pacbio(c) : create_11ts(c));
    BBHIP(hipMalloc(&c->d_counters, bbmsa::kCounterBytes));
    BBHIP(hipMemset(c->d_counters, 0, bbmsa::kCounterBytes));
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

// The steps of one launch sequence, in the order bbmsa_align_impl runs them.  Each takes the launch's Route (msa_route.h).
namespace {
using namespace bbmsa;

// the last kernel of every launch: the one-job-per-thread kernel over the jobs the passes before it handed on
template <class S> int launch_generic(bbmsa_ctx *c, const JobBatch &B, hipStream_t stream, const int *list, const unsigned int *count) {
    bbmsa::GenericParams gp;
    set_batch(gp, c, B);
    gp.list = list; gp.list_count = count;
    gp.matrix = c->d_matrix; gp.limits = c->d_limits; gp.queue = c->d_counters + CNT_GENERIC_QUEUE;
    hipLaunchKernelGGL(bbmsa::msa_fill_generic_kernel<S>, dim3(c->genThreads / 64), dim3(64), 0, stream, gp);
    BBHIP(hipGetLastError());
    BBHIP(hipEventRecord(c->ev[2], stream));
    c->timed = true;
    return BBMAP_OK;
}

// 9PacBio's first kernel: a job per wavefront, or (Route::pipelined) a job's strips over pipeK wavefronts
int launch_strip(bbmsa_ctx *c, const JobBatch &B, const Route &r, hipStream_t stream) {
    bbmsa::StripParams sp;
    set_batch(sp, c, B);
    sp.queue = c->d_counters + CNT_FAST_QUEUE; sp.dirbuf = c->d_dir; sp.dir_slot_dwords = c->stripSlotDwords; sp.dir_strip_dwords = c->stripDwords;
    sp.boundary = c->d_stripBoundary; sp.tmpbuf = c->d_stripTmp; sp.slow_list = c->slowList.as<int>(); sp.slow_count = c->d_counters + CNT_SLOW_COUNT;
    sp.pipeK = 0; sp.pipeSlots = 0; sp.pipeBoundary = nullptr; sp.pipeSync = nullptr;
    sp.pipeSpinLimit = env_int("BBMSA_PIPE_SPIN_LIMIT", 1 << 21);          // polls before a wave of the pipelined form gives up (~3 s; tests force timeouts)
    if (sp.pipeSpinLimit < 1) sp.pipeSpinLimit = 1;
    void *sargs[] = {&sp};
    if (r.pipelined) {
        const long long slots = r.jobs < c->pipeSlots ? r.jobs : c->pipeSlots;
        sp.pipeK = c->pipeK; sp.pipeSlots = (int)slots; sp.pipeBoundary = c->d_pipeBoundary; sp.pipeSync = c->d_pipeSync;
        BBHIP(hipMemsetAsync(c->d_pipeSync, 0, (size_t)(slots * bbmsa::strip_pipe_sync_ints(c->pipeK) * 4), stream));
        BBHIP(hipLaunchKernel(bbmsa::strip_kernel_pacbio_pipelined(), dim3((unsigned)(slots * c->pipeK)), dim3(64), sargs, (size_t)c->stripLds, stream));
        return BBMAP_OK;
    }
    const long long sblocks = r.jobs < c->stripBlocks ? r.jobs : c->stripBlocks;
    BBHIP(hipLaunchKernel(bbmsa::strip_kernel_pacbio(), dim3((unsigned)sblocks), dim3(64), sargs, (size_t)c->stripLds, stream));
    return BBMAP_OK;
}

// the band kernel in front of the first pass: over every job, or over the sort's list of candidates (the third of fastList)
int launch_band(bbmsa_ctx *c, const JobBatch &B, const Route &r, hipStream_t stream) {
    int *const fastList = c->fastList.as<int>();
    bbmsa::NarrowParams np;
    set_batch(np, c, B);
    np.queue = c->d_counters + CNT_BAND_QUEUE; np.fast_list = fastList; np.fast_count = c->d_counters + CNT_LIST_COUNT;
    np.stats = c->d_counters + CNT_BAND_STATS; np.maxSlack = c->narrowSlack;
    np.dirbuf32 = c->d_bandDir; np.tableLen = c->tableLen; np.bandRows = c->bandRows;
    np.list = r.sorted ? fastList + 2 * r.jobs : nullptr; np.list_count = r.sorted ? c->d_counters + CNT_CAND_COUNT : nullptr;
    long long nb = (r.jobs + 63) / 64;
    if (nb > c->narrowBlocks) nb = c->narrowBlocks;
    void *nargs[] = {&np};
    BBHIP(hipLaunchKernel(bbmsa::band_kernel(), dim3((unsigned)nb), dim3(256), nargs, (size_t)c->bandLds, stream));
    return BBMAP_OK;
}

// what the first pass takes; the unlimited build's launch and the 64-lane launch start from a copy
bbmsa::FillParams first_pass_params(const bbmsa_ctx *c, const JobBatch &B, const Route &r) {
    bbmsa::FillParams fp = {};
    set_batch(fp, c, B);
    fp.queue = c->d_counters + CNT_FAST_QUEUE; fp.dirbuf = c->d_dir; fp.dir_slot_dwords = c->dirSlotDwords;
    fp.list = (r.band || r.sorted) ? c->fastList.as<int>() : nullptr; fp.list_count = c->d_counters + CNT_LIST_COUNT; fp.priority = 0;
    fp.slow_list = c->slowList.as<int>(); fp.slow_count = c->d_counters + CNT_SLOW_COUNT;
    fp.lanesPerJob = c->G; fp.fastCols = c->fastCols; fp.tmpBytes = c->tmpBytes; fp.tableLen = c->tableLen;
    fp.unl_stats = c->unlimitedStats ? c->d_counters + CNT_UNL_STATS : nullptr;
    return fp;
}

// the build without limits and prune tests, over the sort's list of unlimited fills (the second third of fastList)
int launch_unlimited(bbmsa_ctx *c, const bbmsa::FillParams &fp, const Route &r, long long blocks, hipStream_t stream) {
    bbmsa::FillParams up = fp;
    up.queue = c->d_counters + CNT_UNL_QUEUE; up.list = c->fastList.as<int>() + r.jobs; up.list_count = c->d_counters + CNT_UNL_LIST_COUNT;
    void *uargs[] = {&up};
    BBHIP(hipLaunchKernel(bbmsa::fast_kernel_unl_for(c->R), dim3((unsigned)blocks), dim3(256), uargs, (size_t)c->ldsBytes, stream));
    return BBMAP_OK;
}

// The 64-lane geometry: the wide pass over the first pass's hand-overs or, on the latency route, over every job of the launch.  What
// it cannot take either (banded rows with holes) goes on to the generic kernel through the second list.
int launch_wide(bbmsa_ctx *c, const bbmsa::FillParams &fp, const Route &r, hipStream_t stream) {
    bbmsa::FillParams wp = fp;
    wp.queue = c->d_counters + CNT_WIDE_QUEUE; wp.dirbuf = c->d_wideDir; wp.dir_slot_dwords = c->wideDirSlotDwords;
    wp.list = r.latency ? nullptr : fp.slow_list; wp.list_count = r.latency ? nullptr : fp.slow_count;
    wp.slow_list = c->slowList2.as<int>(); wp.slow_count = c->d_counters + CNT_WIDE_SLOW_COUNT;
    wp.lanesPerJob = 64; wp.fastCols = c->wideCols; wp.tmpBytes = c->wideTmpBytes; wp.tableLen = c->wideTableLen;
    static const int widePrio = env_int("BBMSA_WIDE_PRIORITY", 2);
    wp.priority = widePrio;
    void *wargs[] = {&wp};
    const long long wblocks = r.latency && r.jobs < c->wideBlocks ? r.jobs : c->wideBlocks;
    const void *bothFn = r.wideBoth ? bbmsa::fast_kernel_both_for(c->wideR) : nullptr;      // null: no such build, the general one runs
    BBHIP(hipLaunchKernel(bothFn ? bothFn : bbmsa::fast_kernel_for(c->wideR, c->sw.banded), dim3((unsigned)wblocks), dim3(64), wargs, (size_t)c->wideLdsBytes, stream));
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
    const JobBatch B = {n_jobs, n_jobs_dev, jobs, reads, refs, results, match, match_stride};
    const Route r = plan_route(c->sw, n_jobs, n_jobs_dev != nullptr);
    const size_t listBytes = (size_t)n_jobs * 4;
    BBHIP(c->slowList.grow(listBytes, 0, &stream));
    if (r.wide) BBHIP(c->slowList2.grow(listBytes, 0, &stream));
    // (sorted: the general list with room for the band kernel's hand-overs, then the unlimited fills' list, then the candidates')
    if (c->sw.bandPresent || r.sorted) BBHIP(c->fastList.grow(r.sorted ? 3 * listBytes : listBytes, 0, &stream));
    BBHIP(hipMemsetAsync(c->d_counters, 0, bbmsa::kCounterBytes, stream));
    c->last = r;
    BBHIP(hipEventRecord(c->ev[0], stream));
    if (c->sw.scheme != BBMSA_SCHEME_11TS) {
        BBHIP(hipEventRecord(c->ev[3], stream));
        BBTRY(launch_strip(c, B, r, stream));
        BBHIP(hipEventRecord(c->ev[1], stream));
        return launch_generic<bbmsa::Scheme9PacBio>(c, B, stream, c->slowList.as<int>(), c->d_counters + CNT_SLOW_COUNT);
    }
    if (r.sorted) BBTRY(bbmsa_width_sort(c, stream, jobs, n_jobs, r.band));
    if (r.band) BBTRY(launch_band(c, B, r, stream));
    BBHIP(hipEventRecord(c->ev[3], stream));
    bbmsa::FillParams fp = first_pass_params(c, B, r);
    const int jobsPerBlock = 4 * (64 / c->G);
    long long blocks = (n_jobs + jobsPerBlock - 1) / jobsPerBlock;
    if (blocks > c->blocks) blocks = c->blocks;
    if (r.unlList) BBTRY(launch_unlimited(c, fp, r, blocks, stream));
    void *args[] = {&fp};
    if (!r.latency)
        BBHIP(hipLaunchKernel(bbmsa::fast_kernel_for(c->R, c->sw.banded), dim3((unsigned)blocks), dim3(256), args, (size_t)c->ldsBytes, stream));
    if (r.wide) BBTRY(launch_wide(c, fp, r, stream));
    BBHIP(hipEventRecord(c->ev[1], stream));
    return launch_generic<bbmsa::Scheme11ts>(c, B, stream, r.wide ? c->slowList2.as<int>() : fp.slow_list,
                                             c->d_counters + (r.wide ? CNT_WIDE_SLOW_COUNT : CNT_SLOW_COUNT));
}

void bbmsa_use_narrow(bbmsa_ctx *c, bool on) { if (c) c->sw.bandOff = !on; }
void bbmsa_sort_by_width(bbmsa_ctx *c, bool on) { if (c) c->sw.sortByWidth = on; }
void bbmsa_sort_with_band(bbmsa_ctx *c, bool on) { if (c) c->sw.sortWithBand = on; }
void bbmsa_set_wide_unlimited(bbmsa_ctx *c, bool on) { if (c) c->sw.wideUnlimited = on; }
int bbmsa_set_latency_jobs(bbmsa_ctx *c, int64_t n) {
    if (!c || c->sw.scheme != BBMSA_SCHEME_11TS || c->legacyOnly) return BBMAP_OK;
    BBHIP(hipSetDevice(c->device));
    if (n > 0) BBTRY(setup_wide_pass(c));
    if (n > 0 && !c->slowList2.p) BBHIP(c->slowList2.grow(c->slowList.cap));   // (its hand-over list, late: as long as the first)
    c->sw.latencyJobs = c->sw.widePresent ? n : 0;
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

// the last launch's counters on the host, once its sequence has finished: what every read-back entry below starts with
static int read_counters(bbmsa_ctx *c, unsigned (&h)[bbmsa::kCounterWords]) {
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(c->ev[2]));
    BBHIP(hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
    return BBMAP_OK;
}

extern "C" int bbmsa_last_counts(bbmsa_ctx *c, int64_t *counts4) {
    if (!c || !c->timed || !counts4) return bbfail(BBMAP_E_ARG, "bbmsa_last_counts: nothing launched yet");
    unsigned h[bbmsa::kCounterWords];
    BBTRY(read_counters(c, h));
    const Route &r = c->last;
    // the wavefront list: what the band kernel left to the wavefront kernel without trying it, plus what it handed on -- on a sorted
    // launch the sort's general and unlimited lists, which hold no candidate (finished + handed on + this = the launch's jobs)
    counts4[0] = h[CNT_BAND_DONE]; counts4[1] = h[CNT_BAND_HANDED];
    counts4[2] = r.band ? (r.sorted ? h[CNT_SORTED_COUNT] + h[CNT_UNL_LIST_COUNT] : h[CNT_LIST_COUNT]) : 0;
    counts4[3] = r.wide ? h[CNT_WIDE_SLOW_COUNT] : h[CNT_SLOW_COUNT];
    if (getenv("BBMAP_DP_COUNTS")) {
        if (r.wide) fprintf(stderr, "   (first pass handed %u jobs to the wide pass)\n", h[CNT_SLOW_COUNT]);
        if (r.sorted) fprintf(stderr, "   (sorted: %u general, %u unlimited, %u band candidates)\n", h[CNT_SORTED_COUNT], h[CNT_UNL_LIST_COUNT], h[CNT_CAND_COUNT]);
        fprintf(stderr, "   (the wavefronts ran %u steps)\n", h[CNT_WAVE_STEPS]);
    }
    return BBMAP_OK;
}

// Test hook: the three lists the last launch's width sort made, as `n_jobs` ints each in lists3 (general, unlimited, band candidates;
// entries past a list's length are not written) and their lengths in lens3.  Fails when the last launch was not sorted.
extern "C" int bbmsa_debug_sorted_lists(bbmsa_ctx *c, int64_t n_jobs, int32_t *lists3, int64_t *lens3) {
    if (!c || !c->timed || !lists3 || !lens3) return bbfail(BBMAP_E_ARG, "bbmsa_debug_sorted_lists: nothing launched yet");
    if (!c->last.sorted || n_jobs != c->last.jobs) return bbfail(BBMAP_E_ARG, "bbmsa_debug_sorted_lists: the last launch was not a sorted launch of n_jobs jobs");
    unsigned h[bbmsa::kCounterWords];
    BBTRY(read_counters(c, h));
    const unsigned len[3] = {h[CNT_SORTED_COUNT], h[CNT_UNL_LIST_COUNT], h[CNT_CAND_COUNT]};
    for (int k = 0; k < 3; k++) {
        if ((int64_t)len[k] > n_jobs) return bbfail(BBMAP_E_HIP, "bbmsa_debug_sorted_lists: a list is longer than the launch");
        lens3[k] = len[k];
        if (len[k]) BBHIP(hipMemcpy(lists3 + (size_t)k * (size_t)n_jobs, c->fastList.as<int>() + (size_t)k * (size_t)n_jobs, (size_t)len[k] * 4, hipMemcpyDeviceToHost));
    }
    return BBMAP_OK;
}

extern "C" int bbmsa_last_unlimited(bbmsa_ctx *c, int64_t *counts4) {
    if (!c || !c->timed || !counts4) return bbfail(BBMAP_E_ARG, "bbmsa_last_unlimited: nothing launched yet");
    const bool wave = c->sw.scheme == BBMSA_SCHEME_11TS && !c->legacyOnly;
    if (wave && !c->unlimitedStats) return bbfail(BBMAP_E_ARG, "bbmsa_last_unlimited: the context does not count (create it with BBMSA_UNLIMITED_STATS=1 in the environment)");
    unsigned h[bbmsa::kCounterWords];
    BBTRY(read_counters(c, h));
    counts4[0] = wave ? h[CNT_UNL_RAN_UNL] : 0; counts4[1] = wave ? h[CNT_UNL_RAN_GENERAL] : 0;
    counts4[2] = wave ? h[CNT_UNL_STEPS] : 0; counts4[3] = wave ? h[CNT_ALL_STEPS] : 0;
    return BBMAP_OK;
}

int bbmsa_last_route_flags(const bbmsa_ctx *c) {
    if (!c || !c->timed) return 0;
    return (c->last.band ? BBMSA_ROUTE_NARROW : 0) | (c->last.sorted ? BBMSA_ROUTE_SORTED : 0) | (c->last.latency ? BBMSA_ROUTE_LATENCY : 0);
}

extern "C" int bbmsa_last_route(bbmsa_ctx *c, int64_t *route8) {
    if (!c || !c->timed || !route8) return bbfail(BBMAP_E_ARG, "bbmsa_last_route: nothing launched yet");
    unsigned h[bbmsa::kCounterWords];
    BBTRY(read_counters(c, h));
    const Route &r = c->last;
    route8[0] = r.band; route8[1] = r.sorted; route8[2] = r.latency; route8[3] = r.wide; route8[4] = r.indirect;
    route8[5] = h[CNT_SLOW_COUNT]; route8[6] = r.wide ? h[CNT_WIDE_SLOW_COUNT] : 0; route8[7] = r.band ? h[CNT_BAND_DONE] : 0;
    return BBMAP_OK;
}

extern "C" int bbmsa_geometry(bbmsa_ctx *c, int32_t *geo4) {
    if (!c || !geo4) return bbfail(BBMAP_E_ARG, "bbmsa_geometry: null argument");
    geo4[0] = geo4[1] = geo4[2] = geo4[3] = 0;
    if (c->legacy) {
        int last = 0, mask = 0;
        bbmsa_legacy_rows_per_lane(c, &last, &mask);
        geo4[0] = 64; geo4[1] = last; geo4[2] = c->cfg.maxColumns; geo4[3] = mask;
    } else if (c->sw.scheme == BBMSA_SCHEME_11TS) {
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
