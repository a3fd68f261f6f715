// The mapper's host side: context creation, and the batch driver that puts the stage kernels of mapper.hip / mapper_final.h, the
// probe and the DP launches on the stream in the reference's order (see mapper.hip's header), round by round.  What reads a
// finished batch is in mapper_output.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "mapper_ctx.h"

using namespace bbmapper;

extern "C" int bbmap_default_config_profile(int32_t profile, bbmap_config *c) {
    if (!c || (profile != BBIDX_PROFILE_BBMAP && profile != BBIDX_PROFILE_PACBIO)) return bbfail(BBMAP_E_ARG, "bbmap_default_config: bad argument");
    memset(c, 0, sizeof *c);
    c->paired = 0; c->max_reads = 0; c->max_sites = 32;
    c->extraPadding = 10; c->maxPairDist = 32000; c->averagePairDist = 100; c->maxRescueDist = 1200; c->maxRescueMismatches = 32;
    c->maxTrimSitesToRetain = 800; c->trimList = 1; c->doRescue = 1; c->clearzone3 = 800; c->fastCols = 0; c->jobsPerRead = 0;
    c->finalStage = profile == BBIDX_PROFILE_BBMAP ? 1 : 0;
    if (profile == BBIDX_PROFILE_PACBIO) {      // BBMapPacBio.setDefaults (BBMapPacBio.java:47-69), BBMapThreadPacBio.java:27-28
        c->max_read_len = 6016; c->minRatio = 0.46f; c->slowAlignPadding = 8; c->slowRescuePadding = 16; c->tipSearchDist = 15;
        c->alignColumns = 7600; c->msaMaxColumns = 7600;
    } else {                                    // BBMap.setDefaults (BBMap.java:45-65), BBMapThread.java:27-28
        c->max_read_len = 150; c->minRatio = 0.56f; c->slowAlignPadding = 4; c->slowRescuePadding = 8; c->tipSearchDist = 100;
        c->alignColumns = 3000; c->msaMaxColumns = 3000;
    }
    c->reserved[3] = profile;
    return BBMAP_OK;
}
extern "C" int bbmap_default_config(bbmap_config *c) { return bbmap_default_config_profile(BBIDX_PROFILE_BBMAP, c); }

extern "C" void bbmap_destroy(bbmap_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->h_counters) (void)hipHostFree(c->h_counters);
    if (c->tierThread.joinable()) c->tierThread.join();
    if (c->tier) bbmap_destroy(c->tier);
    bbidx_launch_free(&c->probeLs);
    for (DevBuf &b : c->buf) b.release();
    c->untrimTmp.release();
    delete c->cov;
    delete c->split;
    if (c->hostStream) (void)hipStreamDestroy(c->hostStream);
    if (c->tierStream) (void)hipStreamDestroy(c->tierStream);
    if (c->dpStream) (void)hipStreamDestroy(c->dpStream);
    if (c->evFork) (void)hipEventDestroy(c->evFork);
    if (c->evJoin) (void)hipEventDestroy(c->evJoin);
    if (c->ownsMsa && c->msaGapped && c->msaGapped != c->msa) bbmsa_destroy(c->msaGapped);
    if (c->ownsMsa && c->msa) bbmsa_destroy(c->msa);
    for (hipEvent_t e : c->ev) if (e) (void)hipEventDestroy(e);
    delete c;
}

// parent != null: the overflow tier of `parent` (longer job logs per read)
static int create_impl(bbidx_ctx *index, const bbmap_config *cfg, bbmap_ctx *parent, bbmap_ctx **out) {
    if (!index || !cfg || !out) return bbfail(BBMAP_E_ARG, "bbmap_create: null argument");
    *out = nullptr;
    const int profile = cfg->reserved[3];
    if (profile != BBIDX_PROFILE_BBMAP && profile != BBIDX_PROFILE_PACBIO) return bbfail(BBMAP_E_ARG, "bbmap_create: unknown profile (bbmap_config.reserved[3])");
    if (profile != index->dev.p.profile) return bbfail(BBMAP_E_ARG, "bbmap_create: the index was built for the other profile (BBIDX_PROFILE_*)");
    const bool pacbio = profile == BBIDX_PROFILE_PACBIO;
    if (cfg->max_reads < 1 || cfg->max_read_len < 1 || cfg->max_read_len > (pacbio ? BBIDX_PACBIO_MAX_READ_LEN : 600))
        return bbfail(BBMAP_E_ARG, "bbmap_create: max_reads >= 1 and max_read_len in 1..600 (1..6016 for BBIDX_PROFILE_PACBIO)");
    if (cfg->max_sites < 1 || cfg->max_sites > BBMAP_MAX_SITES_LIMIT) return bbfail(BBMAP_E_ARG, "bbmap_create: max_sites must be 1..4096");
    if (cfg->paired && (cfg->max_reads & 1)) return bbfail(BBMAP_E_ARG, "bbmap_create: paired mode takes an even number of reads");
    if (cfg->msaMaxColumns < 64 || cfg->msaMaxColumns > (pacbio ? 8192 : 4096)) return bbfail(BBMAP_E_ARG, "bbmap_create: msaMaxColumns must be 64..4096 (..8192 for BBIDX_PROFILE_PACBIO)");
    if (cfg->device != index->device) return bbfail(BBMAP_E_ARG, "bbmap_create: the index lives on another device");
    BBHIP(hipSetDevice(cfg->device));
    bbmap_ctx *c = new (std::nothrow) bbmap_ctx();
    if (!c) return bbfail(BBMAP_E_NOMEM, "bbmap_create: out of host memory");
    c->cfg = *cfg; c->index = index;
    int rc = BBMAP_OK;
    auto bail = [&](int code) { bbmap_destroy(c); return code; };
    if ((rc = bbidx_launch_init(index, &c->probeLs)) != BBMAP_OK) return bail(rc);
    // settings
    Settings &S = c->S;
    const float R = cfg->minRatio;
    S.minRatio = R;
    { const float a = R * .80f, b = 1.0f - ((1.0f - R) * 1.4f); S.ratioPaired = a > b ? a : b; }                // AbstractMapThread.java:106
    { const float a = R * .60f, b = 1.0f - ((1.0f - R) * 1.8f); S.ratioPreRescue = a > b ? a : b; }             // :107
    S.slowAlignPadding = cfg->slowAlignPadding; S.slowRescuePadding = cfg->slowRescuePadding; S.extraPadding = cfg->extraPadding;
    S.tipSearchDist = cfg->tipSearchDist; S.maxPairDist = cfg->maxPairDist; S.averagePairDist = cfg->averagePairDist;
    S.maxRescueDist = cfg->maxRescueDist; S.maxRescueMismatches = cfg->maxRescueMismatches; S.maxTrimSitesToRetain = cfg->maxTrimSitesToRetain;
    S.trimList = cfg->trimList; S.doRescue = cfg->doRescue; S.alignColumns = cfg->alignColumns; S.clearzone3 = cfg->clearzone3;
    S.maxIndel = index->dev.p.maxIndel; S.paired = cfg->paired; S.rescueSkip = 0;
    if (pacbio) { S.ptsMatch = 90; S.ptsMatch2 = 100; S.ptsSub = -137; S.ptsSub2 = -49; S.ptsSub3 = -25; S.impDelta = -305; }   // min(-292, -205 - 100)
    else { S.ptsMatch = 70; S.ptsMatch2 = 100; S.ptsSub = -127; S.ptsSub2 = -51; S.ptsSub3 = -25; S.impDelta = -495; }          // min(-472, -395 - 100)
    S.clearzone1e = 2 * S.ptsMatch2 - S.ptsMatch - S.ptsSub + 1;
    S.msaMaxColumns = cfg->msaMaxColumns;
    // MultiStateAligner9PacBio.java:2375-2407 / MultiStateAligner11tsJNI.c:18-98
    if (pacbio) { S.ptsSubR = -157; S.ptsIns = -205; S.ptsIns2 = -42; S.ptsIns3 = -23; S.ptsIns4 = -8; S.ptsDel = -292; S.ptsDel2 = -37; S.ptsDel3 = -17; S.ptsDel4 = -2; }
    else { S.ptsSubR = -147; S.ptsIns = -395; S.ptsIns2 = -39; S.ptsIns3 = -23; S.ptsIns4 = -8; S.ptsDel = -472; S.ptsDel2 = -33; S.ptsDel3 = -9; S.ptsDel4 = -1; }
    S.ptsDel5 = -1; S.ptsGap = -2;
    // finalStage: 0 off, 1 the profile's own mapping thread (BBMapThread / BBMapThreadPacBio), 2 BBMapThread's whatever the profile
    // (the parity seam: the oracle restates that tail only, oracle/mapper_oracle.c:758)
    if (pacbio && (cfg->finalStage < 0 || cfg->finalStage > 2)) return bail(bbfail(BBMAP_E_ARG, "bbmap_create: finalStage must be 0, 1 or 2"));
    S.finalStage = cfg->finalStage ? 1 : 0;
    S.finalPolicy = (pacbio && cfg->finalStage == 1) ? 1 : 0;
    {   // BBMapThreadPacBio.java:38-41, :112-115; BBMapThread.java:38-44
        const float rP = S.finalPolicy ? 1.5f : 1.6f, r1 = S.finalPolicy ? 2.2f : 2.0f, r1b = S.finalPolicy ? 2.8f : 2.6f, r1c = S.finalPolicy ? 4.8f : 4.6f;
        const float m2 = (float)S.ptsMatch2;
        S.czP = (int)(rP * m2); S.cz1 = (int)(r1 * m2); S.cz1b = (int)(r1b * m2); S.cz1c = (int)(r1c * m2);
        S.czLimit1e = 40;
    }
    // BBMap.java:434: `if(paired){BBIndex.QUIT_AFTER_TWO_PERFECTS=false;}` -- a static of the index class in the reference, so the
    // borrowed index context is switched the same way (and back for a single-ended mapper)
    index->dev.p.quitAfterTwoPerfects = cfg->paired ? 0 : 1;
    S.expLimit = (cfg->alignColumns * 17) / 20 - (2 * (cfg->slowAlignPadding + 10));                            // EXPECTED_LEN_LIMIT, :92
    // DP contexts: the plain one takes every ungapped window (first pass for the common narrow ones, the wide pass for the rest)
    const int maxRows = ((cfg->max_read_len + 31) / 32) * 32;
    c->maxRows = maxRows;
    bbmsa_config mc; memset(&mc, 0, sizeof mc);
    // two DP contexts.  The first takes the ordinary windows (read length + a few dozen columns): its LDS tables and column
    // buffers are sized for `fastCols` columns, which is what lets four blocks share a CU.  The second has the reference's own
    // 3000 columns (BBMapThread.java:27-28) and takes what does not fit the first: gapped references and wide windows.
    mc.device = cfg->device; mc.maxRows = maxRows;
    bbmsa_config gc;
    if (pacbio) {
        // mapPacBio: ONE context with the MultiStateAligner9PacBio scheme (strip-tiled wavefront kernel, msa_fill_strip.hip) and the
        // reference's 7600 columns for every fill, with or without a gap array; its traceback records and scratch matrices take tens
        // of GB, so the overflow tier borrows its parent's context and runs after the main pass instead of beside it
        mc.maxRows = cfg->max_read_len + 4 > 6100 ? 6100 : cfg->max_read_len + 4;
        c->maxRows = mc.maxRows;
        mc.maxColumns = cfg->msaMaxColumns;
        mc.reserved[2] = BBMSA_SCHEME_9PACBIO;
        gc = mc;
        c->plainColumns = mc.maxColumns;
        if (parent) { c->msa = parent->msa; c->msaGapped = parent->msaGapped; c->ownsMsa = false; }
        else {
            c->ownsMsa = true;
            if ((rc = bbmsa_create(&mc, &c->msa)) != BBMAP_OK) return bail(rc);
            c->msaGapped = c->msa;
        }
    } else {
        mc.maxColumns = cfg->fastCols > 0 ? cfg->fastCols : 256;
        if (mc.maxColumns > cfg->msaMaxColumns) mc.maxColumns = cfg->msaMaxColumns;
        c->plainColumns = mc.maxColumns;
        gc = mc;
        gc.maxColumns = cfg->msaMaxColumns;
        gc.reserved[0] = 32; gc.reserved[1] = 640 < gc.maxColumns ? 640 : gc.maxColumns;      // (32 lanes x 5 rows per job: 80 vs 85 ms of scoreSlow with sh/randomreads.sh's deletions; bbmsa_create widens the group for longer reads)
        if (const char *e = getenv("BBMAP_G2_LANES")) { if (*e) gc.reserved[0] = atoi(e); }          // experiments: geometry of the second context
        if (const char *e = getenv("BBMAP_G2_COLS")) { if (*e) gc.reserved[1] = atoi(e) < gc.maxColumns ? atoi(e) : gc.maxColumns; }
        (void)parent;                   // the tier runs beside its parent's pass: DP contexts of its own
        c->ownsMsa = true;
        if ((rc = bbmsa_create(&mc, &c->msa)) != BBMAP_OK) return bail(rc);
        if ((rc = bbmsa_create(&gc, &c->msaGapped)) != BBMAP_OK) return bail(rc);
    }
    const long long n = cfg->max_reads;
    const int cap = cfg->max_sites;
    c->narrowMinJobs = getenv("BBMAP_NARROW_MIN_JOBS") ? atoll(getenv("BBMAP_NARROW_MIN_JOBS")) : 32768;
    c->sortWide = !(getenv("BBMAP_SORT_WIDE") && atoi(getenv("BBMAP_SORT_WIDE")) == 0);      // (experiments: 0 switches the width order off)
    c->sortPlain = !(getenv("BBMAP_SORT_PLAIN") && atoi(getenv("BBMAP_SORT_PLAIN")) == 0);
    // the per-read kernels (0 switches a part off for A/B runs): first rounds in class order, Dev read in
    // place, chunked loads in the byte loops
    c->classOrder = !(getenv("BBMAP_CLASS_ORDER") && atoi(getenv("BBMAP_CLASS_ORDER")) == 0);
    c->classSwap = getenv("BBMAP_CLASS_ORDER") && atoi(getenv("BBMAP_CLASS_ORDER")) == 2;       // (tests: every read on the other list)
    c->kernargDev = !(getenv("BBMAP_KERNARG_DEV") && atoi(getenv("BBMAP_KERNARG_DEV")) == 0);
    S.chunkLoads = !(getenv("BBMAP_CHUNK_LOADS") && atoi(getenv("BBMAP_CHUNK_LOADS")) == 0);
    if (!pacbio) {
        // the 64-lane launches (latency route, wide pass) give unlimited fills the prune-free step loop; BBMAP_WIDE_UNLIMITED=0: no
        const bool wideUnl = !(getenv("BBMAP_WIDE_UNLIMITED") && atoi(getenv("BBMAP_WIDE_UNLIMITED")) == 0);
        bbmsa_set_wide_unlimited(c->msa, wideUnl);
        if (c->msaGapped != c->msa) bbmsa_set_wide_unlimited(c->msaGapped, wideUnl);
    }
    if (!pacbio) {
        // launches of a few hundred fills (the late rounds of scoreSlow and of the final stage) are one wavefront's latency: they take
        // the 64-lane geometry, whose step is the shorter chain (msa_ctx.h; 236 -> 231 ms per step for the second context alone)
        const long long lat = getenv("BBMAP_LATENCY_JOBS") ? atoll(getenv("BBMAP_LATENCY_JOBS")) : 4096;
        if ((rc = bbmsa_set_latency_jobs(c->msa, lat)) != BBMAP_OK) return bail(rc);
        if (c->msaGapped != c->msa && (rc = bbmsa_set_latency_jobs(c->msaGapped, lat)) != BBMAP_OK) return bail(rc);
    }
    // starting capacities of the two fill logs; they grow when a batch needs more (grow_logs)
    const int jpr = cfg->jobsPerRead > 0 ? cfg->jobsPerRead : 3;
    c->jobCap = n * jpr + 1024;
    c->gjobCap = parent ? n * 16 + 4096 : (n * jpr) / 24 + 4096;
    if (cfg->jobsPerRead < 0) c->jobCap = c->gjobCap = -(long long)cfg->jobsPerRead;       // exact starting capacity (tests of the growth path)
    c->rescCap = parent ? n * 64 + 1024 : n * 2 + 1024;
    c->matchStride = ((maxRows + c->plainColumns + 15) / 16) * 16;
    // a gapped match string expands every gap symbol to 128 'D's (traceback, MultiStateAligner11tsJNI.java:481-493)
    c->gmatchStride = ((maxRows + gc.maxColumns + 2 + 128 * 8 + 15) / 16) * 16;
    // the plain log rarely needs more than rows + columns of a NARROW window: cap its slot at what first-pass windows need, and
    // let the rare wide window report match_len = -1?  No: slots are sized for the widest window the context accepts.
#define DA(ptr, count) if ((rc = dalloc(c, &(ptr), (size_t)(count))) != BBMAP_OK) return bail(rc)
    DA(c->d_psites, n * cap); DA(c->d_pnsites, n);
    DA(c->d_ms, n * cap); DA(c->d_mcount, n); DA(c->d_near, n);
    DA(c->d_slow, n);
    DA(c->d_active[0], n); DA(c->d_active[1], n);
    c->d_classList = nullptr;
    if (c->classOrder) DA(c->d_classList, 2 * n);
    DA(c->d_counters, CNT_WORDS);
    DA(c->d_jobs, c->jobCap); DA(c->d_jinfo, c->jobCap); DA(c->d_results, c->jobCap); DA(c->d_match, c->jobCap * c->matchStride);
    DA(c->d_gjobs, c->gjobCap); DA(c->d_ggaps, c->gjobCap); DA(c->d_ginfo, c->gjobCap); DA(c->d_gresults, c->gjobCap); DA(c->d_gmatch, c->gjobCap * c->gmatchStride);
    DA(c->d_rjobs, c->rescCap); DA(c->d_rinfo, c->rescCap); DA(c->d_rres, c->rescCap); DA(c->d_rsite, c->rescCap);
    DA(c->d_pres, n / 2 + 1);
    if (S.finalStage) {
        // match strings of the final stage: one of the read's length per perfect read, about two per imperfect one; grows on demand
        c->poolUnits = (n * (long long)(3 * (cfg->max_read_len + 16)) + 65536) / 4;
        if (const char *e = getenv("BBMAP_FINAL_POOL_UNITS")) { if (*e && atoll(e) >= 64) c->poolUnits = atoll(e); }      // (tests of the growth path)
        DA(c->d_fin, n); DA(c->d_final, n); DA(c->d_pool, c->poolUnits * 4);
    }
    const int nch = index->dev.nchroms;
    DA(c->d_chromMin, nch + 1); DA(c->d_chromOff, nch + 1);
#undef DA
    c->d_chromArr = index->dev.chromArr; c->d_chromArrLen = index->dev.chromArrLen;
    {
        std::vector<const uint8_t *> hc((size_t)nch + 1);
        if (hipMemcpy(hc.data(), index->dev.chromArr, sizeof(void *) * hc.size(), hipMemcpyDeviceToHost) != hipSuccess) return bail(bbfail(BBMAP_E_HIP, "bbmap_create: reading the chromosome table failed"));
        c->refsBase = hc[1];
        std::vector<long long> off((size_t)nch + 1, 0);
        for (int i = 1; i <= nch; i++) off[(size_t)i] = (long long)(hc[(size_t)i] - hc[1]);
        if (hipMemcpy(c->d_chromOff, off.data(), 8 * off.size(), hipMemcpyHostToDevice) != hipSuccess) return bail(bbfail(BBMAP_E_HIP, "bbmap_create: upload failed"));
        if (hipMemset(c->d_chromMin, 0, 4 * ((size_t)nch + 1)) != hipSuccess) return bail(bbfail(BBMAP_E_HIP, "bbmap_create: memset failed"));
    }
    if (hipHostMalloc((void **)&c->h_counters, CNT_WORDS * 4) != hipSuccess) return bail(bbfail(BBMAP_E_NOMEM, "bbmap_create: pinned allocation failed"));
    for (hipEvent_t &e : c->ev) if (hipEventCreate(&e) != hipSuccess) return bail(bbfail(BBMAP_E_HIP, "bbmap_create: hipEventCreate failed"));
    if (!getenv("BBMAP_SERIAL_DP") && !pacbio) {
        if (hipStreamCreateWithFlags(&c->dpStream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming) != hipSuccess) return bail(bbfail(BBMAP_E_HIP, "bbmap_create: stream / event creation failed"));
    }
    *out = c;
    return BBMAP_OK;
}

extern "C" int bbmap_create(bbidx_ctx *index, const bbmap_config *cfg, bbmap_ctx **out) {
    bbmap_ctx *c = nullptr;
    BBTRY(create_impl(index, cfg, nullptr, &c));
    // reserved[1]: reads the overflow tier holds (0 = 4096, < 0 = no tier); reserved[2]: its max_sites (0 = 1024)
    if (cfg->reserved[1] >= 0) {
        bbmap_config tc = *cfg;
        long long tn = cfg->reserved[1] > 0 ? cfg->reserved[1] : 4096;
        if (tn > cfg->max_reads) tn = cfg->max_reads;
        if (cfg->paired) tn &= ~1ll;
        tc.max_reads = (int32_t)tn;
        tc.max_sites = cfg->reserved[2] > 0 ? cfg->reserved[2] : 1024;
        tc.jobsPerRead = 128;
        tc.reserved[1] = -1;
        if (tn >= (cfg->paired ? 2 : 1) && tc.max_sites > cfg->max_sites) {
            const int rc = create_impl(index, &tc, c, &c->tier);
            if (rc != BBMAP_OK) { bbmap_destroy(c); return rc; }
            const long long units = cfg->paired ? cfg->max_reads / 2 : cfg->max_reads;
            if (dalloc(c, &c->d_tierUnits, (size_t)units + 1) != BBMAP_OK || dalloc(c, &c->d_tierReads, (size_t)tn) != BBMAP_OK ||
                dalloc(c, &c->d_tierReadIds, (size_t)tn) != BBMAP_OK) { bbmap_destroy(c); return BBMAP_E_NOMEM; }
            if (hipStreamCreateWithFlags(&c->tierStream, hipStreamNonBlocking) != hipSuccess) { bbmap_destroy(c); return bbfail(BBMAP_E_HIP, "bbmap_create: hipStreamCreate failed"); }
        }
    }
    *out = c;
    return BBMAP_OK;
}

static int read_counters(bbmap_ctx *c, hipStream_t stream) {
    BBHIP(hipMemcpyAsync(c->h_counters, c->d_counters, CNT_WORDS * 4, hipMemcpyDeviceToHost, stream));
    BBHIP(hipStreamSynchronize(stream));
    return BBMAP_OK;
}

// Replaces a device array by a larger one (contents kept), in stream order; the old one is freed once the stream has passed.
template <class T> static int regrow(bbmap_ctx *c, hipStream_t stream, T **p, size_t oldCount, size_t newCount, std::vector<void *> &dead) {
    void *d = nullptr;
    if (hipMalloc(&d, (newCount ? newCount : 1) * sizeof(T)) != hipSuccess) return bbfail(BBMAP_E_NOMEM, "bbmap_map_batch_device: growing a fill log failed (device memory)");
    if (oldCount) BBHIP(hipMemcpyAsync(d, *p, oldCount * sizeof(T), hipMemcpyDeviceToDevice, stream));
    for (void *&q : c->allocs) if (q == (void *)*p) q = d;
    dead.push_back((void *)*p);
    *p = (T *)d;
    return BBMAP_OK;
}
// The reference's per-read lists of fills have no capacity.  When a round asks for more log entries than there are (the kernels
// then hold the affected reads back, emit_fill's NO_ROOM), the logs are grown here before the next round; `needJobs` / `needGapped`
// = entries that must fit.  The device counters are set back to the number of entries that were really written.
// arrays a regrow has replaced: freed when the guard goes out of scope, after the stream has passed the copies (error paths included)
struct DeadArrays {
    hipStream_t stream; std::vector<void *> v;
    explicit DeadArrays(hipStream_t s) : stream(s) {}
    ~DeadArrays() { if (!v.empty()) { (void)hipStreamSynchronize(stream); for (void *q : v) (void)hipFree(q); } }
};
static int grow_logs(bbmap_ctx *c, hipStream_t stream, Dev &D, long long needJobs, long long needGapped, long long usedJobs, long long usedGapped) {
    DeadArrays guard(stream);
    std::vector<void *> &dead = guard.v;
    if (needJobs > c->jobCap) {
        long long nc = c->jobCap * 2; if (nc < needJobs) nc = needJobs + needJobs / 4 + 1024;
        BBTRY(regrow(c, stream, &c->d_jobs, (size_t)usedJobs, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_jinfo, (size_t)usedJobs, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_results, (size_t)usedJobs, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_match, (size_t)usedJobs * c->matchStride, (size_t)nc * c->matchStride, dead));
        c->jobCap = nc;
    }
    if (needGapped > c->gjobCap) {
        long long nc = c->gjobCap * 2; if (nc < needGapped) nc = needGapped + needGapped / 4 + 1024;
        BBTRY(regrow(c, stream, &c->d_gjobs, (size_t)usedGapped, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_ggaps, (size_t)usedGapped, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_ginfo, (size_t)usedGapped, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_gresults, (size_t)usedGapped, (size_t)nc, dead));
        BBTRY(regrow(c, stream, &c->d_gmatch, (size_t)usedGapped * c->gmatchStride, (size_t)nc * c->gmatchStride, dead));
        c->gjobCap = nc;
    }
    c->h_counters[CNT_STAGE_FILLS] = (unsigned)usedJobs; c->h_counters[CNT_STAGE_GAPPED] = (unsigned)usedGapped;
    BBHIP(hipMemcpyAsync(c->d_counters + CNT_FILLS, c->h_counters + CNT_STAGE_FILLS, 8, hipMemcpyHostToDevice, stream));      // both words
    BBHIP(hipStreamSynchronize(stream));
    D.jobs = c->d_jobs; D.jinfo = c->d_jinfo; D.results = c->d_results; D.match = c->d_match; D.jobCap = c->jobCap;
    D.gjobs = c->d_gjobs; D.ggaps = c->d_ggaps; D.ginfo = c->d_ginfo; D.gresults = c->d_gresults; D.gmatch = c->d_gmatch; D.gjobCap = c->gjobCap;
    c->stats.log_growths += 1.0f;              // (how often the logs grew in this batch)
    return BBMAP_OK;
}

// launches the DP over the fills appended since (jobBase, gjobBase)
static int run_fills(bbmap_ctx *c, hipStream_t stream, const uint8_t *bases, long long jobBase, long long nNew, long long gBase, long long gNew,
                     bool finalStage = false) {
    // The band kernel (msa_fill_band.hip) runs in front of the wavefront kernel on the same stream and is a dependent chain of
    // 2 * rows turns however few jobs there are: worth it only for the big first rounds -- of scoreSlow, of rescue and of the final
    // stage (a third to a half of their fills finish in its 32 diagonals).  The second context's wide windows never fit.
    bbmsa_use_narrow(c->msa, nNew >= c->narrowMinJobs);
    // The first context's launches that run the band kernel are sorted too (bbmsa_sort_with_band): two fills share a 32-lane
    // wavefront and step together as long as the wider one needs.  BBMAP_SORT_PLAIN=0 switches it off (A/B runs).
    // Measured: 193.9 ms per step with it, 198.5 without; scoreSlow 57.6 / 59.5, the final stage 55.1 / 57.3 ms.
    // (An older note here had the sorted plain pass lose 6 ms in the final stage; that was before the band kernel took the tight
    // fills and before the second context's unlimited fills had a build of their own, and no longer holds.)
    bbmsa_sort_by_width(c->msa, c->sortPlain && nNew >= c->narrowMinJobs);
    bbmsa_sort_with_band(c->msa, c->sortPlain);
    if (c->msaGapped != c->msa) { bbmsa_use_narrow(c->msaGapped, false); bbmsa_sort_by_width(c->msaGapped, c->sortWide); }
    // the second context's launches first, on their own stream: its blocks take their share of the CUs and the plain context's
    // persistent blocks fill the rest (and the slots the others free)
    hipStream_t gs = (c->dpStream && nNew > 0) ? c->dpStream : stream;
    if (gNew > 0) {
        if (gs != stream) { BBHIP(hipEventRecord(c->evFork, stream)); BBHIP(hipStreamWaitEvent(gs, c->evFork, 0)); }
        BBTRY(bbmsa_align_gapped_batch_device(c->msaGapped, gs, gNew, c->d_gjobs + gBase, c->d_ggaps + gBase, bases, c->refsBase,
                                             c->d_gresults + gBase, c->d_gmatch + gBase * c->gmatchStride, c->gmatchStride));
        if (gs != stream) { BBHIP(hipEventRecord(c->evJoin, gs)); if (nNew > 0) BBTRY(bbmsa_wait_first_pass(c->msaGapped, stream)); }
    }
    if (nNew > 0)
        BBTRY(bbmsa_align_batch_device(c->msa, stream, nNew, c->d_jobs + jobBase, bases, c->refsBase, c->d_results + jobBase,
                                      c->d_match + jobBase * c->matchStride, c->matchStride));
    // which routes the launches took (host flags of the DP contexts, no device read-back)
    const int r1 = nNew > 0 ? bbmsa_last_route_flags(c->msa) : 0;
    const int r2 = gNew > 0 ? bbmsa_last_route_flags(c->msaGapped) : 0;
    c->stats.dp_narrow_launches += (r1 & 1) + (r2 & 1);
    c->stats.dp_sorted_launches += ((r1 >> 1) & 1) + ((r2 >> 1) & 1);
    if (gNew > 0 && gs != stream) BBHIP(hipStreamWaitEvent(stream, c->evJoin, 0));
    return BBMAP_OK;
}

static void add_dp_ms(bbmap_ctx *c, bool plain, bool gapped) {
    float k3[3];
    if (plain && bbmsa_last_kernel_ms3(c->msa, k3) == BBMAP_OK) { c->stats.ms_dp_narrow += k3[0]; c->stats.ms_dp_wave += k3[1]; c->stats.ms_dp_generic += k3[2];
                                                                 if (k3[1] > c->stats.ms_dp_wave_max) c->stats.ms_dp_wave_max = k3[1]; }
    // (mapPacBio has ONE context for both logs: its kernel times are the plain launch's already, a second reading would count them twice)
    if (gapped && c->msaGapped != c->msa && bbmsa_last_kernel_ms3(c->msaGapped, k3) == BBMAP_OK) c->stats.ms_dp_gapped += k3[0] + k3[1] + k3[2];
    static const bool show = getenv("BBMAP_DP_COUNTS") != nullptr;      // where the fills of a launch sequence ended up (experiments)
    if (show) {
        int64_t n4[4], u4[4];
        if (plain && bbmsa_last_counts(c->msa, n4) == BBMAP_OK && bbmsa_last_unlimited(c->msa, u4) == BBMAP_OK)
            fprintf(stderr, "dp counts plain : narrow finished %lld, narrow handed on %lld, wavefront list %lld, to the wide/generic pass %lld, "
                    "unlimited in their own build %lld, in the general build %lld, wavefront steps unlimited %lld of %lld\n",
                    (long long)n4[0], (long long)n4[1], (long long)n4[2], (long long)n4[3], (long long)u4[0], (long long)u4[1], (long long)u4[2], (long long)u4[3]);
        if (gapped && bbmsa_last_counts(c->msaGapped, n4) == BBMAP_OK && bbmsa_last_unlimited(c->msaGapped, u4) == BBMAP_OK)
            fprintf(stderr, "dp counts second: narrow finished %lld, narrow handed on %lld, wavefront list %lld, to the wide/generic pass %lld, "
                    "unlimited in their own build %lld, in the general build %lld, wavefront steps unlimited %lld of %lld\n",
                    (long long)n4[0], (long long)n4[1], (long long)n4[2], (long long)n4[3], (long long)u4[0], (long long)u4[1], (long long)u4[2], (long long)u4[3]);
    }
}

static void tier_start_async(bbmap_ctx *c, long long found);

// scoreSlow and the final stage's genMatchString both run in rounds: a kernel advances every active read until it needs a fill, the
// fills of all reads run through the DP contexts, the next round consumes them.  A round is two halves with the loop's own steps
// between and behind them.
struct Rounds {
    bool finalStage;                // the final stage's rounds: the pool's words are reset with the active count, run_fills is told
    long long jobBase, gBase;       // entries of the two fill logs already used (and run)
    long long nActive;
    int cur = 0;
    bool first = true, ranPlain = false, ranGapped = false;
};
// first half: the round's kernel over the active list, and its counters
template <class K> static int round_begin(bbmap_ctx *c, hipStream_t stream, Dev &D, Rounds &R, K kernel) {
    BBHIP(hipMemsetAsync(c->d_counters + CNT_NEXT_ACTIVE, 0, 4, stream));
    if (R.finalStage) {
        BBHIP(hipMemsetAsync(c->d_counters + CNT_POOL_AT_FAILURE, 0xff, 4, stream));
        BBHIP(hipMemsetAsync(c->d_counters + CNT_POOL_FAILED, 0, 4, stream));
    }
    D.activeIn = R.first ? nullptr : c->d_active[R.cur]; D.nActiveIn = (int)R.nActive; D.activeOut = c->d_active[1 - R.cur];
    BBTRY(launch<128>(kernel, R.nActive, stream, D));
    return read_counters(c, stream);
}
// second half: the fills the round asked for, larger logs when it asked for more than there was room for, the next active list
static int round_end(bbmap_ctx *c, hipStream_t stream, Dev &D, Rounds &R, const uint8_t *bases) {
    add_dp_ms(c, R.ranPlain, R.ranGapped);          // (the round before this one: its launches are over)
    const long long asked = c->h_counters[CNT_FILLS], gasked = c->h_counters[CNT_GAPPED_FILLS];
    const long long total = asked < c->jobCap ? asked : c->jobCap, gtotal = gasked < c->gjobCap ? gasked : c->gjobCap;     // entries really written
    BBTRY(run_fills(c, stream, bases, R.jobBase, total - R.jobBase, R.gBase, gtotal - R.gBase, R.finalStage));
    R.ranPlain = total > R.jobBase; R.ranGapped = gtotal > R.gBase;
    R.jobBase = total; R.gBase = gtotal;
    // a log was too small: the reads that found no room ask again next round (emit_fill's NO_ROOM), after it has grown
    if (asked > c->jobCap || gasked > c->gjobCap) BBTRY(grow_logs(c, stream, D, asked, gasked, total, gtotal));
    R.nActive = c->h_counters[CNT_NEXT_ACTIVE];
    R.cur = 1 - R.cur; R.first = false;
    return BBMAP_OK;
}

// Replaces the final stage's match-string pool by one of `units` units, the first `used` of them kept.
static int grow_pool(bbmap_ctx *c, hipStream_t stream, Dev &D, long long used, long long units, bool setCounter) {
    if (units > 0x7ffffff0LL) return bbfail(BBMAP_E_NOMEM, "bbmap_map_batch_device: the final stage's match strings exceed 8 GB; map smaller batches");
    DeadArrays guard(stream);                          // (frees the old pool when this scope is left, also on an error return)
    BBTRY(regrow(c, stream, &c->d_pool, (size_t)used * 4, (size_t)units * 4, guard.v));
    if (setCounter) {                                  // the device counter back to the units really handed out
        c->h_counters[CNT_STAGE_POOL] = (unsigned)used;
        BBHIP(hipMemcpyAsync(c->d_counters + CNT_POOL_UNITS, c->h_counters + CNT_STAGE_POOL, 4, hipMemcpyHostToDevice, stream));
    }
    BBHIP(hipStreamSynchronize(stream));
    c->poolUnits = units; D.pool = c->d_pool; D.poolUnits = units;
    return BBMAP_OK;
}

// The final alignment stage (mapper_final.h) over the site lists in c->d_ms: policy, genMatchString in rounds, policy,
// toLocalAlignment.  jobBase / gBase: entries of the two fill logs already used (and run).
static int run_final_stage(bbmap_ctx *c, hipStream_t stream, Dev &D, int64_t n_reads, const uint8_t *bases, long long jobBase, long long gBase,
                           long long &finalRounds, long long &finalLocal) {
    const long long units = c->cfg.paired ? n_reads / 2 : n_reads;
    const unsigned *h = c->h_counters;
    D.fin = c->d_fin; D.finalOut = c->d_final; D.pool = c->d_pool; D.poolUnits = c->poolUnits;
    D.match = c->d_match; D.gmatch = c->d_gmatch; D.matchStride = c->matchStride; D.gmatchStride = c->gmatchStride;
    if (D.classList) BBHIP(hipMemsetAsync(c->d_counters + CNT_CLASS_LONG, 0, 8, stream));       // and CNT_CLASS_SHORT behind it
    BBTRY(launch<128>(final_begin_kernel, units, stream, D));
    Rounds R; R.finalStage = true; R.jobBase = jobBase; R.gBase = gBase; R.nActive = n_reads;
    for (int round = 0; R.nActive > 0; round++) {
        if (round > 64 * c->cfg.max_sites + 64) return bbfail(BBMAP_E_HIP, "bbmap_map_batch_device: the final stage does not come to an end (internal error)");
        BBTRY(round_begin(c, stream, D, R, DEV_KERNEL(c, final_round_kernel)));
        BBTRY(round_end(c, stream, D, R, bases));
        if (h[CNT_POOL_FAILED] > 0) {           // the match-string pool was full for some reads: they repeat their step next round
            const long long used = h[CNT_POOL_AT_FAILURE];                      // units handed out before the first request that failed
            long long nu = c->poolUnits * 2, need = used + ((long long)h[CNT_POOL_UNITS] - used) * 2 + 65536;
            if (nu < need) nu = need;
            BBTRY(grow_pool(c, stream, D, used, nu, true));
        }
        finalRounds++;
    }
    BBHIP(hipStreamSynchronize(stream));
    add_dp_ms(c, R.ranPlain, R.ranGapped);
    BBHIP(hipMemsetAsync(c->d_counters + CNT_LOCAL_READS, 0, 8, stream));       // and CNT_LOCAL_UNITS behind it
    BBTRY(launch<128>(final_end_kernel, units, stream, D));
    BBTRY(read_counters(c, stream));
    finalLocal = h[CNT_LOCAL_READS];
    const long long used = h[CNT_POOL_UNITS], local = h[CNT_LOCAL_UNITS];
    if (used + local + 64 > c->poolUnits) BBTRY(grow_pool(c, stream, D, used, used + local + 65536, false));      // room for toLocalAlignment's strings
    BBTRY(launch<128>(final_local_kernel, units, stream, D));
    return BBMAP_OK;
}


static void fill_dev(bbmap_ctx *c, Dev &D, int64_t n_reads, const bbidx_read *reads, uint8_t *bases, int64_t minus_delta) {
    memset(&D, 0, sizeof D);
    D.S = c->S; D.reads = reads; D.bases = bases; D.minusDelta = minus_delta; D.nreads = n_reads;
    D.chromArr = c->d_chromArr; D.chromArrLen = c->d_chromArrLen; D.refsBase = c->refsBase;
    D.psites = c->d_psites; D.pnsites = c->d_pnsites; D.maxSites = c->cfg.max_sites;
    D.ms = c->d_ms; D.mcount = c->d_mcount; D.cap = c->cfg.max_sites; D.nearArr = c->d_near; D.slow = c->d_slow;
    D.classList = c->d_classList; D.classSwap = c->classSwap ? 1 : 0;
    D.counters = c->d_counters; D.plainColumns = c->plainColumns; D.fillAhead = c->cfg.reserved[0] ? 0 : 1;
    D.jobs = c->d_jobs; D.jinfo = c->d_jinfo; D.results = c->d_results; D.jobCap = c->jobCap;
    D.gjobs = c->d_gjobs; D.ggaps = c->d_ggaps; D.ginfo = c->d_ginfo; D.gresults = c->d_gresults; D.gjobCap = c->gjobCap;
    D.rjobs = c->d_rjobs; D.rinfo = c->d_rinfo; D.rres = c->d_rres; D.pres = c->d_pres; D.rescCap = c->rescCap; D.rsite = c->d_rsite;
    if (c->index->scafFilter) D.scaf = c->index->scaf;
}

// The end of a batch: its counters and stage times become bbmap_stats.  whole: the whole flow ran (map_records); else the final stage
// alone (bbmap_final_batch_device), which has no other stage's counts or times.  fillsBefore: log entries used before the final stage.
static int finish_stats(bbmap_ctx *c, hipStream_t stream, bool whole, long long fillsBefore, long long finalRounds, long long finalLocal) {
    BBHIP(hipEventRecord(c->ev[EV_FINAL_END], stream));
    BBTRY(read_counters(c, stream));
    const unsigned *h = c->h_counters;
    const hipEvent_t *ev = c->ev;
    c->poolUsed = 4ll * h[CNT_POOL_UNITS];
    c->nJobs = h[CNT_FILLS]; c->nGapped = h[CNT_GAPPED_FILLS];
    c->finalFills = c->S.finalStage ? (c->nJobs + c->nGapped) - fillsBefore : 0;
    bbmap_stats &st = c->stats;
    st.fills = c->nJobs; st.gapped_fills = c->nGapped;
    (void)hipEventElapsedTime(&st.ms_final, ev[EV_RESCUE_END], ev[EV_FINAL_END]);
    if (whole) {
        st.reads_overflowed = h[CNT_OVERFLOWED]; st.reads_without_site = h[CNT_NO_SITE];
        st.refills = h[CNT_REFILLS]; st.rescue_fills = h[CNT_RESCUE_FILLS]; st.fills_dropped = h[CNT_FILLS_DROPPED];
        st.sites_cross_scaffold = h[CNT_CROSS_SCAFFOLD];
        (void)hipEventElapsedTime(&st.ms_probe, ev[EV_START], ev[EV_PROBE_END]);
        (void)hipEventElapsedTime(&st.ms_begin, ev[EV_PROBE_END], ev[EV_BEGIN_END]);
        (void)hipEventElapsedTime(&st.ms_score, ev[EV_BEGIN_END], ev[EV_SCORE_END]);
        (void)hipEventElapsedTime(&st.ms_slow, ev[EV_SCORE_END], ev[EV_SLOW_END]);
        (void)hipEventElapsedTime(&st.ms_finish, ev[EV_SLOW_END], ev[EV_FINISH_END]);
        (void)hipEventElapsedTime(&st.ms_rescue, ev[EV_FINISH_END], ev[EV_RESCUE_END]);
        (void)hipEventElapsedTime(&st.ms_total, ev[EV_START], ev[EV_FINAL_END]);
    } else st.ms_total = st.ms_final;
    st.final_fills = c->finalFills; st.final_rounds = finalRounds; st.final_local = finalLocal;
    return BBMAP_OK;
}

// one context's pass over `n_reads` read records
static int map_records(bbmap_ctx *c, hipStream_t stream, int64_t n_reads, const bbidx_read *reads, uint8_t *bases,
                       int64_t minus_delta, const int8_t *baseScores, const int32_t *keyinfo, bool writeRc) {
    memset(&c->stats, 0, sizeof c->stats);
    c->stats.reads = n_reads;
    BBHIP(hipMemsetAsync(c->d_counters, 0, CNT_WORDS * 4, stream));
    BBHIP(hipEventRecord(c->ev[EV_START], stream));
    // ---- probe (BBIndex.findAdvanced); reverse complements are written on the way
    BBTRY(bbidx_find_batch_device_with(c->index, &c->probeLs, stream, n_reads, reads, bases, baseScores, keyinfo, c->d_psites, c->cfg.max_sites,
                                      c->d_pnsites, writeRc ? bases + minus_delta : nullptr));
    if (writeRc) BBTRY(launch<128>(revcomp_unprobed_kernel, n_reads, stream, reads, (long long)n_reads, (int)c->index->dev.p.k, (const uint8_t *)bases, bases + minus_delta));
    BBHIP(hipEventRecord(c->ev[EV_PROBE_END], stream));
    Dev D;
    fill_dev(c, D, n_reads, reads, bases, minus_delta);
    const long long units = c->cfg.paired ? n_reads / 2 : n_reads;
    BBTRY(launch<128>(begin_kernel, units, stream, D));
    if (c->tier) {                       // the units the probe flagged: known now, so the tier can work beside the rest of this pass
        BBTRY(launch<128>(collect_overflow_kernel, units, stream, c->d_mcount, units, c->cfg.paired, c->d_tierUnits, c->d_counters + CNT_TIER_FOUND));
    }
    BBHIP(hipEventRecord(c->ev[EV_BEGIN_END], stream));
    BBTRY(launch<128>(DEV_KERNEL(c, score_kernel), n_reads, stream, D));
    BBHIP(hipEventRecord(c->ev[EV_SCORE_END], stream));
    // ---- scoreSlow in rounds
    Rounds R; R.finalStage = false; R.jobBase = R.gBase = 0; R.nActive = n_reads;
    for (int round = 0; R.nActive > 0 && round < 4 * c->cfg.max_sites + 4; round++) {
        BBTRY(round_begin(c, stream, D, R, slow_round_kernel));
        if (round == 0) {
            // the probe is over: its statistics are read now
            float pms = 0; long long ps[5];       // (not for the tier's own pass: the synchronous copy inside would wait for the main stream)
            if (writeRc && bbidx_last_stats_with(c->index, &c->probeLs, (int64_t *)ps, &pms) == BBMAP_OK) for (int i = 0; i < 5; i++) c->stats.probe_stats[i] = ps[i];
            c->overAfterBegin = c->h_counters[CNT_OVERFLOWED];
            if (c->tier && c->h_counters[CNT_TIER_FOUND] > 0 && c->tier->msa != c->msa) tier_start_async(c, c->h_counters[CNT_TIER_FOUND]);     // (a tier that borrows the DP context runs after the pass)
        }
        BBTRY(round_end(c, stream, D, R, bases));
        c->stats.rounds++;
    }
    long long jobBase = R.jobBase, gBase = R.gBase;
    BBHIP(hipEventRecord(c->ev[EV_SLOW_END], stream));
    BBTRY(launch<128>(finish_kernel, n_reads, stream, D));
    BBHIP(hipEventRecord(c->ev[EV_FINISH_END], stream));
    // ---- rescue: mate 1 anchors, then mate 2
    if (c->cfg.paired && c->cfg.doRescue) {
        const long long pairs = n_reads / 2;
        for (int pass = 0; pass < 2; pass++) {
            D.pass = pass;
            // each pass gets its own region of the search list: reset the search counter, keep the fills' counters
            BBHIP(hipMemsetAsync(c->d_counters + CNT_RESCUE_SEARCHES, 0, 4, stream));
            BBTRY(launch<128>(rescue_plan_kernel, pairs, stream, D));
            BBTRY(read_counters(c, stream));
            const long long nsearch = c->h_counters[CNT_RESCUE_SEARCHES];
            if (nsearch > c->rescCap) return bbfail(BBMAP_E_NOMEM, "bbmap_map_batch_device: rescue list full");
            c->stats.rescue_scans += nsearch;
            if (nsearch == 0) {
                BBTRY(launch<128>(rescue_finish_kernel, pairs, stream, D));
                continue;
            }
            hipEvent_t q0 = c->ev[EV_QUICK_BEGIN], q1 = c->ev[EV_QUICK_END];
            BBHIP(hipEventRecord(q0, stream));
            BBTRY(bbpipe_quick_rescue_device(stream, nsearch, c->d_rjobs, bases, (const int64_t *)c->d_chromOff, c->d_chromArrLen, c->d_chromMin, c->refsBase,
                                            c->d_rres, c->S.ptsMatch, c->S.ptsMatch2, 1, 100));
            BBHIP(hipEventRecord(q1, stream));
            // every search issues at most one fill, into either log: room for all of them before the kernel that writes them
            if (jobBase + nsearch > c->jobCap || gBase + nsearch > c->gjobCap) BBTRY(grow_logs(c, stream, D, jobBase + nsearch, gBase + nsearch, jobBase, gBase));
            BBTRY(launch<128>(DEV_KERNEL(c, rescue_prep_kernel), pairs, stream, D));
            BBTRY(read_counters(c, stream));
            { float ms = 0; if (hipEventElapsedTime(&ms, q0, q1) == hipSuccess) c->stats.ms_quick_rescue += ms; }
            const long long total = c->h_counters[CNT_FILLS], gtotal = c->h_counters[CNT_GAPPED_FILLS];
            if (total > c->jobCap || gtotal > c->gjobCap) return bbfail(BBMAP_E_HIP, "bbmap_map_batch_device: rescue fills beyond the reserved log entries (internal error)");
            BBTRY(run_fills(c, stream, bases, jobBase, total - jobBase, gBase, gtotal - gBase));
            const bool ranPlain = total > jobBase, ranGapped = gtotal > gBase;
            jobBase = total; gBase = gtotal;
            BBTRY(launch<128>(rescue_finish_kernel, pairs, stream, D));
            BBHIP(hipStreamSynchronize(stream));
            add_dp_ms(c, ranPlain, ranGapped);
        }
    }
    BBHIP(hipEventRecord(c->ev[EV_RESCUE_END], stream));
    // ---- the final alignment stage
    c->finalFills = 0; c->poolUsed = 0;
    long long finalRounds = 0, finalLocal = 0;
    if (c->S.finalStage) BBTRY(run_final_stage(c, stream, D, n_reads, bases, jobBase, gBase, finalRounds, finalLocal));
    BBTRY(finish_stats(c, stream, true, jobBase + gBase, finalRounds, finalLocal));
    c->ran = true;
    return BBMAP_OK;
}

// The reference's ArrayList<SiteScore> has no capacity (BBIndex.java:1537-1604).  Reads whose list did not fit max_sites are
// mapped again, from the probe on, by the tier context with its long lists (pairs as pairs); a read the tier cannot hold either
// stays flagged.  The reads the PROBE flagged are known once begin_kernel has run, and the tier maps them on its own stream
// beside the rest of the main pass.  A list can also outgrow max_sites when rescue appends to it (rare): then the tier runs once
// more after the main pass, over all flagged reads.
static int tier_pass(bbmap_ctx *c, hipStream_t s, long long found) {
    bbmap_ctx *t = c->tier;
    const bbmap_ctx::BatchArgs &B = c->batch;
    const int paired = c->cfg.paired;
    c->tierReads = 0; t->ran = false;
    std::vector<int> ids((size_t)found);
    BBHIP(hipMemcpyAsync(ids.data(), c->d_tierUnits, 4 * (size_t)found, hipMemcpyDeviceToHost, s));
    BBHIP(hipStreamSynchronize(s));
    std::sort(ids.begin(), ids.end());
    const long long room = paired ? t->cfg.max_reads / 2 : t->cfg.max_reads;
    const long long take = found < room ? found : room;           // the first `room` units in read order; the rest stay flagged
    BBHIP(hipMemcpyAsync(c->d_tierUnits, ids.data(), 4 * (size_t)take, hipMemcpyHostToDevice, s));
    BBTRY(launch<128>(gather_reads_kernel, take, s, B.reads, c->d_tierUnits, (int)take, paired, c->d_tierReads, c->d_tierReadIds));
    BBHIP(hipStreamSynchronize(s));                                // `ids` is done with
    const long long tn = paired ? 2 * take : take;
    // the reverse complements of these reads are in place (the main probe wrote them)
    BBTRY(map_records(t, s, tn, c->d_tierReads, B.bases, B.minus_delta, B.baseScores, B.keyinfo, false));
    c->tierReads = tn;
    return BBMAP_OK;
}

static void tier_start_async(bbmap_ctx *c, long long found) {
    c->tierStarted = true; c->tierRc = BBMAP_OK; c->tierErr[0] = 0;
    c->tierThread = std::thread([c, found]() {
        int rc = hipSetDevice(c->cfg.device) == hipSuccess ? BBMAP_OK : BBMAP_E_HIP;
        if (rc == BBMAP_OK) rc = tier_pass(c, c->tierStream, found);
        if (rc != BBMAP_OK) { snprintf(c->tierErr, sizeof c->tierErr, "overflow tier: %s", bbmap_last_error()); }
        c->tierRc = rc;
    });
}

// after the tier's pass: its reads are marked in the main list, its counts join the batch's statistics
static int tier_finish(bbmap_ctx *c, hipStream_t stream) {
    bbmap_ctx *t = c->tier;
    const long long tn = c->tierReads;
    if (tn == 0) return BBMAP_OK;
    BBHIP(hipMemsetAsync(c->d_counters + CNT_TIER_RESOLVED, 0, 4, stream));
    BBTRY(launch<128>(mark_tier_kernel, tn, stream, c->d_mcount, t->d_mcount, c->d_tierReadIds, (int)tn, c->d_counters + CNT_TIER_RESOLVED));
    BBTRY(read_counters(c, stream));
    bbmap_stats &st = c->stats; const bbmap_stats &ts = t->stats;
    st.reads_reprobed = tn;
    st.reads_overflowed -= (long long)c->h_counters[CNT_TIER_RESOLVED];
    st.reads_without_site += ts.reads_without_site;
    st.fills += ts.fills; st.gapped_fills += ts.gapped_fills; st.refills += ts.refills; st.rescue_scans += ts.rescue_scans;
    st.rescue_fills += ts.rescue_fills; st.fills_dropped += ts.fills_dropped;
    st.final_fills += ts.final_fills; st.final_local += ts.final_local;
    st.dp_narrow_launches += ts.dp_narrow_launches; st.dp_sorted_launches += ts.dp_sorted_launches;
    st.sites_cross_scaffold += ts.sites_cross_scaffold;
    if (getenv("BBMAP_TIER_DEBUG"))
        fprintf(stderr, "[bbmap tier] reads %lld: probe %.2f begin %.2f score %.2f slow %.2f (rounds %lld) finish %.2f rescue %.2f total %.2f\n",
                tn, ts.ms_probe, ts.ms_begin, ts.ms_score, ts.ms_slow, (long long)ts.rounds, ts.ms_finish, ts.ms_rescue, ts.ms_total);
    return BBMAP_OK;
}

// ---- the adaptive state (bbmap_set_adaptive): rules over the run statistics that bbmap_map_batch_device applies around a batch
// `if(mappedRetained2>1000 && numMated*20L<mappedRetained2){return;}` (AbstractMapThread.java:1146) on the running counters
static int rescue_skip_rule(bbmap_ctx *c, bool *skip) {
    *skip = false;
    if (!c->d_runStats) return BBMAP_OK;
    bbmap_runstats rs;
    BBHIP(hipStreamSynchronize(c->accum[ACC_STATS].stream));        // not the device: only that stream's work writes the counters
    BBHIP(hipMemcpy(&rs, c->d_runStats, sizeof rs, hipMemcpyDeviceToHost));
    *skip = rs.mappedRetained2 > 1000 && rs.numMated * 20LL < rs.mappedRetained2;
    return BBMAP_OK;
}

// `if(DYNAMIC_INSERT_LENGTH && numMated>1000 && r.paired()){AVERAGE_PAIR_DIST=(int)(innerLengthSum*1f/numMated);}`
// (BBMapThread.java:1307-1309) once per batch.  "The batch held a paired read" is tested as "numMated moved": calcStatistics1 adds one
// to numMated for exactly the pairs whose mate 1 is paired() (AbstractMapThread.java:1542-1543; a paired read is mapped), so the two are
// equivalent.  Java's arithmetic: long -> float,
// float * 1f, numMated -> float, float division, truncation (this file is compiled with contraction off).  One deviation: inner
// lengths clamp at MIN_PAIR_DIST -160, so the quotient can be negative and Java would store it; bbmap_set_average_pair_dist takes no
// negative distance (the pairing code never met one), so a negative quotient leaves the value as it was.
static int adapt_after_batch(bbmap_ctx *c, hipStream_t stream) {
    if (!(c->adaptive & BBMAP_ADAPT_INSERT_LENGTH)) return BBMAP_OK;
    bbmap_runstats rs;
    BBHIP(hipMemcpyAsync(&rs, c->d_runStats, sizeof rs, hipMemcpyDeviceToHost, stream));
    BBHIP(hipStreamSynchronize(stream));
    const bool heldPaired = rs.numMated > c->numMatedSeen;
    c->numMatedSeen = rs.numMated;
    if (rs.numMated > 1000 && heldPaired) {
        volatile float sum = (float)rs.innerLengthSum, cnt = (float)rs.numMated;
        const float q = sum * 1.0f / cnt;
        const int v = (int)q;
        if (v >= 0) BBTRY(bbmap_set_average_pair_dist(c, v));
    }
    return BBMAP_OK;
}

extern "C" int bbmap_get_adaptive_state(bbmap_ctx *c, int32_t *averagePairDist, int32_t *rescueSkipped) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_get_adaptive_state: null context");
    if (averagePairDist) *averagePairDist = c->cfg.averagePairDist;
    if (rescueSkipped) {
        bool skip = false;
        if (c->adaptive & BBMAP_ADAPT_RESCUE_SKIP) { BBHIP(hipSetDevice(c->cfg.device)); BBTRY(rescue_skip_rule(c, &skip)); }
        *rescueSkipped = skip ? 1 : 0;
    }
    return BBMAP_OK;
}

static int map_batch_device(bbmap_ctx *c, hipStream_t stream, int64_t n_reads, const bbidx_read *reads, uint8_t *bases,
                            int64_t minus_delta, const int8_t *baseScores, const int32_t *keyinfo) {
    c->batch = {n_reads, reads, bases, minus_delta, baseScores, keyinfo};
    c->tierStarted = false; c->tierReads = 0;
    if (c->tier) c->tier->ran = false;
    const int rc = map_records(c, stream, n_reads, reads, bases, minus_delta, baseScores, keyinfo, true);
    hipEvent_t e0 = c->ev[EV_TIER_BEGIN], e1 = c->ev[EV_TIER_END];
    // the tier's helper thread is joined before anything else can return: a joinable std::thread left behind would terminate the
    // process at the next batch's assignment
    if (c->tierStarted) {
        c->tierThread.join();
        if (rc == BBMAP_OK && c->tierRc != BBMAP_OK) return bbfail(c->tierRc, "%s", c->tierErr);
    }
    BBTRY(rc);
    if (c->tier) BBHIP(hipEventRecord(e0, stream));
    if (!c->tier || c->stats.reads_overflowed == 0) return BBMAP_OK;
    if (c->stats.reads_overflowed > c->overAfterBegin || !c->tierStarted) {
        // lists that outgrew max_sites in rescue: one more tier pass, over every flagged read
        const long long units = c->cfg.paired ? n_reads / 2 : n_reads;
            BBHIP(hipMemsetAsync(c->d_counters + CNT_TIER_FOUND, 0, 4, stream));
        BBTRY(launch<128>(collect_overflow_kernel, units, stream, c->d_mcount, units, c->cfg.paired, c->d_tierUnits, c->d_counters + CNT_TIER_FOUND));
        BBTRY(read_counters(c, stream));
        if (c->h_counters[CNT_TIER_FOUND] > 0) BBTRY(tier_pass(c, stream, c->h_counters[CNT_TIER_FOUND]));
    }
    BBTRY(tier_finish(c, stream));
    BBHIP(hipEventRecord(e1, stream));
    BBHIP(hipStreamSynchronize(stream));
    (void)hipEventElapsedTime(&c->stats.ms_overflow, e0, e1);      // what the tier added to the batch after the main pass
    c->stats.ms_total += c->stats.ms_overflow;
    return BBMAP_OK;
}

extern "C" int bbmap_map_batch_device(bbmap_ctx *c, void *stream_, int64_t n_reads, const bbidx_read *reads, uint8_t *bases,
                                      int64_t minus_delta, const int8_t *baseScores, const int32_t *keyinfo) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_map_batch_device: null context");
    if (n_reads < 0 || n_reads > c->cfg.max_reads) return bbfail(BBMAP_E_ARG, "bbmap_map_batch_device: more reads than the context was made for");
    if (c->cfg.paired && (n_reads & 1)) return bbfail(BBMAP_E_ARG, "bbmap_map_batch_device: paired mode takes an even number of reads");
    if (n_reads == 0) { c->ran = false; c->truthNext = nullptr; return BBMAP_OK; }      // (the truth array was for this batch alone)
    if (!reads || !bases || !baseScores || !keyinfo) return bbfail(BBMAP_E_ARG, "bbmap_map_batch_device: null buffer");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    c->new_batch();
    const bbmap_truth *truth = c->truthNext;
    c->truthNext = nullptr;
    bool skip = false;
    if (c->adaptive & BBMAP_ADAPT_RESCUE_SKIP) BBTRY(rescue_skip_rule(c, &skip));
    c->S.rescueSkip = skip ? 1 : 0;
    if (c->tier) c->tier->S.rescueSkip = c->S.rescueSkip;
    BBTRY(map_batch_device(c, stream, n_reads, reads, bases, minus_delta, baseScores, keyinfo));
    if (c->adaptive && c->S.finalStage) {
        BBTRY(bbmap_add_run_stats(c, stream, truth));
        BBTRY(adapt_after_batch(c, stream));
    }
    return BBMAP_OK;
}

// The final alignment stage alone, over site lists the caller provides (see include/bbmap_amd.h).
extern "C" int bbmap_final_batch_device(bbmap_ctx *c, void *stream_, int64_t n_reads, const bbidx_read *reads, uint8_t *bases, int64_t minus_delta,
                                        const bbmap_msite *sites, const int32_t *nsites) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_final_batch_device: null context");
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_final_batch_device: the context was created without the final stage");
    if (n_reads < 1 || n_reads > c->cfg.max_reads || (c->cfg.paired && (n_reads & 1))) return bbfail(BBMAP_E_ARG, "bbmap_final_batch_device: bad read count");
    if (!reads || !bases || !sites || !nsites) return bbfail(BBMAP_E_ARG, "bbmap_final_batch_device: null buffer");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    c->tierStarted = false; c->tierReads = 0;
    if (c->tier) c->tier->ran = false;
    c->new_batch();
    memset(&c->stats, 0, sizeof c->stats);
    c->stats.reads = n_reads;
    c->batch = {n_reads, reads, bases, minus_delta, nullptr, nullptr};
    BBHIP(hipMemsetAsync(c->d_counters, 0, CNT_WORDS * 4, stream));
    BBHIP(hipMemsetAsync(c->d_slow, 0, sizeof(SlowState) * (size_t)n_reads, stream));      // fills are numbered from 0
    BBHIP(hipMemcpyAsync(c->d_ms, sites, sizeof(bbmap_msite) * (size_t)n_reads * (size_t)c->cfg.max_sites, hipMemcpyDeviceToDevice, stream));
    BBHIP(hipMemcpyAsync(c->d_mcount, nsites, 4 * (size_t)n_reads, hipMemcpyDeviceToDevice, stream));
    BBHIP(hipEventRecord(c->ev[EV_RESCUE_END], stream));
    Dev D;
    fill_dev(c, D, n_reads, reads, bases, minus_delta);
    long long finalRounds = 0, finalLocal = 0;
    BBTRY(run_final_stage(c, stream, D, n_reads, bases, 0, 0, finalRounds, finalLocal));
    BBTRY(finish_stats(c, stream, false, 0, finalRounds, finalLocal));
    c->ran = true;
    return BBMAP_OK;
}
