// Host side of the k-mer index probe's C ABI (include/bbmap_amd.h): the index context, its launch states, the dispatcher that
// chooses between the wave kernel (index_probe_wave.hip), the long-read kernel (index_probe_long.hip) and the lane kernel
// (index_probe.hip), and what reads a finished launch.  bbidx_build (index_build.hip) ends in bbidx_finish_create here.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>
#include <vector>

#include "bbmap_amd.h"
#include "host_common.h"
#include "index_ctx.h"

namespace bbidx {

__global__ void build_fused_kernel(KeyEntry *out, const int *starts, const int *sites, const int *counts, int k, long long nkeys) {
    const long long key = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= nkeys) return;
    const int rc = rc_key((int)key, k);
    KeyEntry e;
    e.cnt = counts[key]; e.cntRC = counts[rc];
    e.startF = starts[key]; e.lenF = starts[key + 1] - e.startF; e.firstF = e.lenF > 0 ? sites[e.startF] : 0;
    e.startR = starts[rc]; e.lenR = starts[rc + 1] - e.startR; e.firstR = e.lenR > 0 ? sites[e.startR] : 0;
    out[key] = e;
}

}  // namespace bbidx

template <typename T>
static int upload(bbidx_ctx *c, const T *host, size_t count, const T **dev) {
    void *d = nullptr;
    BBHIP(hipMalloc(&d, (count > 0 ? count : 1) * sizeof(T)));
    c->allocs.push_back(d);
    if (count > 0) BBHIP(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    *dev = (const T *)d;
    return BBMAP_OK;
}

int bbidx_finish_create(bbidx_ctx *c, const std::vector<const int *> &hs, const std::vector<const int *> &hsi) {
    const bbidx_params &p = c->dev.p;
    const size_t keyspace = (size_t)1 << (2 * p.k);
    const int nblocks = c->dev.nblocks;
    int rc = BBMAP_OK;
    {
        // fused per-key records for the wave kernel; if HBM cannot hold them the context stays on the per-lane kernel
        std::vector<const bbidx::KeyEntry *> hf((size_t)nblocks, nullptr);
        bool ok = true;
        for (int b = 0; b < nblocks && ok; b++) {
            void *f = nullptr;
            if (hipMalloc(&f, keyspace * sizeof(bbidx::KeyEntry)) != hipSuccess) { (void)hipGetLastError(); ok = false; break; }
            c->allocs.push_back(f);
            hf[(size_t)b] = (const bbidx::KeyEntry *)f;
            hipLaunchKernelGGL(bbidx::build_fused_kernel, dim3((unsigned)((keyspace + 255) / 256)), dim3(256), 0, nullptr,
                               (bbidx::KeyEntry *)f, hs[(size_t)b], hsi[(size_t)b], c->dev.counts, p.k, (long long)keyspace);
            if (hipGetLastError() != hipSuccess) ok = false;
        }
        if (ok && hipDeviceSynchronize() != hipSuccess) ok = false;
        c->dev.fused = nullptr;
        if (ok) rc = upload(c, hf.data(), hf.size(), (const bbidx::KeyEntry *const **)&c->dev.fused);
        else c->kernelKind = BBIDX_KERNEL_LANE;
    }
    if (rc == BBMAP_OK) rc = bbidx_launch_init(c, &c->own);
    return rc;
}

int bbidx_launch_init(bbidx_ctx *c, bbidx_launch *ls) {
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipMalloc(&ls->d_queue, 64));
    BBHIP(hipMalloc(&ls->d_stats, bbidx::STAT_SHARDS * 64));
    BBHIP(hipEventCreate(&ls->ev[0]));
    BBHIP(hipEventCreate(&ls->ev[1]));
    ls->timed = false; ls->d_longWs = nullptr; ls->longBlocks = 0;
    return BBMAP_OK;
}
void bbidx_launch_free(bbidx_launch *ls) {
    if (!ls) return;
    if (ls->d_queue) (void)hipFree(ls->d_queue);
    if (ls->d_stats) (void)hipFree(ls->d_stats);
    if (ls->d_longWs) (void)hipFree(ls->d_longWs);
    if (ls->ev[0]) (void)hipEventDestroy(ls->ev[0]);
    if (ls->ev[1]) (void)hipEventDestroy(ls->ev[1]);
    *ls = bbidx_launch();
}

int bbidx_env_max_groups() {
    const int v = env_int("BBIDX_MAX_GROUPS", 0);
    return v > 0 ? v : 0;
}

extern "C" int bbidx_create(int32_t device, const bbidx_index_desc *d, bbidx_ctx **out) {
    if (!d || !out) return bbfail(BBMAP_E_ARG, "bbidx_create: null argument");
    *out = nullptr;
    const bbidx_params &p = d->params;
    if (p.k < 8 || p.k > 15 || p.chromBits < 0 || p.chromBits > 16 || d->nblocks < 1 || d->nchroms < 1)
        return bbfail(BBMAP_E_ARG, "bbidx_create: bad index geometry (k must be 8..15)");
    if (p.profile != BBIDX_PROFILE_BBMAP && p.profile != BBIDX_PROFILE_PACBIO) return bbfail(BBMAP_E_ARG, "bbidx_create: unknown profile");
    for (int b = 0; b < d->nblocks; b++)
        if (d->numSites[b] < 0 || (long long)d->numSites[b] > 0x7fffffffLL - 64)
            return bbfail(BBMAP_E_ARG, "bbidx_create: a block holds more than 2^31 - 64 sites");
    hipDeviceProp_t prop;
    BBTRY(bb_use_gfx950("bbidx_create", device, &prop));
    bbidx_ctx *c = new (std::nothrow) bbidx_ctx();
    if (!c) return bbfail(BBMAP_E_NOMEM, "bbidx_create: out of memory");
    c->device = device;
    c->kernelKind = BBIDX_KERNEL_AUTO;
    c->blocks = prop.multiProcessorCount * 8;
    c->totalSites = 0; c->maxReadLen = BBIDX_MAX_READ_LEN;
    c->maxGroups = bbidx_env_max_groups();
    for (int b = 0; b < d->nblocks; b++) c->totalSites += (long long)d->numSites[b];
    const size_t keyspace = (size_t)1 << (2 * p.k);
    int rc = BBMAP_OK;
    std::vector<const int *> hs((size_t)d->nblocks), hsi((size_t)d->nblocks);
    std::vector<const uint8_t *> hc((size_t)d->nchroms + 1, nullptr);
    c->dev.p = p; c->dev.nblocks = d->nblocks; c->dev.nchroms = d->nchroms;
    for (int b = 0; b < d->nblocks && rc == BBMAP_OK; b++) {
        rc = upload(c, d->starts[b], keyspace + 1, &hs[(size_t)b]);
        if (rc == BBMAP_OK) rc = upload(c, d->sites[b], (size_t)d->numSites[b], &hsi[(size_t)b]);
    }
    for (int ch = 1; ch <= d->nchroms && rc == BBMAP_OK; ch++) rc = upload(c, d->chromArr[ch], (size_t)d->chromArrLen[ch], &hc[(size_t)ch]);
    if (rc == BBMAP_OK) rc = upload(c, hs.data(), hs.size(), (const int *const **)&c->dev.starts);
    if (rc == BBMAP_OK) rc = upload(c, hsi.data(), hsi.size(), (const int *const **)&c->dev.sites);
    if (rc == BBMAP_OK) rc = upload(c, hc.data(), hc.size(), (const uint8_t *const **)&c->dev.chromArr);
    if (rc == BBMAP_OK) rc = upload(c, d->counts, keyspace, &c->dev.counts);
    if (rc == BBMAP_OK) rc = upload(c, d->lengthHistogram, (size_t)1001, &c->dev.lengthHistogram);
    if (rc == BBMAP_OK) rc = upload(c, d->chromArrLen, (size_t)d->nchroms + 1, &c->dev.chromArrLen);
    if (rc == BBMAP_OK) rc = upload(c, d->chromLengths, (size_t)d->nchroms + 1, &c->dev.chromLengths);
    if (rc == BBMAP_OK) rc = bbidx_finish_create(c, hs, hsi);
    if (rc != BBMAP_OK) { bbidx_destroy(c); return rc; }
    *out = c;
    return BBMAP_OK;
}

extern "C" void bbidx_destroy(bbidx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->scafBuf) (void)hipFree(c->scafBuf);
    bbidx_launch_free(&c->own);
    delete c;
}

extern "C" int bbidx_find_batch_device(bbidx_ctx *c, void *stream_, int64_t n, const bbidx_read *reads,
                                       const uint8_t *bases, const int8_t *baseScores, const int32_t *keyinfo,
                                       bbidx_site *sites, int32_t max_sites, int32_t *nsites) {
    return bbidx_find_batch_device_rc(c, stream_, n, reads, bases, baseScores, keyinfo, sites, max_sites, nsites, nullptr);
}

extern "C" int bbidx_find_batch_device_rc(bbidx_ctx *c, void *stream_, int64_t n, const bbidx_read *reads,
                                          const uint8_t *bases, const int8_t *baseScores, const int32_t *keyinfo,
                                          bbidx_site *sites, int32_t max_sites, int32_t *nsites, uint8_t *bases_rc_out) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbidx_find_batch_device: null context");
    return bbidx_find_batch_device_with(c, &c->own, stream_, n, reads, bases, baseScores, keyinfo, sites, max_sites, nsites, bases_rc_out);
}

int bbidx_find_batch_device_with(bbidx_ctx *c, bbidx_launch *ls, void *stream_, int64_t n, const bbidx_read *reads,
                                 const uint8_t *bases, const int8_t *baseScores, const int32_t *keyinfo,
                                 bbidx_site *sites, int32_t max_sites, int32_t *nsites, uint8_t *bases_rc_out) {
    if (!c || !ls) return bbfail(BBMAP_E_ARG, "bbidx_find_batch_device: null context");
    if (n < 0 || n > 0x7fffffffLL || max_sites < 1) return bbfail(BBMAP_E_ARG, "bbidx_find_batch_device: bad size");
    if (n == 0) return BBMAP_OK;
    if (!reads || !bases || !baseScores || !keyinfo || !sites || !nsites) return bbfail(BBMAP_E_ARG, "bbidx_find_batch_device: null buffer");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipMemsetAsync(ls->d_queue, 0, 64, stream));
    BBHIP(hipMemsetAsync(ls->d_stats, 0, bbidx::STAT_SHARDS * 64, stream));
    bbidx::Params P;
    P.stats = ls->d_stats;
    P.ix = c->dev; P.reads = reads; P.bases = bases; P.baseScores = baseScores; P.keyinfo = keyinfo;
    P.sites = sites; P.nsites = nsites; P.nreads = n; P.maxSites = max_sites; P.queue = ls->d_queue;
    P.onlyPending = 0;
    P.rcOut = bases_rc_out;
    long long blocks = (n + 63) / 64;
    if (blocks > c->blocks) blocks = c->blocks;
    if (c->maxGroups > 0 && blocks > c->maxGroups) blocks = c->maxGroups;
    ls->waveGroups = ls->lastLaneGroups = ls->lastLongGroups = 0;
    ls->waveLongLists = ls->waveShort = ls->longMaxLen = ls->longMaxKeys = 0;
    BBHIP(hipEventRecord(ls->ev[0], stream));
    if (c->dev.p.profile == BBIDX_PROFILE_PACBIO || c->kernelKind == BBIDX_KERNEL_LONG) {
        // mapPacBio's reads (thousands of bases, hundreds of keys), or the long-read kernel asked for by name
        if (!c->dev.fused) return bbfail(BBMAP_E_NOMEM, "bbidx_find_batch_device: the long-read kernel needs the fused key table, which could not be allocated");
        if (!ls->d_longWs) {
            ls->longBlocks = bbidx_long_blocks(c->dev.p.profile == BBIDX_PROFILE_PACBIO ? 1 : 0);
            if (ls->longBlocks < 1) return bbfail(BBMAP_E_HIP, "bbidx_find_batch_device: the long-read kernel does not fit this device");
            BBHIP(hipMalloc(&ls->d_longWs, (size_t)ls->longBlocks * (size_t)bbidx_long_workspace_ints_per_block() * 4));
        }
        BBTRY(bbidx_launch_long(P, stream, c->dev.p.profile == BBIDX_PROFILE_PACBIO ? 1 : 0, ls->d_longWs, ls->longBlocks, c->maxGroups, ls));
        BBHIP(hipEventRecord(ls->ev[1], stream));
        ls->timed = true;
        return BBMAP_OK;
    }
    if (c->kernelKind == BBIDX_KERNEL_AUTO) {
        // one read per wavefront; reads it cannot take (more than 64 keys) are marked and picked up by the per-lane kernel
        // average list length >= 1/2: the variant with batched pops / bulk skips (it gates them per strand by list size);
        // below that (small genomes) the plain variant, which is a few per cent faster there
        bool longLists = c->totalSites * 2 >= (1LL << (2 * c->dev.p.k)) * (long long)c->dev.nblocks;
        if (const char *ev = getenv("BBIDX_LONG_LISTS")) { if (*ev) longLists = atoi(ev) != 0; }      // tests force either variant
        bool shortReads = false;
        BBTRY(bbidx_launch_wave(P, stream, longLists, c->maxReadLen, c->maxGroups, &ls->waveGroups, &shortReads));
        ls->waveLongLists = longLists ? 1 : 0; ls->waveShort = shortReads ? 1 : 0;
        P.onlyPending = 1;
    }
    hipLaunchKernelGGL(bbidx::probe_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, P);
    BBHIP(hipGetLastError());
    ls->lastLaneGroups = blocks;
    BBHIP(hipEventRecord(ls->ev[1], stream));
    ls->timed = true;
    return BBMAP_OK;
}

extern "C" int bbidx_find_batch(bbidx_ctx *c, int64_t n, const bbidx_read *reads, const uint8_t *bases, const int8_t *baseScores,
                                int64_t bases_bytes, const int32_t *keyinfo, int64_t keyinfo_ints,
                                bbidx_site *sites, int32_t max_sites, int32_t *nsites) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbidx_find_batch: null context");
    if (n == 0) return BBMAP_OK;
    if (n < 0 || !reads || !bases || !baseScores || !keyinfo || !sites || !nsites || max_sites < 1)
        return bbfail(BBMAP_E_ARG, "bbidx_find_batch: bad argument");
    for (int64_t i = 0; i < n; i++) {
        const bbidx_read &r = reads[i];
        if (r.len < 0 || r.nkeys < 0 || r.bases_off < 0 || r.keys_off < 0 || r.bases_off + r.len > bases_bytes ||
            r.keys_off + 2LL * r.nkeys > keyinfo_ints)
            return bbfail(BBMAP_E_ARG, "bbidx_find_batch: a read lies outside its buffers");
        for (int q = 0; q < r.nkeys && q < BBIDX_PACBIO_MAX_KEYS; q++) {
            const int o = keyinfo[r.keys_off + q];
            if (o < 0 || o + c->dev.p.k > r.len) return bbfail(BBMAP_E_ARG, "bbidx_find_batch: a key offset lies outside its read");
        }
    }
    BBHIP(hipSetDevice(c->device));
    DevTmp<bbidx_read> dr; DevTmp<uint8_t> db; DevTmp<int8_t> dq; DevTmp<int32_t> dk, dn; DevTmp<bbidx_site> ds;
    BBTRY(dr.upload(reads, (size_t)n));
    BBTRY(db.upload(bases, (size_t)bases_bytes));
    BBTRY(dq.upload(baseScores, (size_t)bases_bytes));
    BBTRY(dk.upload(keyinfo, (size_t)keyinfo_ints));
    BBTRY(dn.alloc((size_t)n));
    BBTRY(ds.alloc((size_t)n * (size_t)max_sites));
    BBTRY(bbidx_find_batch_device(c, nullptr, n, dr, db, dq, dk, ds, max_sites, dn));
    BBHIP(hipStreamSynchronize(nullptr));
    BBHIP(hipMemcpy(nsites, dn, (size_t)n * 4, hipMemcpyDeviceToHost));
    BBHIP(hipMemcpy(sites, ds, (size_t)n * (size_t)max_sites * sizeof(bbidx_site), hipMemcpyDeviceToHost));
    return BBMAP_OK;
}

// Work counters and duration of the last bbidx_find_batch_device launch (valid once its stream has been synchronised):
// stats[0..4] = list entries consumed by the prescan, by the walk, extendScore calls, reference bytes compared,
// site records written.
extern "C" int bbidx_last_stats(bbidx_ctx *c, int64_t *stats5, float *kernel_ms) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbidx_last_stats: null context");
    return bbidx_last_stats_with(c, &c->own, stats5, kernel_ms);
}
int bbidx_last_stats_with(bbidx_ctx *c, bbidx_launch *ls, int64_t *stats5, float *kernel_ms) {
    if (!c || !ls || !ls->timed) return bbfail(BBMAP_E_ARG, "bbidx_last_stats: nothing launched yet");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(ls->ev[1]));
    if (kernel_ms) BBHIP(hipEventElapsedTime(kernel_ms, ls->ev[0], ls->ev[1]));
    if (stats5) {
        std::vector<unsigned long long> h((size_t)bbidx::STAT_SHARDS * 8);
        BBHIP(hipMemcpy(h.data(), ls->d_stats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int j = 0; j < 5; j++) stats5[j] = 0;
        for (int s = 0; s < bbidx::STAT_SHARDS; s++) for (int j = 0; j < 5; j++) stats5[j] += (int64_t)h[(size_t)s * 8 + j];
    }
    return BBMAP_OK;
}

// What the last bbidx_find_batch_device launch ran (waits for it): launch8 = {wave-kernel groups, long-list variant (0/1),
// short-read instantiation (0/1), reads the wave kernel left to the per-lane kernel (queue[1]), per-lane kernel groups,
// long-read kernel groups, the long kernel's maxLen, its maxKeys}; 0 for a kernel that did not run.
extern "C" int bbidx_last_launch(bbidx_ctx *c, int64_t *launch8) {
    if (!c || !launch8) return bbfail(BBMAP_E_ARG, "bbidx_last_launch: null argument");
    bbidx_launch *ls = &c->own;
    if (!ls->timed) return bbfail(BBMAP_E_ARG, "bbidx_last_launch: nothing launched yet");
    BBHIP(hipSetDevice(c->device));
    BBHIP(hipEventSynchronize(ls->ev[1]));
    unsigned int pending = 0;
    if (ls->waveGroups > 0) BBHIP(hipMemcpy(&pending, ls->d_queue + 1, sizeof pending, hipMemcpyDeviceToHost));
    launch8[0] = ls->waveGroups; launch8[1] = ls->waveLongLists; launch8[2] = ls->waveShort; launch8[3] = pending;
    launch8[4] = ls->lastLaneGroups; launch8[5] = ls->lastLongGroups; launch8[6] = ls->longMaxLen; launch8[7] = ls->longMaxKeys;
    return BBMAP_OK;
}

extern "C" int bbidx_set_max_read_len(bbidx_ctx *c, int32_t max_len) {
    if (!c || max_len < 1) return bbfail(BBMAP_E_ARG, "bbidx_set_max_read_len: bad argument");
    c->maxReadLen = max_len;
    return BBMAP_OK;
}

extern "C" int bbidx_set_kernel(bbidx_ctx *c, int32_t kind) {
    if (!c || (kind != BBIDX_KERNEL_AUTO && kind != BBIDX_KERNEL_LANE && kind != BBIDX_KERNEL_LONG)) return bbfail(BBMAP_E_ARG, "bbidx_set_kernel: bad argument");
    if (c->dev.p.profile == BBIDX_PROFILE_PACBIO && kind != BBIDX_KERNEL_LONG && kind != BBIDX_KERNEL_AUTO)
        return bbfail(BBMAP_E_ARG, "bbidx_set_kernel: a BBIDX_PROFILE_PACBIO context only has the long-read kernel");
    if (kind != BBIDX_KERNEL_LANE && !c->dev.fused) return bbfail(BBMAP_E_NOMEM, "bbidx_set_kernel: the fused key table could not be allocated");
    c->kernelKind = kind;
    return BBMAP_OK;
}
