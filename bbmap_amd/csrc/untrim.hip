// bbmap_untrim_batch_device: align2.TrimRead.untrim (current/align2/TrimRead.java:415-463) and untrim(SiteScore) (:465-508) over the last
// batch's final records, site lists and match strings, overflow tier included.  AbstractMapThread.run calls it behind processRead
// (current/align2/AbstractMapThread.java:518-521), so everything that prints a read sees the full read with its trimmed ends as soft
// clips ('C' in the long match format).
//
// The strings grow by left + right bytes, so they cannot stay where they are: a sizing pass (bytes of a read's strings after padding,
// each in 4-byte units as the pool hands them out), a device-wide exclusive scan, and an emit pass that copies every string into a
// second pool and rewrites the records; then the context's two pools change places.  Both passes take one wavefront per read: the
// lanes share a string's bytes, lane 0 writes the record.  Every string gets a copy of its own in the new pool.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mapper_ctx.h"
#include "scan_offsets.h"

using namespace bbmapper;

namespace bbuntrim {

struct Args {
    bbmap_final *fin; bbmap_msite *sites; const int *nsites; int cap;
    const uint8_t *pool; long long poolBytes;          // the pool in use and the bytes of it that hold strings
    const int *ids;                                     // record i is batch read ids[i] (the overflow tier); null: read i
    const bbtrim_rec *trims;                            // per batch read
    long long n;
};

__device__ inline long long units4(long long bytes) { return (bytes + 3) & ~3ll; }
// a string the records refer to: inside the pool, or treated as absent
__device__ inline bool in_pool(const Args &a, long long off, int len) { return len > 0 && off >= 0 && off + len <= a.poolBytes; }
__device__ inline int site_count(const Args &a, long long i) { const int n = a.nsites[i]; return n < 0 ? 0 : (n > a.cap ? a.cap : n); }

// counts[i] = bytes of the new pool that record i's strings take
__global__ void __launch_bounds__(256) size_kernel(Args a, int *counts) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= a.n) return;
    const bbtrim_rec t = a.trims[a.ids ? a.ids[i] : i];
    const int pad = t.left + t.right;
    long long bytes = 0;
    if (lane == 0) {
        const bbmap_final f = a.fin[i];
        if (in_pool(a, f.match_off, f.match_len)) bytes += units4((long long)f.match_len + pad);
    }
    const bbmap_msite *list = a.sites + i * a.cap;
    for (int s = lane, ns = site_count(a, i); s < ns; s += 64) {
        const int at = list[s].reserved[0], len = list[s].reserved[1] & 0x7fffffff;
        if (at > 0 && in_pool(a, 4ll * (at - 1), len)) bytes += units4((long long)len + pad);
    }
    for (int d = 32; d > 0; d >>= 1) bytes += __shfl_xor(bytes, d, 64);
    if (lane == 0) counts[i] = (int)bytes;
}

// dst = lt x 'C' + src[0 .. len) + rt x 'C', one byte per lane and turn
__device__ inline void pad_copy(uint8_t *dst, const uint8_t *src, int len, int lt, int rt, int lane) {
    for (int k = lane; k < lt; k += 64) dst[k] = 'C';
    for (int k = lane; k < len; k += 64) dst[lt + k] = src[k];
    for (int k = lane; k < rt; k += 64) dst[lt + len + k] = 'C';
}

__global__ void __launch_bounds__(256) emit_kernel(Args a, const long long *offsets, uint8_t *out) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= a.n) return;
    const bbtrim_rec t = a.trims[a.ids ? a.ids[i] : i];
    const bool trimmed = t.left + t.right > 0;
    long long at = offsets[i];                          // the next free byte of this record's share (a multiple of 4)
    {   // the record: TrimRead.untrim() :415-463
        bbmap_final *fp = a.fin + i;
        const bbmap_final f = *fp;
        const int lt = f.strand == 0 ? t.left : t.right, rt = f.strand == 0 ? t.right : t.left;
        const bool has = in_pool(a, f.match_off, f.match_len);
        if (has) pad_copy(out + at, a.pool + f.match_off, f.match_len, lt, rt, lane);
        if (lane == 0) {
            if (trimmed) {
                fp->perfect = 0;
                if (f.mapped) { fp->start = f.start - lt; fp->stop = f.stop + rt; }      // (an unmapped record keeps -1 / -1)
            }
            if (has) { fp->match_off = at; fp->match_len = f.match_len + lt + rt; }
            else if (f.match_len > 0) { fp->match_off = 0; fp->match_len = 0; }
        }
        if (has) at += units4((long long)f.match_len + lt + rt);
    }
    bbmap_msite *list = a.sites + i * a.cap;
    for (int s = 0, ns = site_count(a, i); s < ns; s++) {       // untrim(SiteScore) :465-508
        bbmap_msite *sp = list + s;
        const int strand = sp->strand, start = sp->start, stop = sp->stop, ref = sp->reserved[0], len = sp->reserved[1] & 0x7fffffff;
        const int lt = strand == 0 ? t.left : t.right, rt = strand == 0 ? t.right : t.left;
        const bool has = ref > 0 && in_pool(a, 4ll * (ref - 1), len);
        if (has) pad_copy(out + at, a.pool + 4ll * (ref - 1), len, lt, rt, lane);
        if (lane == 0) {
            if (trimmed) { sp->start = start - lt; sp->stop = stop + rt; sp->perfect = 0; sp->semiperfect = 0; }
            if (has) { sp->reserved[0] = (int)(at / 4 + 1); sp->reserved[1] = len + lt + rt; }
            else if (ref > 0) { sp->reserved[0] = 0; sp->reserved[1] = 0; }
        }
        if (has) at += units4((long long)len + lt + rt);
    }
}

// one context's records (the main one's, or the overflow tier's with ids = the tier's read numbers)
static int untrim_ctx(bbmap_ctx *c, hipStream_t stream, long long n, const int *ids, const bbtrim_rec *trims) {
    if (n <= 0) return BBMAP_OK;
    if (!c->d_untrimCounts) {
        BBTRY(dalloc(c, &c->d_untrimCounts, (size_t)c->cfg.max_reads + 1));
        BBTRY(dalloc(c, &c->d_untrimOffsets, (size_t)c->cfg.max_reads + 1));
    }
    Args a;
    a.fin = c->d_final; a.sites = c->d_ms; a.nsites = c->d_mcount; a.cap = c->cfg.max_sites;
    a.pool = c->d_pool; a.poolBytes = c->poolUsed; a.ids = ids; a.trims = trims; a.n = n;
    BBTRY(launch<256>(size_kernel, 64 * n, stream, a, c->d_untrimCounts));
    long long total = 0;
    BBTRY(scan_offsets(c->d_untrimCounts, n, c->d_untrimOffsets, c->untrimTmp, stream, &total));
    if (total / 4 > 0x7ffffff0LL) return bbfail(BBMAP_E_NOMEM, "bbmap_untrim_batch_device: the match strings exceed 8 GB; map smaller batches");
    if (!c->d_pool2 || c->pool2Units * 4 < total) {         // (the stream has just been waited for: nothing reads the old one)
        const long long units = std::max(c->poolUnits, total / 4 + 16384);
        if (c->d_pool2) {
            c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void *)c->d_pool2), c->allocs.end());
            (void)hipFree(c->d_pool2);
            c->d_pool2 = nullptr; c->pool2Units = 0;
        }
        BBTRY(dalloc(c, &c->d_pool2, (size_t)units * 4));
        c->pool2Units = units;
    }
    BBTRY(launch<256>(emit_kernel, 64 * n, stream, a, (const long long *)c->d_untrimOffsets, c->d_pool2));
    std::swap(c->d_pool, c->d_pool2); std::swap(c->poolUnits, c->pool2Units);
    c->poolUsed = total;
    return BBMAP_OK;
}

}  // namespace bbuntrim

extern "C" int bbmap_untrim_batch_device(bbmap_ctx *c, void *stream_, const bbidx_read *reads_untrimmed, const bbtrim_rec *trims) {
    if (!c || !reads_untrimmed || !trims) return bbfail(BBMAP_E_ARG, "bbmap_untrim_batch_device: null argument");
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_untrim_batch_device: the context runs without the final stage (bbmap_config.finalStage)");
    if (!c->ran) return bbfail(BBMAP_E_ARG, "bbmap_untrim_batch_device: no batch has been mapped yet");
    if (c->untrimmed) return bbfail(BBMAP_E_ARG, "bbmap_untrim_batch_device: the last batch has been untrimmed already");
    if (!c->batch.reads || !c->batch.bases || c->batch.n_reads != c->stats.reads)
        return bbfail(BBMAP_E_ARG, "bbmap_untrim_batch_device: the context does not hold the last batch's reads");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    const long long n = c->stats.reads;
    BBTRY(bbuntrim::untrim_ctx(c, stream, n, nullptr, trims));
    if (c->tier && c->tierReads > 0 && c->tier->ran) BBTRY(bbuntrim::untrim_ctx(c->tier, stream, c->tierReads, c->d_tierReadIds, trims));
    // the batch is the full reads from here on; their reverse complements replace the trimmed reads'
    c->batch.reads = reads_untrimmed;
    BBTRY(bbpipe_revcomp_device(stream, n, reads_untrimmed, c->batch.bases, c->batch.bases + c->batch.minus_delta));
    c->untrimmed = true;
    return BBMAP_OK;
}
