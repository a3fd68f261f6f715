// What reads a finished batch of the mapper (mapper_host.hip maps it): packed site lists, the host-buffer form of the batch call, the
// log and final records, scaffold records, SAM records, run statistics, coverage, read histograms, reference-set binning.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "coverage.h"
#include "mapper_ctx.h"
#include "read_hist.h"
#include "ref_split.h"
#include "run_stats.h"
#include "sam_records.h"
#include "scan_offsets.h"

using namespace bbmapper;

// The batch's site lists without the empty slots: counts[r] sites of read r (0 for a read without a list: no site, flagged, or
// mapped by the overflow tier) at packed[offsets[r] ...], offsets = exclusive prefix sums of counts (offsets[n] = their total).
extern "C" int bbmap_pack_sites_device(bbmap_ctx *c, void *stream_, int64_t n_reads, int32_t *counts, int64_t *offsets, bbmap_msite *packed,
                                       int64_t packed_cap) {
    if (!c || !counts || !offsets || !packed) return bbfail(BBMAP_E_ARG, "bbmap_pack_sites_device: null argument");
    if (!c->ran || n_reads != c->stats.reads) return bbfail(BBMAP_E_ARG, "bbmap_pack_sites_device: n_reads is not the last batch's");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    const long long n = n_reads;
    BBTRY(launch<256>(pack_counts_kernel, n, stream, c->d_mcount, n, counts));
    BBTRY(scan_offsets(counts, n, (long long *)offsets, c->buf[BUF_PACK_TMP], stream, nullptr));
    const long long threads = n * c->cfg.max_sites * 8;
    BBTRY(launch<256>(pack_sites_kernel, threads, stream, c->d_ms, c->d_mcount, (const long long *)offsets, n, c->cfg.max_sites, (long long)packed_cap, packed));
    return BBMAP_OK;
}

// Host-buffer form of the batch call, for a host that owns no device memory (the JNI glue, jni/hip_glue.c): uploads the batch,
// maps it, packs the site lists and copies them back.  Lists of reads the overflow tier mapped are appended behind the packed ones.
extern "C" int bbmap_map_batch(bbmap_ctx *c, int64_t n_reads, const bbidx_read *reads, const uint8_t *bases, int64_t bases_bytes,
                               const int8_t *baseScores, const int32_t *keyinfo, int64_t keyinfo_ints, int32_t *nsites_out,
                               int64_t *offsets_out, bbmap_msite *sites_out, int64_t sites_cap, int64_t *total_out) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_map_batch: null context");
    if (n_reads < 0 || n_reads > c->cfg.max_reads) return bbfail(BBMAP_E_ARG, "bbmap_map_batch: more reads than the context was made for");
    if (total_out) *total_out = 0;
    if (n_reads == 0) return BBMAP_OK;
    if (!reads || !bases || !baseScores || !keyinfo || !nsites_out || !offsets_out || (sites_cap > 0 && !sites_out) || sites_cap < 0 ||
        bases_bytes < 0 || keyinfo_ints < 0)
        return bbfail(BBMAP_E_ARG, "bbmap_map_batch: bad argument");
    for (int64_t r = 0; r < n_reads; r++) {
        const bbidx_read &rd = reads[r];
        if (rd.len < 0 || rd.bases_off < 0 || rd.bases_off + rd.len > bases_bytes)
            return bbfail(BBMAP_E_ARG, "bbmap_map_batch: a read lies outside the bases buffer");
        if (rd.nkeys < 0 || rd.keys_off < 0 || rd.keys_off + 2LL * rd.nkeys > keyinfo_ints)
            return bbfail(BBMAP_E_ARG, "bbmap_map_batch: a read's key offsets and scores lie outside keyinfo");
        // the probe kernels index the read with these offsets (LDS and global memory): every key inside its read, offsets ascending
        // (KeyRing.makeOffsets3 gives them so), no more keys than the profile's kernels take
        if (rd.nkeys > (c->cfg.reserved[3] == BBIDX_PROFILE_PACBIO ? BBIDX_PACBIO_MAX_KEYS : BBIDX_MAX_KEYS))
            return bbfail(BBMAP_E_ARG, "bbmap_map_batch: a read has more keys than the index profile allows (BBIDX_MAX_KEYS / BBIDX_PACBIO_MAX_KEYS)");
        const int kk = c->index->dev.p.k;
        for (int q = 0; q < rd.nkeys; q++) {
            const int o = keyinfo[rd.keys_off + q];
            if (o < 0 || o + kk > rd.len || (q > 0 && o < keyinfo[rd.keys_off + q - 1]))
                return bbfail(BBMAP_E_ARG, "bbmap_map_batch: a key offset lies outside its read, or the offsets are not ascending");
        }
    }
    BBHIP(hipSetDevice(c->cfg.device));
    const size_t nb = (size_t)bases_bytes;
    DevBuf *io = c->buf;
    auto room = [io](int i, size_t need) { return io[i].grow(need, need / 4 + 256); };      // (nothing is in flight on them between calls)
    BBHIP(room(HIO_READS, (size_t)n_reads * sizeof(bbidx_read)));
    BBHIP(room(HIO_BASES, 2 * nb + 16));
    BBHIP(room(HIO_SCORES, nb + 16));
    BBHIP(room(HIO_KEYINFO, (size_t)keyinfo_ints * 4 + 16));
    BBHIP(room(HIO_COUNTS, (size_t)(n_reads + 1) * 4));
    BBHIP(room(HIO_OFFSETS, (size_t)(n_reads + 1) * 8));
    BBHIP(room(HIO_PACKED, (size_t)(sites_cap > 0 ? sites_cap : 1) * sizeof(bbmap_msite)));
    // A stream of this context's own, non-blocking: several mapping threads, each with its own bbmap_ctx on one shared index (BBMap's
    // thread model), then overlap on the GPU instead of queueing behind one another on the legacy default stream.
    if (!c->hostStream) BBHIP(hipStreamCreateWithFlags(&c->hostStream, hipStreamNonBlocking));
    hipStream_t hs = c->hostStream;
    BBHIP(hipMemcpyAsync(io[HIO_READS].p, reads, (size_t)n_reads * sizeof(bbidx_read), hipMemcpyHostToDevice, hs));
    BBHIP(hipMemcpyAsync(io[HIO_BASES].p, bases, nb, hipMemcpyHostToDevice, hs));
    BBHIP(hipMemcpyAsync(io[HIO_SCORES].p, baseScores, nb, hipMemcpyHostToDevice, hs));
    BBHIP(hipMemcpyAsync(io[HIO_KEYINFO].p, keyinfo, (size_t)keyinfo_ints * 4, hipMemcpyHostToDevice, hs));
    BBTRY(bbmap_map_batch_device(c, hs, n_reads, (const bbidx_read *)io[HIO_READS].p, (uint8_t *)io[HIO_BASES].p, (int64_t)nb,
                                (const int8_t *)io[HIO_SCORES].p, (const int32_t *)io[HIO_KEYINFO].p));
    BBTRY(bbmap_pack_sites_device(c, hs, n_reads, (int32_t *)io[HIO_COUNTS].p, (int64_t *)io[HIO_OFFSETS].p, (bbmap_msite *)io[HIO_PACKED].p, sites_cap));
    BBHIP(hipMemcpyAsync(nsites_out, c->d_mcount, (size_t)n_reads * 4, hipMemcpyDeviceToHost, hs));      // counts, or the flags (-1, -2, -3)
    BBHIP(hipMemcpyAsync(offsets_out, io[HIO_OFFSETS].p, (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, hs));
    BBHIP(hipStreamSynchronize(hs));
    long long total = offsets_out[n_reads];
    const long long have = total < sites_cap ? total : sites_cap;
    if (have > 0) { BBHIP(hipMemcpyAsync(sites_out, io[HIO_PACKED].p, (size_t)have * sizeof(bbmap_msite), hipMemcpyDeviceToHost, hs)); BBHIP(hipStreamSynchronize(hs)); }
    bbmap_overflow_output ov;
    BBTRY(bbmap_get_overflow_output(c, &ov));
    if (ov.n_reads > 0) {
        std::vector<int32_t> ids((size_t)ov.n_reads), tn((size_t)ov.n_reads);
        BBHIP(hipMemcpy(ids.data(), ov.read_ids, (size_t)ov.n_reads * 4, hipMemcpyDeviceToHost));
        BBHIP(hipMemcpy(tn.data(), ov.out.nsites, (size_t)ov.n_reads * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < ov.n_reads; i++) {
            const int32_t r = ids[(size_t)i];
            if (r < 0 || r >= n_reads || nsites_out[r] != BBMAP_NSITES_IN_TIER) continue;
            nsites_out[r] = tn[(size_t)i];
            offsets_out[r] = total;
            if (tn[(size_t)i] <= 0) continue;
            if (total + tn[(size_t)i] <= sites_cap)
                BBHIP(hipMemcpy(sites_out + total, ov.out.sites + i * (int64_t)ov.out.cap, (size_t)tn[(size_t)i] * sizeof(bbmap_msite), hipMemcpyDeviceToHost));
            total += tn[(size_t)i];
        }
    }
    if (total_out) *total_out = total;
    return BBMAP_OK;
}

extern "C" int bbmap_get_overflow_output(bbmap_ctx *c, bbmap_overflow_output *o) {
    if (!c || !o) return bbfail(BBMAP_E_ARG, "bbmap_get_overflow_output: null argument");
    if (!c->ran) return bbfail(BBMAP_E_ARG, "bbmap_get_overflow_output: no batch has been mapped yet");
    memset(o, 0, sizeof *o);
    if (!c->tier || c->tierReads == 0 || !c->tier->ran) return BBMAP_OK;
    o->n_reads = c->tierReads; o->read_ids = c->d_tierReadIds;
    return bbmap_get_output(c->tier, &o->out);
}

extern "C" int bbmap_get_output(bbmap_ctx *c, bbmap_output *o) {
    if (!c || !o) return bbfail(BBMAP_E_ARG, "bbmap_get_output: null argument");
    if (!c->ran) return bbfail(BBMAP_E_ARG, "bbmap_get_output: no batch has been mapped yet");
    memset(o, 0, sizeof *o);
    o->sites = c->d_ms; o->nsites = c->d_mcount; o->cap = c->cfg.max_sites;
    o->match_stride = c->matchStride; o->gmatch_stride = c->gmatchStride;
    o->n_jobs = c->nJobs; o->n_gapped_jobs = c->nGapped;
    o->jobs = c->d_jobs; o->results = c->d_results; o->jobinfo = c->d_jinfo; o->match = c->d_match;
    o->gjobs = c->d_gjobs; o->gresults = c->d_gresults; o->gjobinfo = c->d_ginfo; o->gmatch = c->d_gmatch; o->ggaps = c->d_ggaps;
    if (c->S.finalStage) { o->final = c->d_final; o->final_match = c->d_pool; o->final_match_bytes = c->poolUsed; o->n_final_fills = c->finalFills; }
    return BBMAP_OK;
}

extern "C" int bbmap_set_average_pair_dist(bbmap_ctx *c, int32_t v) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_set_average_pair_dist: null context");
    if (v < 0) return bbfail(BBMAP_E_ARG, "bbmap_set_average_pair_dist: negative distance");
    c->S.averagePairDist = v; c->cfg.averagePairDist = v;
    if (c->tier) { c->tier->S.averagePairDist = v; c->tier->cfg.averagePairDist = v; }
    return BBMAP_OK;
}

// The last batch's final records on the host, overflow tier included; match strings packed in read order.
extern "C" int bbmap_get_final(bbmap_ctx *c, int64_t n_reads, bbmap_final *out, uint8_t *match_out, int64_t match_cap, int64_t *match_bytes) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_final: null argument");
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_get_final: the context runs without the final stage (bbmap_config.finalStage)");
    if (!c->ran || n_reads != c->stats.reads) return bbfail(BBMAP_E_ARG, "bbmap_get_final: n_reads is not the last batch's");
    if (match_cap < 0 || (match_cap > 0 && !match_out)) return bbfail(BBMAP_E_ARG, "bbmap_get_final: bad match buffer");
    BBHIP(hipSetDevice(c->cfg.device));
    BBHIP(hipMemcpy(out, c->d_final, (size_t)n_reads * sizeof(bbmap_final), hipMemcpyDeviceToHost));
    std::vector<uint8_t> pool, tpool;
    if (match_out) {
        pool.resize((size_t)c->poolUsed + 4);
        if (c->poolUsed > 0) BBHIP(hipMemcpy(pool.data(), c->d_pool, (size_t)c->poolUsed, hipMemcpyDeviceToHost));
    }
    std::vector<uint8_t> fromTier((size_t)n_reads, 0);
    if (c->tier && c->tierReads > 0 && c->tier->ran) {
        bbmap_ctx *t = c->tier;
        std::vector<int32_t> ids((size_t)c->tierReads);
        std::vector<bbmap_final> tf((size_t)c->tierReads);
        BBHIP(hipMemcpy(ids.data(), c->d_tierReadIds, (size_t)c->tierReads * 4, hipMemcpyDeviceToHost));
        BBHIP(hipMemcpy(tf.data(), t->d_final, (size_t)c->tierReads * sizeof(bbmap_final), hipMemcpyDeviceToHost));
        if (match_out) {
            tpool.resize((size_t)t->poolUsed + 4);
            if (t->poolUsed > 0) BBHIP(hipMemcpy(tpool.data(), t->d_pool, (size_t)t->poolUsed, hipMemcpyDeviceToHost));
        }
        for (long long i = 0; i < c->tierReads; i++) {
            const int32_t r = ids[(size_t)i];
            if (r < 0 || r >= n_reads || out[r].nsites != BBMAP_NSITES_IN_TIER) continue;
            out[r] = tf[(size_t)i]; fromTier[(size_t)r] = 1;
        }
    }
    int64_t used = 0;
    for (int64_t r = 0; r < n_reads; r++) {
        bbmap_final &f = out[r];
        if (f.match_len <= 0) { f.match_off = 0; continue; }
        if (match_out) {
            const std::vector<uint8_t> &src = fromTier[(size_t)r] ? tpool : pool;
            if (f.match_off < 0 || f.match_off + f.match_len > (int64_t)src.size()) return bbfail(BBMAP_E_HIP, "bbmap_get_final: a match string lies outside its pool (internal error)");
            if (used + f.match_len <= match_cap) memcpy(match_out + used, src.data() + f.match_off, (size_t)f.match_len);
        }
        f.match_off = used; used += f.match_len;
    }
    if (match_bytes) *match_bytes = used;
    return BBMAP_OK;
}

// The last batch as the stages' kernels see it (batch_view.h), on `stream`: the main context's arrays, and where the tier mapped reads
// its arrays and the map read -> tier record (-1 = not a tier read), which is filled here.
static int batch_view(bbmap_ctx *c, hipStream_t stream, BatchView *V) {
    *V = BatchView{};
    V->reads = c->batch.reads; V->bases = c->batch.bases; V->n = c->stats.reads; V->paired = c->cfg.paired;
    V->fin = c->d_final; V->pool = c->d_pool; V->sites = c->d_ms; V->nsites = c->d_mcount; V->cap = c->cfg.max_sites;
    const bbmap_ctx *t = c->tier;
    if (!(t && c->tierReads > 0 && t->ran && V->n > 0)) return BBMAP_OK;
    if (!c->d_scafTier) BBTRY(dalloc(c, &c->d_scafTier, (size_t)c->cfg.max_reads));
    BBHIP(hipMemsetAsync(c->d_scafTier, 0xff, (size_t)V->n * 4, stream));
    BBTRY(launch<256>(tier_index_kernel, c->tierReads, stream, c->d_tierReadIds, c->tierReads, V->n, c->d_scafTier));
    V->tfin = t->d_final; V->tpool = t->d_pool; V->tsites = t->d_ms; V->tnsites = t->d_mcount; V->tcap = t->cfg.max_sites;
    V->tierIdx = c->d_scafTier;
    return BBMAP_OK;
}

// bbmap_get_scaffold_records; *V is the view it made, for a caller that goes on with the same batch on the same stream
static int scaffold_records(bbmap_ctx *c, hipStream_t stream, BatchView *V, const bbmap_scafrec **out) {
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_get_scaffold_records: the context runs without the final stage (bbmap_config.finalStage)");
    if (!c->ran) return bbfail(BBMAP_E_ARG, "bbmap_get_scaffold_records: no batch has been mapped yet");
    const bbscaf::Table T = c->index->scaf;
    if (!T.off) return bbfail(BBMAP_E_ARG, "bbmap_get_scaffold_records: the index has no scaffold table (bbidx_set_scaffolds)");
    BBHIP(hipSetDevice(c->cfg.device));
    if (!c->d_scafRec) {
        BBTRY(dalloc(c, &c->d_scafRec, (size_t)c->cfg.max_reads));
    }
    BBTRY(batch_view(c, stream, V));
    const long long units = V->paired ? V->n / 2 : V->n;
    if (units > 0)          // one wavefront per unit
        BBTRY(launch<256>(scaffold_coords_kernel, 64 * units, stream, T, *V, c->d_scafRec));
    *out = c->d_scafRec;
    return BBMAP_OK;
}

extern "C" int bbmap_get_scaffold_records(bbmap_ctx *c, void *stream_, const bbmap_scafrec **out) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_scaffold_records: null argument");
    BatchView V;
    return scaffold_records(c, (hipStream_t)stream_, &V, out);
}

// ---- SAM records (sam_records.hip)
static const int SAM_ALL_FLAGS = BBMAP_SAM_CIGAR13 | BBMAP_SAM_MD;
static const int SAM_ALL_TAGS = BBMAP_SAM_MAKE_NM | BBMAP_SAM_MAKE_AM | BBMAP_SAM_MAKE_SM | BBMAP_SAM_MAKE_XM | BBMAP_SAM_MAKE_XS |
                                BBMAP_SAM_XS_SECONDSTRAND | BBMAP_SAM_MAKE_NH | BBMAP_SAM_MAKE_STOP | BBMAP_SAM_MAKE_LENGTH |
                                BBMAP_SAM_MAKE_IDENTITY | BBMAP_SAM_MAKE_SCORE | BBMAP_SAM_MAKE_INSERT | BBMAP_SAM_MAKE_BOUNDS | BBMAP_SAM_NO_TAGS;
static const int SAM_MAX_READ_LEN = 6016;                   // bbmap_config.max_read_len's limit

extern "C" int bbmap_sam_default_config(bbmap_sam_config *cfg) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "bbmap_sam_default_config: null argument");
    memset(cfg, 0, sizeof *cfg);
    cfg->intronLimit = INT32_MAX;                           // SamLine.INTRON_LIMIT = Integer.MAX_VALUE (SamLine.java:2424)
    cfg->tags = BBMAP_SAM_MAKE_NM | BBMAP_SAM_MAKE_AM;
    return BBMAP_OK;
}

static int check_sam_config(const char *fn, const bbmap_sam_config *cfg) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "%s: null argument", fn);
    if (cfg->flags & ~SAM_ALL_FLAGS) return bbfail(BBMAP_E_ARG, "%s: unknown flag bits", fn);
    if (cfg->tags & ~SAM_ALL_TAGS) return bbfail(BBMAP_E_ARG, "%s: unknown tag bits", fn);
    if (cfg->intronLimit < 0) return bbfail(BBMAP_E_ARG, "%s: negative intron limit", fn);
    return BBMAP_OK;
}

// SamLine's remaining fields for the last batch: the coordinate kernel, the sizing pass, a device-wide exclusive scan of the per-read
// byte counts, the emit pass.  The blob's size comes back once between the scan and the emit pass (it sizes the blob).
static int sam_records(bbmap_ctx *c, hipStream_t stream, const bbmap_sam_config &cfg, bool wantTags, const bbmap_samrec **recs,
                       const bbmap_samtags **tags, const uint8_t **text, int64_t *text_bytes) {
    bbsam::Args a = {};
    BBTRY(scaffold_records(c, stream, &a.V, &a.scaf));      // its error cases are this call's: no final stage, no batch, no scaffold table
    if (!c->batch.reads || !c->batch.bases || c->batch.n_reads != c->stats.reads)
        return bbfail(BBMAP_E_ARG, "bbmap_get_sam_records: the context does not hold the last batch's reads");
    const long long n = a.V.n;
    const int maxLen = c->cfg.max_read_len;
    if (!c->d_samRec) {
        BBTRY(dalloc(c, &c->d_samRec, (size_t)c->cfg.max_reads));
        BBTRY(dalloc(c, &c->d_samCounts, (size_t)c->cfg.max_reads + 1));
        BBTRY(dalloc(c, &c->d_samOffsets, (size_t)c->cfg.max_reads + 1));
        BBTRY(dalloc(c, &c->d_mapqMax, (size_t)maxLen + 1));
        std::vector<float> table((size_t)maxLen + 1);
        bbsam::fill_mapq_max(table.data(), maxLen);
        BBHIP(hipMemcpy(c->d_mapqMax, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (wantTags && !c->d_samTags) BBTRY(dalloc(c, &c->d_samTags, (size_t)c->cfg.max_reads));
    a.chromArr = c->d_chromArr; a.chromArrLen = c->d_chromArrLen;
    a.mapqMax = c->d_mapqMax; a.mapqMaxLen = maxLen;
    a.flags = cfg.flags; a.intronLimit = cfg.intronLimit; a.tags = cfg.tags;
    BBHIP(bbsam::launch_size(a, c->d_samRec, wantTags ? c->d_samTags : nullptr, c->d_samCounts, stream));
    long long total = 0;
    BBTRY(scan_offsets(c->d_samCounts, n, c->d_samOffsets, c->buf[BUF_SAM_TMP], stream, &total));
    BBHIP(c->buf[BUF_SAM_TEXT].grow((size_t)total, (size_t)total / 4 + 256));       // (the stream has just been waited for)
    uint8_t *blob = (uint8_t *)c->buf[BUF_SAM_TEXT].p;
    a.textCap = total;
    BBHIP(bbsam::launch_emit(a, c->d_samRec, c->d_samOffsets, blob, stream));
    c->samTextBytes = total;
    *recs = c->d_samRec; *text = blob;
    if (tags) *tags = wantTags ? c->d_samTags : nullptr;
    if (text_bytes) *text_bytes = total;
    return BBMAP_OK;
}

// (the default configuration of the call below)
extern "C" int bbmap_get_sam_records(bbmap_ctx *c, void *stream_, int32_t flags, const bbmap_samrec **recs, const uint8_t **text,
                                     int64_t *text_bytes) {
    if (!c || !recs || !text) return bbfail(BBMAP_E_ARG, "bbmap_get_sam_records: null argument");
    if (flags & ~SAM_ALL_FLAGS) return bbfail(BBMAP_E_ARG, "bbmap_get_sam_records: unknown flag bits");
    bbmap_sam_config cfg;
    bbmap_sam_default_config(&cfg);
    cfg.flags = flags;
    return sam_records(c, (hipStream_t)stream_, cfg, false, recs, nullptr, text, text_bytes);
}

extern "C" int bbmap_get_sam_records_cfg(bbmap_ctx *c, void *stream_, const bbmap_sam_config *cfg, const bbmap_samrec **recs,
                                         const bbmap_samtags **tags, const uint8_t **text, int64_t *text_bytes) {
    if (!c || !recs || !text) return bbfail(BBMAP_E_ARG, "bbmap_get_sam_records_cfg: null argument");
    BBTRY(check_sam_config("bbmap_get_sam_records_cfg", cfg));
    return sam_records(c, (hipStream_t)stream_, *cfg, tags != nullptr, recs, tags, text, text_bytes);
}

// Host forms: the records and the blob as they are on the device (packed in read order already), two or three copies.
extern "C" int bbmap_get_sam_cfg(bbmap_ctx *c, int64_t n_reads, const bbmap_sam_config *cfg, bbmap_samrec *out, bbmap_samtags *tags_out,
                                 uint8_t *text_out, int64_t text_cap, int64_t *text_bytes) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_sam_cfg: null argument");
    BBTRY(check_sam_config("bbmap_get_sam_cfg", cfg));
    if (!c->ran || n_reads != c->stats.reads) return bbfail(BBMAP_E_ARG, "bbmap_get_sam_cfg: n_reads is not the last batch's");
    if (text_cap < 0 || (text_cap > 0 && !text_out)) return bbfail(BBMAP_E_ARG, "bbmap_get_sam_cfg: bad text buffer");
    const bbmap_samrec *recs = nullptr; const bbmap_samtags *tags = nullptr; const uint8_t *text = nullptr; int64_t total = 0;
    BBTRY(sam_records(c, nullptr, *cfg, tags_out != nullptr, &recs, &tags, &text, &total));
    if (n_reads > 0) BBHIP(hipMemcpy(out, recs, (size_t)n_reads * sizeof(bbmap_samrec), hipMemcpyDeviceToHost));    // (waits for the null stream)
    if (n_reads > 0 && tags_out) BBHIP(hipMemcpy(tags_out, tags, (size_t)n_reads * sizeof(bbmap_samtags), hipMemcpyDeviceToHost));
    if (text_out && total > 0 && total <= text_cap) BBHIP(hipMemcpy(text_out, text, (size_t)total, hipMemcpyDeviceToHost));
    if (text_bytes) *text_bytes = total;
    return BBMAP_OK;
}

extern "C" int bbmap_get_sam(bbmap_ctx *c, int64_t n_reads, int32_t flags, bbmap_samrec *out, uint8_t *text_out, int64_t text_cap,
                             int64_t *text_bytes) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_sam: null argument");
    if (!c->ran || n_reads != c->stats.reads) return bbfail(BBMAP_E_ARG, "bbmap_get_sam: n_reads is not the last batch's");
    if (text_cap < 0 || (text_cap > 0 && !text_out)) return bbfail(BBMAP_E_ARG, "bbmap_get_sam: bad text buffer");
    const bbmap_samrec *recs = nullptr; const uint8_t *text = nullptr; int64_t total = 0;
    BBTRY(bbmap_get_sam_records(c, nullptr, flags, &recs, &text, &total));
    if (n_reads > 0) BBHIP(hipMemcpy(out, recs, (size_t)n_reads * sizeof(bbmap_samrec), hipMemcpyDeviceToHost));    // (waits for the null stream)
    if (text_out && total > 0 && total <= text_cap) BBHIP(hipMemcpy(text_out, text, (size_t)total, hipMemcpyDeviceToHost));
    if (text_bytes) *text_bytes = total;
    return BBMAP_OK;
}

// The raw form over arrays the caller owns (include/bbmap_amd.h).  Workspace: the MAPQ table, the per-read byte counts, their prefix
// sums, the scan's scratch, each at a multiple of 256 bytes.
static size_t sam_align(size_t b) { return (b + 255) & ~(size_t)255; }
static const std::vector<float> &sam_mapq_table() {          // (a static: the asynchronous upload reads it after the call has returned)
    static const std::vector<float> table = [] {
        std::vector<float> t((size_t)SAM_MAX_READ_LEN + 1);
        bbsam::fill_mapq_max(t.data(), SAM_MAX_READ_LEN);
        return t;
    }();
    return table;
}
static long long sam_workspace_bytes(long long n, int maxLen, size_t *scanBytes) {
    if (scan_scratch_bytes(n, scanBytes) != hipSuccess) return -1;
    return (long long)(sam_align(((size_t)maxLen + 1) * 4) + sam_align(((size_t)n + 1) * 4) + sam_align(((size_t)n + 1) * 8) + sam_align(*scanBytes) + 256);
}

extern "C" int64_t bbpipe_sam_records_workspace_bytes(int64_t n_reads, int32_t max_read_len) {
    if (n_reads < 0 || n_reads >= (1ll << 31) - 1 || max_read_len < 1 || max_read_len > SAM_MAX_READ_LEN)
        return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_workspace_bytes: bad argument");
    size_t scanBytes = 0;
    const long long b = sam_workspace_bytes(n_reads, max_read_len, &scanBytes);
    if (b < 0) return bbfail(BBMAP_E_HIP, "bbpipe_sam_records_workspace_bytes: the scan could not be sized");
    return b;
}

extern "C" int bbpipe_sam_records_device(void *stream_, int64_t n_reads, int32_t paired, const bbmap_sam_config *cfg, int32_t max_read_len,
                                         const bbidx_read *reads, const uint8_t *bases, const bbmap_final *finals, const uint8_t *pool,
                                         const bbmap_scafrec *scaf, const bbmap_msite *sites, const int32_t *nsites, int32_t cap,
                                         const uint8_t *const *chrom_arr, const int32_t *chrom_arr_len, bbmap_samrec *recs, bbmap_samtags *tags,
                                         uint8_t *text, int64_t text_cap, int64_t *text_bytes_dev, void *workspace, int64_t workspace_bytes) {
    if (n_reads < 0 || n_reads >= (1ll << 31) - 1 || (paired && (n_reads & 1)) || max_read_len < 1 || max_read_len > SAM_MAX_READ_LEN ||
        text_cap < 0 || cap < 0 || cap > BBMAP_MAX_SITES_LIMIT)
        return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_device: bad argument");
    BBTRY(check_sam_config("bbpipe_sam_records_device", cfg));
    if (!text_bytes_dev || (text_cap > 0 && !text)) return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_device: null buffer");
    hipStream_t stream = (hipStream_t)stream_;
    if (n_reads == 0) { BBHIP(hipMemsetAsync(text_bytes_dev, 0, 8, stream)); return BBMAP_OK; }
    if (!reads || !bases || !finals || !pool || !scaf || !recs) return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_device: null buffer");
    const bool tagged = !(cfg->tags & BBMAP_SAM_NO_TAGS);
    if (tagged && tags && (cfg->tags & BBMAP_SAM_MAKE_XM) && (!sites || !nsites || cap < 1))
        return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_device: BBMAP_SAM_MAKE_XM needs the site lists");
    if (tagged && (cfg->flags & BBMAP_SAM_MD) && (!chrom_arr || !chrom_arr_len))
        return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_device: BBMAP_SAM_MD needs the chromosome arrays");
    size_t scanBytes = 0;
    const long long need = sam_workspace_bytes(n_reads, max_read_len, &scanBytes);
    if (need < 0) return bbfail(BBMAP_E_HIP, "bbpipe_sam_records_device: the scan could not be sized");
    if (!workspace || workspace_bytes < need)
        return bbfail(BBMAP_E_ARG, "bbpipe_sam_records_device: the workspace is too small (bbpipe_sam_records_workspace_bytes)");
    uint8_t *ws = (uint8_t *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float *mapqMax = (float *)ws; ws += sam_align(((size_t)max_read_len + 1) * 4);
    int *counts = (int *)ws; ws += sam_align(((size_t)n_reads + 1) * 4);
    long long *offsets = (long long *)ws; ws += sam_align(((size_t)n_reads + 1) * 8);
    BBHIP(hipMemcpyAsync(mapqMax, sam_mapq_table().data(), ((size_t)max_read_len + 1) * 4, hipMemcpyHostToDevice, stream));
    bbsam::Args a = {};
    a.V.reads = reads; a.V.bases = bases; a.V.n = n_reads; a.V.paired = paired ? 1 : 0;
    a.V.fin = finals; a.V.pool = pool; a.V.sites = sites; a.V.nsites = nsites; a.V.cap = cap;      // (no tier)
    a.scaf = scaf; a.chromArr = chrom_arr; a.chromArrLen = chrom_arr_len;
    a.mapqMax = mapqMax; a.mapqMaxLen = max_read_len;
    a.flags = cfg->flags; a.intronLimit = cfg->intronLimit; a.tags = cfg->tags; a.textCap = text_cap;
    BBHIP(bbsam::launch_size(a, recs, tags, counts, stream));
    BBHIP(scan_offsets_scratch(counts, n_reads, offsets, ws, scanBytes, stream));
    BBHIP(bbsam::launch_emit(a, recs, offsets, text, stream));
    BBHIP(hipMemcpyAsync(text_bytes_dev, offsets + n_reads, 8, hipMemcpyDeviceToDevice, stream));
    return BBMAP_OK;
}

// ---- the accumulating stages (Accum, mapper_ctx.h): what their add, get, reset and enable calls share
enum { NEEDS_FINAL = 1, NEEDS_TRIMMED = 2, NEEDS_BASES = 4, SAYS_ADDED = 8 };

static bool table_replaced(const bbmap_ctx *c, long long gen) { return gen != c->index->scafGen || !c->index->scaf.off; }

// Whether `fn` may add the last batch to stage `st`: the refusals of every add call, in the order they have always been tested.
// off: what to say when the stage is not enabled (null: it is).  needs: what the stage reads (NEEDS_*).  gen: the scaffold table's
// generation when the stage was enabled (null: the stage reads no table); `since` names the stage in that refusal.
static int may_add(bbmap_ctx *c, int st, const char *fn, const char *off, int needs, const long long *gen = nullptr, const char *since = nullptr) {
    if (off) return bbfail(BBMAP_E_ARG, "%s: %s", fn, off);
    if ((needs & NEEDS_FINAL) && !c->S.finalStage) return bbfail(BBMAP_E_ARG, "%s: the context runs without the final stage (bbmap_config.finalStage)", fn);
    if (!c->ran) return bbfail(BBMAP_E_ARG, "%s: no batch has been mapped yet", fn);
    if (c->accum[st].counted) return bbfail(BBMAP_E_ARG, "%s: the last batch has been %s already", fn, needs & SAYS_ADDED ? "added" : "counted");
    if ((needs & NEEDS_TRIMMED) && c->untrimmed)
        return bbfail(BBMAP_E_ARG, "%s: the last batch has been untrimmed already (call it before bbmap_untrim_batch_device)", fn);
    if (!c->batch.reads || ((needs & NEEDS_BASES) && !c->batch.bases) || c->batch.n_reads != c->stats.reads)
        return bbfail(BBMAP_E_ARG, "%s: the context does not hold the last batch's reads", fn);
    if (gen && table_replaced(c, *gen)) return bbfail(BBMAP_E_ARG, "%s: the scaffold table has been replaced since %s enabled", fn, since);
    return BBMAP_OK;
}

// `bytes` of a stage's state to the host, behind the work that last wrote it
static int copy_out(bbmap_ctx *c, int st, void *dst, const void *src, size_t bytes) {
    BBHIP(hipStreamSynchronize(c->accum[st].stream));       // the state is written on that stream only
    BBHIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return BBMAP_OK;
}

// Zeroes a stage's state behind its last add and waits.  forget: the state no longer holds the batch the context still has, so that
// batch may be added again.
struct Span { void *p; size_t bytes; };
static int reset_state(bbmap_ctx *c, int st, std::initializer_list<Span> spans, bool forget = true) {
    Accum &a = c->accum[st];
    BBHIP(hipSetDevice(c->cfg.device));
    for (const Span &s : spans)
        if (s.bytes) BBHIP(hipMemsetAsync(s.p, 0, s.bytes, a.stream));
    BBHIP(hipStreamSynchronize(a.stream));
    if (forget) a.counted = false;
    return BBMAP_OK;
}

// The index's scaffold table as a stage that is sized by it keeps it: the number of scaffolds, the table's generation, and (hostLen
// not null) the scaffolds' lengths on the host.
static int scaf_snapshot(bbmap_ctx *c, int *nscaf, long long *gen, std::vector<int> *hostLen) {
    const bbscaf::Table T = c->index->scaf;
    std::vector<int> off((size_t)T.nchroms + 2);
    BBHIP(hipMemcpy(off.data(), T.off, off.size() * 4, hipMemcpyDeviceToHost));
    *nscaf = off[(size_t)T.nchroms + 1]; *gen = c->index->scafGen;
    if (!hostLen) return BBMAP_OK;
    hostLen->resize((size_t)*nscaf);
    BBHIP(hipMemcpy(hostLen->data(), T.len, (size_t)*nscaf * 4, hipMemcpyDeviceToHost));
    return BBMAP_OK;
}

// ---- run statistics (run_stats.hip) and the adaptive state they drive
static int run_stats_buffers(bbmap_ctx *c) {
    if (c->d_runStats) return BBMAP_OK;
    BBTRY(dalloc(c, &c->d_insertHist, (size_t)BBMAP_INSERT_HIST_BINS));
    BBHIP(hipMemset(c->d_insertHist, 0, 8 * (size_t)BBMAP_INSERT_HIST_BINS));
    unsigned long long *p = nullptr;
    BBTRY(dalloc(c, &p, (size_t)bbrunstats::N_COUNTERS));
    BBHIP(hipMemset(p, 0, sizeof(bbmap_runstats)));
    c->d_runStats = p;
    return BBMAP_OK;
}

extern "C" int bbmap_add_run_stats(bbmap_ctx *c, void *stream_, const bbmap_truth *truth) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_add_run_stats: null context");
    // (NEEDS_TRIMMED: calcStatistics runs inside processRead, on the trimmed read; AbstractMapThread.java:518-521 come after it)
    BBTRY(may_add(c, ACC_STATS, "bbmap_add_run_stats", nullptr, NEEDS_FINAL | NEEDS_TRIMMED));
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    BBTRY(run_stats_buffers(c));
    bbrunstats::Args a = {};
    BBTRY(batch_view(c, stream, &a.V));
    a.truth = truth;
    a.ptsMatch = c->S.ptsMatch; a.ptsMatch2 = c->S.ptsMatch2;
    a.thresh = 0; a.maxPairDist = c->cfg.maxPairDist;
    BBHIP(bbrunstats::launch(a, c->d_runStats, c->d_insertHist, stream));
    c->accum[ACC_STATS] = {true, stream};
    return BBMAP_OK;
}

extern "C" int bbmap_get_run_stats(bbmap_ctx *c, bbmap_runstats *out, int64_t *ihist_out) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_run_stats: null argument");
    BBHIP(hipSetDevice(c->cfg.device));
    if (!c->d_runStats) {
        memset(out, 0, sizeof *out);
        if (ihist_out) memset(ihist_out, 0, 8 * (size_t)BBMAP_INSERT_HIST_BINS);
        return BBMAP_OK;
    }
    BBTRY(copy_out(c, ACC_STATS, out, c->d_runStats, sizeof *out));
    if (ihist_out) BBTRY(copy_out(c, ACC_STATS, ihist_out, c->d_insertHist, 8 * (size_t)BBMAP_INSERT_HIST_BINS));
    return BBMAP_OK;
}

extern "C" int bbmap_reset_run_stats(bbmap_ctx *c) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_reset_run_stats: null context");
    c->numMatedSeen = 0;
    if (!c->d_runStats) return BBMAP_OK;
    // (the one reset that does not forget the batch: a second add of it stays refused)
    return reset_state(c, ACC_STATS, {{c->d_runStats, sizeof(bbmap_runstats)}, {c->d_insertHist, 8 * (size_t)BBMAP_INSERT_HIST_BINS}}, false);
}

extern "C" int bbmap_set_adaptive(bbmap_ctx *c, int32_t flags) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_set_adaptive: null context");
    if (flags & ~(BBMAP_ADAPT_INSERT_LENGTH | BBMAP_ADAPT_RESCUE_SKIP)) return bbfail(BBMAP_E_ARG, "bbmap_set_adaptive: unknown flag bits");
    if (flags && !c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_set_adaptive: the context runs without the final stage (bbmap_config.finalStage)");
    c->adaptive = flags;
    return BBMAP_OK;
}

extern "C" int bbmap_set_truth(bbmap_ctx *c, const bbmap_truth *truth) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_set_truth: null context");
    c->truthNext = truth;
    return BBMAP_OK;
}

// ---- coverage (coverage.hip): thin wrappers over the raw calls' launches
static const int COV_FLAGS = BBMAP_COV_START_ONLY | BBMAP_COV_EXCLUDE_DELETIONS | BBMAP_COV_STRANDED | BBMAP_COV_32BIT;

extern "C" int bbmap_cov_enable(bbmap_ctx *c, int32_t flags) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: null context");
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: the context runs without the final stage (bbmap_config.finalStage)");
    const bbscaf::Table T = c->index->scaf;
    if (!T.off) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: the index has no scaffold table (bbidx_set_scaffolds)");
    if (flags & ~COV_FLAGS) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: unknown flag bits");
    if (c->cov) {
        if (c->cov->flags != flags) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: coverage is enabled already with other flags");
        if (table_replaced(c, c->cov->gen)) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: the scaffold table has been replaced since coverage was enabled");
        return BBMAP_OK;
    }
    BBHIP(hipSetDevice(c->cfg.device));
    std::unique_ptr<CovState> v(new CovState);
    v->flags = flags;
    BBTRY(scaf_snapshot(c, &v->nscaf, &v->gen, &v->hostLen));
    const size_t ns = (size_t)v->nscaf;
    std::vector<int64_t> covoff(ns + 1);
    BBTRY(bbpipe_coverage_layout(v->nscaf, v->hostLen.data(), 0, covoff.data(), nullptr));
    v->slots = covoff[ns];
    if (v->slots > (1ll << 32)) return bbfail(BBMAP_E_ARG, "bbmap_cov_enable: more than 2^32 reference bases");
    const int strands = flags & BBMAP_COV_STRANDED ? 2 : 1;
    const size_t slots = (size_t)v->slots, hb = (size_t)bbcov::hist_bins(flags);
    if (v->covoff.grow((ns + 1) * 8) != hipSuccess || v->binoff.grow((ns + 1) * 8) != hipSuccess || v->recs.grow(ns * sizeof(bbmap_covrec)) != hipSuccess ||
        v->refgc.grow(ns * 32) != hipSuccess || v->totals.grow(sizeof(bbmap_covtotals)) != hipSuccess ||
        v->ws.grow((size_t)bbcov::workspace_bytes(v->nscaf, v->slots)) != hipSuccess)
        return bbfail(BBMAP_E_NOMEM, "bbmap_cov_enable: device allocation failed");
    for (int t = 0; t < strands; t++)
        if (v->diff[t].grow(slots * 4) != hipSuccess || v->depth[t].grow(slots * (flags & BBMAP_COV_32BIT ? 4 : 2)) != hipSuccess ||
            v->hist[t].grow(hb * 8) != hipSuccess)
            return bbfail(BBMAP_E_NOMEM, "bbmap_cov_enable: device allocation failed (4 + 2 or 4 bytes per reference base and strand)");
    BBHIP(hipMemcpy(v->covoff.p, covoff.data(), (ns + 1) * 8, hipMemcpyHostToDevice));
    for (int t = 0; t < strands; t++) BBHIP(hipMemset(v->diff[t].p, 0, slots * 4));
    BBHIP(hipMemset(v->recs.p, 0, ns * sizeof(bbmap_covrec)));
    BBHIP(hipMemset(v->totals.p, 0, sizeof(bbmap_covtotals)));
    BBHIP(bbcov::launch_refgc(T, v->nscaf, c->d_chromArr, v->refgc.as<long long>(), nullptr));      // once per enable, not per finalize
    BBHIP(hipStreamSynchronize(nullptr));
    c->cov = v.release();
    return BBMAP_OK;
}

extern "C" int bbmap_add_coverage(bbmap_ctx *c, void *stream_) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_add_coverage: null context");
    CovState *v = c->cov;
    BBTRY(may_add(c, ACC_COV, "bbmap_add_coverage", v ? nullptr : "coverage is not enabled (bbmap_cov_enable)", NEEDS_BASES, v ? &v->gen : nullptr,
                  "coverage was"));
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    bbcov::AddArgs a = {};
    BBTRY(batch_view(c, stream, &a.V));
    a.flags = v->flags;
    a.T = c->index->scaf; a.nscaf = v->nscaf; a.covoff = v->covoff.as<long long>();
    a.diff[0] = v->diff[0].as<int>(); a.diff[1] = v->diff[1].as<int>();
    a.recs = v->recs.as<unsigned long long>(); a.totals = v->totals.as<unsigned long long>();
    BBHIP(bbcov::launch_add(a, stream));
    c->accum[ACC_COV] = {true, stream};
    return BBMAP_OK;
}

extern "C" int bbmap_cov_finalize(bbmap_ctx *c, void *stream_, int32_t binsize, bbmap_cov_view *out) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_cov_finalize: null argument");
    if (!c->cov) return bbfail(BBMAP_E_ARG, "bbmap_cov_finalize: coverage is not enabled (bbmap_cov_enable)");
    if (binsize < 0) return bbfail(BBMAP_E_ARG, "bbmap_cov_finalize: binsize must be >= 0");
    CovState *v = c->cov;
    if (table_replaced(c, v->gen)) return bbfail(BBMAP_E_ARG, "bbmap_cov_finalize: the scaffold table has been replaced since coverage was enabled");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    const int strands = v->flags & BBMAP_COV_STRANDED ? 2 : 1;
    const size_t ns = (size_t)v->nscaf;
    Accum &acc = c->accum[ACC_COV];
    if (stream != acc.stream) BBHIP(hipStreamSynchronize(acc.stream));     // behind everything added so far
    if (binsize != v->binsize) {
        std::vector<int64_t> binoff(ns + 1, 0);
        BBTRY(bbpipe_coverage_layout(v->nscaf, v->hostLen.data(), binsize, nullptr, binoff.data()));
        BBHIP(hipStreamSynchronize(stream));                               // an earlier finalize may still read the old offsets
        for (int t = 0; t < strands; t++) BBHIP(v->bins[t].grow((size_t)binoff[ns] * 8));
        BBHIP(hipMemcpy(v->binoff.p, binoff.data(), (ns + 1) * 8, hipMemcpyHostToDevice));
        v->binsize = binsize; v->nbins = binoff[ns];
    }
    bbcov::FinArgs a = {};
    a.flags = v->flags; a.nscaf = v->nscaf; a.slots = v->slots; a.len = c->index->scaf.len; a.covoff = v->covoff.as<long long>();
    for (int t = 0; t < strands; t++) {
        a.diff[t] = v->diff[t].as<int>(); a.depth[t] = v->depth[t].p;
        a.hist[t] = v->hist[t].as<unsigned long long>(); a.bins[t] = v->bins[t].as<unsigned long long>();
    }
    a.recs = v->recs.as<unsigned long long>(); a.refgc = v->refgc.as<long long>();
    a.binsize = binsize; a.binoff = v->binoff.as<long long>(); a.nbins = v->nbins;
    a.totals = v->totals.as<unsigned long long>(); a.ws = v->ws.p;
    BBHIP(bbcov::launch_finalize(a, stream));
    acc.stream = stream;
    memset(out, 0, sizeof *out);
    out->flags = v->flags; out->nscaf = v->nscaf; out->binsize = binsize; out->depth_bytes = v->flags & BBMAP_COV_32BIT ? 4 : 2;
    out->slots = v->slots; out->hist_bins = bbcov::hist_bins(v->flags); out->nbins = v->nbins;
    out->covoff = v->covoff.as<int64_t>(); out->recs = v->recs.as<bbmap_covrec>();
    out->binoff = v->binoff.as<int64_t>(); out->totals = v->totals.as<bbmap_covtotals>();
    for (int t = 0; t < strands; t++) { out->depth[t] = v->depth[t].p; out->hist[t] = v->hist[t].as<int64_t>(); out->bins[t] = v->bins[t].as<int64_t>(); }
    return BBMAP_OK;
}

extern "C" int bbmap_get_coverage(bbmap_ctx *c, int32_t binsize, bbmap_covrec *recs_out, int64_t nscaf_cap, bbmap_covtotals *totals_out,
                                  int64_t *hist_out, int64_t hist_cap, void *depth_out, int64_t depth_cap, int64_t *bins_out, int64_t bins_cap,
                                  bbmap_cov_view *view_out) {
    if (!c || !recs_out || !totals_out) return bbfail(BBMAP_E_ARG, "bbmap_get_coverage: null argument");
    if (nscaf_cap < 0 || hist_cap < 0 || depth_cap < 0 || bins_cap < 0 || (hist_cap > 0 && !hist_out) || (depth_cap > 0 && !depth_out) ||
        (bins_cap > 0 && !bins_out))
        return bbfail(BBMAP_E_ARG, "bbmap_get_coverage: bad buffer");
    if (c->cov && nscaf_cap < c->cov->nscaf) return bbfail(BBMAP_E_ARG, "bbmap_get_coverage: recs_out holds fewer records than the table has scaffolds");
    bbmap_cov_view w;
    BBTRY(bbmap_cov_finalize(c, nullptr, binsize, &w));
    BBHIP(hipStreamSynchronize(nullptr));
    if (view_out) *view_out = w;
    const int strands = w.flags & BBMAP_COV_STRANDED ? 2 : 1;
    BBHIP(hipMemcpy(recs_out, w.recs, (size_t)w.nscaf * sizeof(bbmap_covrec), hipMemcpyDeviceToHost));
    BBHIP(hipMemcpy(totals_out, w.totals, sizeof(bbmap_covtotals), hipMemcpyDeviceToHost));
    const size_t db = (size_t)w.slots * (size_t)w.depth_bytes;
    for (int t = 0; t < strands; t++) {
        if (hist_cap >= w.hist_bins) BBHIP(hipMemcpy(hist_out + (size_t)t * (size_t)hist_cap, w.hist[t], (size_t)w.hist_bins * 8, hipMemcpyDeviceToHost));
        if ((size_t)depth_cap >= db && db > 0) BBHIP(hipMemcpy((char *)depth_out + (size_t)t * (size_t)depth_cap, w.depth[t], db, hipMemcpyDeviceToHost));
        if (w.nbins > 0 && bins_cap >= w.nbins) BBHIP(hipMemcpy(bins_out + (size_t)t * (size_t)bins_cap, w.bins[t], (size_t)w.nbins * 8, hipMemcpyDeviceToHost));
    }
    return BBMAP_OK;
}

extern "C" int bbmap_reset_coverage(bbmap_ctx *c) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_reset_coverage: null context");
    CovState *v = c->cov;
    if (!v) return BBMAP_OK;
    const size_t diff = (size_t)v->slots * 4;                  // (an unstranded state has no second array: an empty span)
    return reset_state(c, ACC_COV, {{v->diff[0].p, diff}, {v->diff[1].p, v->flags & BBMAP_COV_STRANDED ? diff : 0},
                                    {v->recs.p, (size_t)v->nscaf * sizeof(bbmap_covrec)}, {v->totals.p, sizeof(bbmap_covtotals)}});
}

// ---- read histograms (read_hist.hip): thin wrappers over the raw calls' launch
extern "C" int bbmap_hist_enable(bbmap_ctx *c, int32_t flags) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_hist_enable: null context");
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_hist_enable: the context runs without the final stage (bbmap_config.finalStage)");
    if (flags & ~BBMAP_RH_ALL) return bbfail(BBMAP_E_ARG, "bbmap_hist_enable: unknown flag bits");
    if (!flags) return bbfail(BBMAP_E_ARG, "bbmap_hist_enable: no histogram group selected");
    if (c->d_readHist) {
        if (c->rhFlags != flags) return bbfail(BBMAP_E_ARG, "bbmap_hist_enable: the histograms are enabled already with other flags");
        return BBMAP_OK;
    }
    BBHIP(hipSetDevice(c->cfg.device));
    const size_t words = (size_t)bbrh::layout_of(flags).words;
    unsigned long long *p = nullptr;
    BBTRY(dalloc(c, &p, words));
    BBHIP(hipMemset(p, 0, 8 * words));
    BBHIP(hipStreamSynchronize(nullptr));                   // a first add on a non-blocking stream finds the state zeroed
    c->d_readHist = p; c->rhFlags = flags;
    return BBMAP_OK;
}

extern "C" int bbmap_add_read_hist(bbmap_ctx *c, void *stream_, const uint8_t *quality) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_add_read_hist: null context");
    BBTRY(may_add(c, ACC_HIST, "bbmap_add_read_hist", c->d_readHist ? nullptr : "the histograms are not enabled (bbmap_hist_enable)", NEEDS_BASES));
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    bbrh::Args a = {};
    BBTRY(batch_view(c, stream, &a.V));
    a.qual = quality; a.flags = c->rhFlags;
    a.state = c->d_readHist;
    BBHIP(bbrh::launch_add(a, stream));
    c->accum[ACC_HIST] = {true, stream};
    return BBMAP_OK;
}

extern "C" int bbmap_get_read_hist_view(bbmap_ctx *c, bbmap_readhist_view *out) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_read_hist_view: null argument");
    if (!c->d_readHist) return bbfail(BBMAP_E_ARG, "bbmap_get_read_hist_view: the histograms are not enabled (bbmap_hist_enable)");
    return bbpipe_read_hist_view(c->rhFlags, c->d_readHist, out);
}

extern "C" int bbmap_get_read_hist(bbmap_ctx *c, int64_t *out, int64_t cap_words, bbmap_readhist_view *view_out) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_get_read_hist: null context");
    if (!c->d_readHist) return bbfail(BBMAP_E_ARG, "bbmap_get_read_hist: the histograms are not enabled (bbmap_hist_enable)");
    if (cap_words < 0 || (cap_words > 0 && !out)) return bbfail(BBMAP_E_ARG, "bbmap_get_read_hist: bad buffer");
    bbmap_readhist_view w;
    BBTRY(bbpipe_read_hist_view(c->rhFlags, c->d_readHist, &w));
    if (view_out) *view_out = w;
    if (cap_words < w.words) return BBMAP_OK;
    BBHIP(hipSetDevice(c->cfg.device));
    return copy_out(c, ACC_HIST, out, c->d_readHist, 8 * (size_t)w.words);
}

extern "C" int bbmap_reset_read_hist(bbmap_ctx *c) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_reset_read_hist: null context");
    if (!c->d_readHist) return BBMAP_OK;
    return reset_state(c, ACC_HIST, {{c->d_readHist, 8 * (size_t)bbrh::layout_of(c->rhFlags).words}});
}

// ---- reference-set binning (ref_split.hip): thin wrappers over the raw calls' launches
extern "C" int bbmap_split_enable(bbmap_ctx *c, const bbmap_split_config *cfg_, const uint64_t *scaf_sets, const int32_t *scaf_key) {
    if (!c || !cfg_ || !scaf_sets || !scaf_key) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: null argument");
    if (!c->S.finalStage) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: the context runs without the final stage (bbmap_config.finalStage)");
    const bbscaf::Table T = c->index->scaf;
    if (!T.off) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: the index has no scaffold table (bbidx_set_scaffolds)");
    bbmap_split_config cfg = *cfg_;
    if (cfg.clearzone == 0) cfg.clearzone = c->S.cz1;                                          // CLEARZONE1()
    if (cfg.maxSites == 0) cfg.maxSites = c->cfg.reserved[3] == BBIDX_PROFILE_PACBIO ? 100 : 5;     // BBMapPacBio.java:65 / BBMap.java:62
    cfg.reserved[0] = cfg.reserved[1] = 0;
    if (const char *why = bbsplit::check_config(cfg)) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: %s", why);
    if (!cfg.flags) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: nothing selected");
    if (c->split) {
        if (memcmp(&c->split->cfg, &cfg, sizeof cfg) != 0) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: the stage is enabled already with another configuration");
        if (table_replaced(c, c->split->gen)) return bbfail(BBMAP_E_ARG, "bbmap_split_enable: the scaffold table has been replaced since the stage was enabled");
        return BBMAP_OK;
    }
    BBHIP(hipSetDevice(c->cfg.device));
    std::unique_ptr<SplitState> v(new SplitState);
    v->cfg = cfg;
    BBTRY(scaf_snapshot(c, &v->nscaf, &v->gen, nullptr));
    const size_t ns = (size_t)v->nscaf, sb = (size_t)bbpipe_refsplit_state_bytes(cfg.nkeys, cfg.nsets);
    if (v->sets.grow(ns * 8 + 8) != hipSuccess || v->keys.grow(ns * 4 + 4) != hipSuccess || v->state.grow(sb) != hipSuccess ||
        v->setoff.grow(8 * (2 * (size_t)cfg.nsets + 1)) != hipSuccess)
        return bbfail(BBMAP_E_NOMEM, "bbmap_split_enable: device allocation failed");
    if (cfg.flags & (BBMAP_SPLIT_RECORDS | BBMAP_SPLIT_LISTS))
        if (v->recs.grow((size_t)(c->cfg.max_reads > 0 ? c->cfg.max_reads : 1) * sizeof(bbmap_splitrec)) != hipSuccess)
            return bbfail(BBMAP_E_NOMEM, "bbmap_split_enable: device allocation failed");
    BBHIP(hipMemcpy(v->sets.p, scaf_sets, ns * 8, hipMemcpyHostToDevice));
    BBHIP(hipMemcpy(v->keys.p, scaf_key, ns * 4, hipMemcpyHostToDevice));
    BBHIP(hipMemset(v->state.p, 0, sb));
    BBHIP(hipStreamSynchronize(nullptr));                   // a first add on a non-blocking stream finds the state zeroed
    c->split = v.release();
    return BBMAP_OK;
}

extern "C" int bbmap_add_split(bbmap_ctx *c, void *stream_) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_add_split: null context");
    SplitState *v = c->split;
    BBTRY(may_add(c, ACC_SPLIT, "bbmap_add_split", v ? nullptr : "the stage is not enabled (bbmap_split_enable)", SAYS_ADDED, v ? &v->gen : nullptr,
                  "the stage was"));
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    bbsplit::Args a = {};
    BBTRY(batch_view(c, stream, &a.V));
    a.T = c->index->scaf; a.scafSets = v->sets.as<unsigned long long>(); a.scafKey = v->keys.as<int>();
    a.flags = v->cfg.flags; a.mode = v->cfg.ambiguous2; a.clearzone = v->cfg.clearzone; a.maxSites = v->cfg.maxSites;
    a.nsets = v->cfg.nsets; a.nkeys = v->cfg.nkeys;
    a.state = v->state.as<unsigned long long>(); a.recs = v->recs.as<bbmap_splitrec>();
    BBHIP(bbsplit::launch_assign(a, stream));
    c->accum[ACC_SPLIT] = {true, stream};
    v->added = a.V.n; v->total = -1;
    return BBMAP_OK;
}

extern "C" int bbmap_get_split_records(bbmap_ctx *c, const bbmap_splitrec **out) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_split_records: null argument");
    SplitState *v = c->split;
    if (!v) return bbfail(BBMAP_E_ARG, "bbmap_get_split_records: the stage is not enabled (bbmap_split_enable)");
    if (!v->recs.p) return bbfail(BBMAP_E_ARG, "bbmap_get_split_records: the stage keeps no records (BBMAP_SPLIT_RECORDS)");
    if (v->added < 0) return bbfail(BBMAP_E_ARG, "bbmap_get_split_records: no batch has been added yet");
    *out = v->recs.as<bbmap_splitrec>();
    return BBMAP_OK;
}

extern "C" int bbmap_get_split_lists_device(bbmap_ctx *c, void *stream_, const int64_t **set_off, const int32_t **units, int64_t *total) {
    if (!c || !set_off || !units) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists_device: null argument");
    SplitState *v = c->split;
    if (!v) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists_device: the stage is not enabled (bbmap_split_enable)");
    if (!(v->cfg.flags & BBMAP_SPLIT_LISTS)) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists_device: the stage builds no lists (BBMAP_SPLIT_LISTS)");
    if (v->added < 0) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists_device: no batch has been added yet");
    hipStream_t stream = (hipStream_t)stream_;
    BBHIP(hipSetDevice(c->cfg.device));
    if (stream != c->accum[ACC_SPLIT].stream) BBHIP(hipStreamSynchronize(c->accum[ACC_SPLIT].stream));      // behind the add that wrote the records
    const long long n = v->added;
    const int paired = c->cfg.paired, nsets = v->cfg.nsets;
    const long long need = bbsplit::lists_workspace_bytes(n, paired, nsets);
    if (need < 0) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists_device: the batch is too large for one scan");
    BBHIP(v->ws.grow((size_t)need, 0, &stream));
    long long *so = v->setoff.as<long long>();
    // sizing pass (counts, scan, set_off), the total comes back once, then the placing pass into an array of that size
    BBHIP(bbsplit::launch_lists(n, paired, nsets, v->recs.as<bbmap_splitrec>(), v->ws.p, need, so, nullptr, 0, stream));
    long long tot = 0;
    BBHIP(hipMemcpyAsync(&tot, so + 2 * nsets, 8, hipMemcpyDeviceToHost, stream));
    BBHIP(hipStreamSynchronize(stream));
    BBHIP(v->units.grow((size_t)(tot > 0 ? tot : 1) * 4, (size_t)tot));
    if (tot > 0) BBHIP(bbsplit::launch_lists(n, paired, nsets, v->recs.as<bbmap_splitrec>(), v->ws.p, need, so, v->units.as<int>(), tot, stream));
    v->total = tot;
    *set_off = v->setoff.as<int64_t>(); *units = v->units.as<int32_t>();
    if (total) *total = tot;
    return BBMAP_OK;
}

extern "C" int bbmap_get_split_lists(bbmap_ctx *c, int64_t *set_off_out, int32_t *units_out, int64_t units_cap, int64_t *total_out) {
    if (!c || !set_off_out) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists: null argument");
    if (units_cap < 0 || (units_cap > 0 && !units_out)) return bbfail(BBMAP_E_ARG, "bbmap_get_split_lists: bad buffer");
    const int64_t *so = nullptr; const int32_t *un = nullptr; int64_t tot = 0;
    BBTRY(bbmap_get_split_lists_device(c, nullptr, &so, &un, &tot));
    BBHIP(hipMemcpy(set_off_out, so, 8 * (2 * (size_t)c->split->cfg.nsets + 1), hipMemcpyDeviceToHost));      // (waits for the null stream)
    if (tot > 0 && tot <= units_cap) BBHIP(hipMemcpy(units_out, un, (size_t)tot * 4, hipMemcpyDeviceToHost));
    if (total_out) *total_out = tot;
    return BBMAP_OK;
}

extern "C" int bbmap_get_split_stats(bbmap_ctx *c, int64_t *out, int64_t cap_words) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_get_split_stats: null argument");
    SplitState *v = c->split;
    if (!v) return bbfail(BBMAP_E_ARG, "bbmap_get_split_stats: the stage is not enabled (bbmap_split_enable)");
    const int64_t bytes = bbpipe_refsplit_state_bytes(v->cfg.nkeys, v->cfg.nsets);
    if (cap_words * 8 < bytes) return bbfail(BBMAP_E_ARG, "bbmap_get_split_stats: the buffer is too small (4 + 4 nkeys + 4 nsets words)");
    BBHIP(hipSetDevice(c->cfg.device));
    return copy_out(c, ACC_SPLIT, out, v->state.p, (size_t)bytes);
}

extern "C" int bbmap_reset_split(bbmap_ctx *c) {
    if (!c) return bbfail(BBMAP_E_ARG, "bbmap_reset_split: null context");
    SplitState *v = c->split;
    if (!v) return BBMAP_OK;
    return reset_state(c, ACC_SPLIT, {{v->state.p, (size_t)bbpipe_refsplit_state_bytes(v->cfg.nkeys, v->cfg.nsets)}});
}

extern "C" int bbidx_get_chrom_table(bbidx_ctx *ix, int32_t *nchroms, const uint8_t **chromArr, int32_t *chromArrLen, int32_t cap) {
    if (!ix || !nchroms) return bbfail(BBMAP_E_ARG, "bbidx_get_chrom_table: null argument");
    *nchroms = ix->dev.nchroms;
    if (!chromArr && !chromArrLen) return BBMAP_OK;
    if (cap < ix->dev.nchroms + 1) return bbfail(BBMAP_E_ARG, "bbidx_get_chrom_table: buffers too small (need nchroms + 1 entries)");
    BBHIP(hipSetDevice(ix->device));
    if (chromArr) BBHIP(hipMemcpy(chromArr, ix->dev.chromArr, sizeof(void *) * (size_t)(ix->dev.nchroms + 1), hipMemcpyDeviceToHost));
    if (chromArrLen) BBHIP(hipMemcpy(chromArrLen, ix->dev.chromArrLen, 4 * (size_t)(ix->dev.nchroms + 1), hipMemcpyDeviceToHost));
    return BBMAP_OK;
}

extern "C" int bbmap_last_stats(bbmap_ctx *c, bbmap_stats *out) {
    if (!c || !out) return bbfail(BBMAP_E_ARG, "bbmap_last_stats: null argument");
    if (!c->ran) return bbfail(BBMAP_E_ARG, "bbmap_last_stats: no batch has been mapped yet");
    *out = c->stats;
    return BBMAP_OK;
}

extern "C" int bbmap_copy_to_host(void *dst, const void *src_device, int64_t bytes) {
    if (bytes < 0 || (bytes > 0 && (!dst || !src_device))) return bbfail(BBMAP_E_ARG, "bbmap_copy_to_host: bad argument");
    if (bytes > 0) BBHIP(hipMemcpy(dst, src_device, (size_t)bytes, hipMemcpyDeviceToHost));
    return BBMAP_OK;
}
