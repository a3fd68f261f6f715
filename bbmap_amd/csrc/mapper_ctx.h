// Host-side context of the mapper's entry points (mapper_host.hip: creation and the batch driver; mapper_output.hip: everything that
// reads a finished batch).  The error and launch helpers and DevBuf are the library's common ones (host_common.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <thread>
#include <vector>

#include "bbmap_amd.h"
#include "host_common.h"
#include "index_ctx.h"
#include "mapper_dev.h"
#include "msa_ctx.h"

// bbmap_map_batch's device copies (reads, bases of both strands, base scores, keyinfo, counts, offsets, packed sites), the scan
// scratch of bbmap_pack_sites_device, and bbmap_get_sam_records' scan scratch and text blob
enum { HIO_READS, HIO_BASES, HIO_SCORES, HIO_KEYINFO, HIO_COUNTS, HIO_OFFSETS, HIO_PACKED, BUF_PACK_TMP, BUF_SAM_TMP, BUF_SAM_TEXT, BUF_COUNT };

// The stages that accumulate finished batches into a state of their own.  Each takes a batch once (`counted`, cleared when the next
// batch is mapped or the state is reset), and only the work on `stream` -- that of the stage's last add, or of coverage's last
// finalize -- writes its state: getters wait for that stream, resets queue behind it.
enum { ACC_STATS, ACC_COV, ACC_HIST, ACC_SPLIT, ACC_COUNT };
struct Accum { bool counted = false; hipStream_t stream = nullptr; };

struct bbmap_ctx {
    bbmap_config cfg;
    bbidx_ctx *index;
    hipStream_t hostStream = nullptr;   // bbmap_map_batch (host buffers in and out) runs on it
    bbidx_launch probeLs;       // this context's probe launches: queue, work counters, events (the index is shared, read-only; index_ctx.h)
    bbmsa_ctx *msa, *msaGapped;
    bbmapper::Settings S;
    std::vector<void *> allocs;
    // device buffers
    bbidx_site *d_psites; int *d_pnsites;
    bbmap_msite *d_ms; int *d_mcount, *d_near;
    bbmapper::SlowState *d_slow;
    int *d_active[2];
    int *d_classList;               // Dev.classList: the long-path and the short-path read list (2 x max_reads), null without classOrder
    unsigned *d_counters;
    bbmsa_job *d_jobs; bbmap_jobinfo *d_jinfo; bbmsa_result *d_results; uint8_t *d_match;
    bbmsa_job *d_gjobs; bbmsa_gaps *d_ggaps; bbmap_jobinfo *d_ginfo; bbmsa_result *d_gresults; uint8_t *d_gmatch;
    bbresc_job *d_rjobs; bbmapper::RescInfo *d_rinfo; bbresc_result *d_rres; bbmapper::PairResc *d_pres; bbmap_msite *d_rsite;
    const uint8_t *const *d_chromArr; const int *d_chromArrLen; const uint8_t *refsBase;
    int *d_chromMin;
    long long *d_chromOff;
    long long jobCap, gjobCap, rescCap;
    bbmapper::FinalRead *d_fin; bbmap_final *d_final; uint8_t *d_pool; long long poolUnits, poolUsed, finalFills;
    int matchStride, gmatchStride, maxRows, plainColumns;
    unsigned *h_counters;           // pinned
    hipEvent_t ev[bbmapper::EV_COUNT];
    bbmap_stats stats;
    long long nJobs, nGapped;
    bool ran;
    // overflow tier: a second, small context with long site lists for the reads whose list did not fit max_sites
    bbmap_ctx *tier;
    bool ownsMsa;
    long long narrowMinJobs;        // plain-context launches with at least this many fills run the narrow kernel (BBMAP_NARROW_MIN_JOBS)
    bool sortWide;                  // the second context hands its fills on widest first (BBMAP_SORT_WIDE=0 switches it off)
    bool sortPlain;                 // so does the first context where it runs the band kernel (BBMAP_SORT_PLAIN=0 switches it off)
    bool classSwap;                 // BBMAP_CLASS_ORDER=2: the two lists swapped (tests: a read on the wrong list only costs time)
    bool classOrder;                // first rounds take their reads by class (BBMAP_CLASS_ORDER=0 switches it off)
    bool kernargDev;                // score / rescue_prep / final_round kernels read Dev in the kernel-argument segment (BBMAP_KERNARG_DEV=0: by value)
    int *d_tierUnits; bbidx_read *d_tierReads; int *d_tierReadIds;
    long long tierReads;            // reads the tier mapped in the last batch
    // The tier's pass runs beside the main pass (its reads are known once begin_kernel has run): its own stream, driven by its
    // own host thread, joined at the end of the batch.
    hipStream_t tierStream;
    // second-context fills (few jobs, wide windows: a handful of waves per CU) run on a stream of their own beside the plain ones
    hipStream_t dpStream; hipEvent_t evFork, evJoin;
    std::thread tierThread;
    bool tierStarted;
    int tierRc; char tierErr[320];
    long long overAfterBegin;       // reads flagged by the probe (CNT_OVERFLOWED after begin_kernel)
    struct BatchArgs { int64_t n_reads; const bbidx_read *reads; uint8_t *bases; int64_t minus_delta; const int8_t *baseScores; const int32_t *keyinfo; } batch;
    DevBuf buf[BUF_COUNT];          // HIO_* / BUF_*: kept between calls, grown on demand
    // bbmap_get_scaffold_records: its output (max_reads records) and the read -> overflow-tier record map, allocated on first use
    bbmap_scafrec *d_scafRec = nullptr;
    int *d_scafTier = nullptr;
    // bbmap_get_sam_records: records, per-read byte counts and their prefix sums, the MAPQ table (allocated on first use)
    bbmap_samrec *d_samRec = nullptr;
    bbmap_samtags *d_samTags = nullptr;     // (bbmap_get_sam_records_cfg with tags wanted: on its first use)
    int *d_samCounts = nullptr;
    long long *d_samOffsets = nullptr;
    float *d_mapqMax = nullptr;
    long long samTextBytes = 0;
    // run statistics (bbmap_add_run_stats): the running counters and the insert-size histogram, allocated on first use
    unsigned long long *d_runStats = nullptr, *d_insertHist = nullptr;
    int adaptive = 0;               // BBMAP_ADAPT_*
    long long numMatedSeen = 0;     // numMated after the last accumulation the insert-length rule looked at
    const bbmap_truth *truthNext = nullptr;     // bbmap_set_truth: for the next batch's own accumulation
    // coverage (bbmap_cov_enable): null until enabled
    struct CovState *cov = nullptr;
    // read histograms (bbmap_hist_enable): null until enabled
    unsigned long long *d_readHist = nullptr;
    int rhFlags = 0;
    // bbmap_untrim_batch_device (untrim.hip): the second match-string pool (swapped with d_pool by the call), per-read byte counts and
    // their prefix sums, allocated on first use
    uint8_t *d_pool2 = nullptr; long long pool2Units = 0;
    int *d_untrimCounts = nullptr;
    long long *d_untrimOffsets = nullptr;
    DevBuf untrimTmp;               // the scan's scratch
    bool untrimmed = false;         // the last batch has been untrimmed already
    // reference-set binning (bbmap_split_enable): null until enabled
    struct SplitState *split = nullptr;
    Accum accum[ACC_COUNT];         // run statistics, coverage, read histograms, reference-set binning
    // a new batch: no stage has taken it yet
    void new_batch() { for (Accum &a : accum) a.counted = false; untrimmed = false; }
};

// Reference-set binning state of a context (ref_split.hip): the tables are the host's, one entry per scaffold of the index's table as
// it was at bbmap_split_enable (`gen`).
struct SplitState {
    bbmap_split_config cfg = {};
    int nscaf = 0;
    long long gen = 0, added = -1, total = 0;       // added: reads of the batch the records belong to (-1 = none yet)
    DevBuf sets, keys, state, recs, ws, setoff, units;
    SplitState() = default;
    SplitState(const SplitState &) = delete;
    ~SplitState() { for (DevBuf *b : {&sets, &keys, &state, &recs, &ws, &setoff, &units}) b->release(); }
};

// Coverage state of a context: everything is sized by the index's scaffold table as it was at bbmap_cov_enable (`gen`).
struct CovState {
    int flags = 0, nscaf = 0, binsize = -1;
    long long slots = 0, nbins = 0, gen = 0;
    DevBuf covoff, len, diff[2], depth[2], recs, hist[2], totals, ws, refgc, binoff, bins[2];
    std::vector<int> hostLen;
    CovState() = default;
    CovState(const CovState &) = delete;
    ~CovState() {
        for (DevBuf *b : {&covoff, &len, &diff[0], &diff[1], &depth[0], &depth[1], &recs, &hist[0], &hist[1], &totals, &ws, &refgc, &binoff,
                          &bins[0], &bins[1]})
            b->release();
    }
};

// a device array of the context's that lives until bbmap_destroy
template <class T> static int dalloc(bbmap_ctx *c, T **p, size_t count) {
    void *d = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    if (hipMalloc(&d, bytes) != hipSuccess) return bbfail(BBMAP_E_NOMEM, "bbmap_create: device allocation failed");
    c->allocs.push_back(d);
    *p = (T *)d;
    return BBMAP_OK;
}
