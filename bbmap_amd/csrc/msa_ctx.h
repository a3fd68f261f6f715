// Host-side context of the MultiStateAligner11ts entry points (msa_host.hip, msa_sort.hip, msa_gapped.hip, msa_legacy.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "bbmap_amd.h"
#include "host_common.h"
#include "msa_route.h"

struct bbmsa_ctx {
    bbmsa_config cfg = {};
    int device = 0;
    int numCUs = 0;
    RouteSwitches sw;           // scheme, band, and every switch the route of a launch depends on (msa_route.h)
    Route last;                 // the last launch's route, for the read-back entries (bbmsa_last_route, bbmsa_last_counts, ...)
    // fast kernel geometry
    int G = 0, R = 0, fastCols = 0, tmpBytes = 0, blocks = 0, ldsBytes = 0, tableLen = 0, wideTableLen = 0;
    long long dirSlotDwords = 0;
    unsigned int *d_dir = nullptr;
    unsigned int *d_counters = nullptr;   // bbmsa::kCounterWords words, named by bbmsa::CounterSlot (msa_common.h)
    DevBuf slowList;            // ints: the jobs the wavefront kernel hands on; as long as the largest launch so far
    // generic kernel
    int genThreads = 0;
    int *d_matrix = nullptr;
    int *d_limits = nullptr;
    // wide pass: the wavefront kernel again, 64 lanes per job and one job per 64-thread block, with an LDS column buffer as
    // wide as maxColumns, for the jobs the first pass found too wide for its own buffer (0 blocks = not needed)
    int wideR = 0, wideCols = 0, wideTmpBytes = 0, wideBlocks = 0, wideLdsBytes = 0;
    long long wideDirSlotDwords = 0;
    unsigned int *d_wideDir = nullptr;
    DevBuf slowList2;           // the wide pass's own hand-over list (only with a wide pass), as long as slowList
    // band kernel (msa_fill_band.hip): a job over 8 lanes, 32 diagonals, in front of the first pass.  Its switches and counters keep the
    // name of its predecessor, the one-job-per-lane narrow-window kernel.
    int narrowBlocks = 0, narrowSlack = 0;     // 0 blocks = disabled
    bool unlimitedStats = false;       // the kernels count for bbmsa_last_unlimited (BBMSA_UNLIMITED_STATS=1 or BBMAP_DP_COUNTS at bbmsa_create)
    unsigned int *d_widthHist = nullptr;       // the width sort's buckets (msa_sort.hip), allocated by the first sorted launch
    int bandRows = 0, bandLds = 0;     // longest read the band kernel takes, its LDS bytes per block
    unsigned int *d_bandDir = nullptr; // its records: per resident wave (bandRows + 1) x 2 jobs x 64 lanes dwords
    DevBuf fastList;            // ints: the wavefront kernel's job list when the band kernel or the width sort writes one
    // gapped-reference scratch (msa_gapped.hip), grown on demand: gapped references, their bookkeeping, the derived jobs
    DevBuf gref, gaux, gjobs;
    hipEvent_t ev[4] = {};  // start, after wavefront kernel, after generic kernel, after band kernel
    bool timed = false;
    bool legacyOnly = false;    // created with BBMSA_LEGACY_ONLY: bbmsa_fill_submit / _collect / _packed only
    struct bbmsa_legacy *legacy = nullptr;   // the per-call service of such a context (msa_legacy.hip)
    // strip-tiled wavefront kernel of the 9PacBio scheme (msa_fill_strip.hip)
    int stripBlocks = 0, stripLds = 0;
    long long stripDwords = 0, stripSlotDwords = 0;
    int *d_stripBoundary = nullptr;
    uint8_t *d_stripTmp = nullptr;
    // pipelined form of the strip kernel for launches with few jobs: pipeK wavefronts per job, pipeSlots jobs at a time
    int pipeK = 0, pipeSlots = 0;
    int *d_pipeBoundary = nullptr, *d_pipeSync = nullptr;
};

// the caller's arguments of one launch
struct JobBatch {
    int64_t n_jobs; const uint32_t *n_jobs_dev; const bbmsa_job *jobs; const uint8_t *reads, *refs; bbmsa_result *results; uint8_t *match;
    int32_t match_stride;
};
// what every kernel's parameter struct takes from the batch and the context
template <class P> void set_batch(P &p, const bbmsa_ctx *c, const JobBatch &B) {
    p.jobs = B.jobs; p.reads = B.reads; p.refs = B.refs; p.results = B.results; p.match = B.match;
    p.njobs = B.n_jobs; p.njobs_dev = B.n_jobs_dev; p.match_stride = B.match_stride;
    p.maxRows = c->cfg.maxRows; p.maxColumns = c->cfg.maxColumns; p.bandwidth = c->cfg.bandwidth; p.bandwidthRatio = c->cfg.bandwidthRatio;
}

// msa_sort.hip: the width sort in front of a sorted launch's first pass.  Writes the three thirds of c->fastList (each n_jobs ints:
// general, unlimited, band candidates) and the lists' lengths (CNT_LIST_COUNT and CNT_SORTED_COUNT, CNT_UNL_LIST_COUNT,
// CNT_CAND_COUNT).  band: the launch runs the band kernel, so its candidates get the third list.
int bbmsa_width_sort(bbmsa_ctx *c, hipStream_t stream, const bbmsa_job *jobs, int64_t n_jobs, bool band);

// msa_host.hip.  n_jobs_dev == NULL: n_jobs jobs.  Otherwise n_jobs is the capacity of the buffers and the kernels read the real
// count from *n_jobs_dev when they run.
int bbmsa_align_impl(bbmsa_ctx *c, void *stream_, int64_t n_jobs, const uint32_t *n_jobs_dev, const bbmsa_job *jobs,
                     const uint8_t *reads, const uint8_t *refs, bbmsa_result *results, uint8_t *match, int32_t match_stride);

// Internal (mapper_host.hip, which includes this header through mapper_ctx.h).  The mapper switches the band kernel off for launches it
// cannot help: small ones (its fill is a dependent chain of 2 * rows turns however few jobs there are, in front of the wavefront kernel
// on the same stream).  The final alignment stage's launches run it since it has 32 diagonals: realign_new pads its windows by >= 6
// columns and passes minScore - 120, which keeps 17-24 diagonals alive -- a third of those fills finish in the band.
void bbmsa_use_narrow(bbmsa_ctx *c, bool on);
// Makes `waiter` (a stream) wait until the context's last launch sequence has reached its first wavefront pass.  The mapper's two
// contexts run side by side; the second one's sequence begins with make_gref_kernel, and if the first context's persistent blocks
// are resident on every CU by then, the second context's passes (among them the latency-bound wide pass, which needs something
// to overlap with) only start when those drain: measured, the final stage 86 -> 93 ms.
int bbmsa_wait_first_pass(bbmsa_ctx *c, void *waiter);
// Launches of this context hand their jobs to the wavefront kernel in descending window width (a counting sort by columns / 8 in
// front of the first pass, the unlimited fills in front of the limited ones); results are indexed by job as always.  The mapper asks for it on its second context, whose windows
// span 170..640+ columns.
void bbmsa_sort_by_width(bbmsa_ctx *c, bool on);
// BBMSA_SORT_BY_WIDTH=1 in the environment switches it on for every context bbmsa_create makes (default 0; a caller that sets it,
// like the mapper, overrides it per context).
// A context with both the band kernel and bbmsa_sort_by_width on does not sort the launches the band kernel runs in (both write the
// wavefront kernel's list) -- unless this is on.  Then the sort's key is (class, width): unlimited fills, band candidates (the band
// kernel's own rule, band_is_candidate), everything else.  The band kernel walks the candidates' list and appends what it hands on
// behind the sorted general list, which the wavefront kernel's general build reads after it: [general, widest first | hand-overs].
// Two jobs of a 32-lane wavefront step together for max(columns) + lanes - 1 steps; sorted, partners have one width.
// Default off; BBMSA_SORT_WITH_BAND=1 in the environment applies it at bbmsa_create.  The mapper asks for it on its first context.
void bbmsa_sort_with_band(bbmsa_ctx *c, bool on);
// The launches of the 64-lane geometry (the latency route and the wide pass: one job per wavefront) take the build of the wavefront
// kernel that holds both step loops and gives an unlimited fill the prune-free one (a limited fill never takes it: fill_is_limited
// per job).  Default off; BBMSA_WIDE_UNLIMITED=1 applies it at bbmsa_create.  Without effect in a banded context (no such build).
void bbmsa_set_wide_unlimited(bbmsa_ctx *c, bool on);
// Launches of at most n jobs skip the first pass and run in the wide pass's geometry (64 lanes x ceil(rows / 64) rows per lane, one job
// per block): with few jobs a launch costs one wavefront's dependent chain, and three rows per lane make a step ~450 instructions
// instead of ~740.  Measured on the mapper's late rounds (a few hundred fills each): 236.0 -> 230.9 ms per step for the second
// context alone.  0 = off (the default of a context).
int bbmsa_set_latency_jobs(bbmsa_ctx *c, int64_t n);
// BBMSA_LATENCY_JOBS=n in the environment applies bbmsa_set_latency_jobs(c, n) to every 11ts context bbmsa_create makes (default 0;
// the mapper overrides it per context with BBMAP_LATENCY_JOBS).
// The route of the last launch as host flags, for callers that count launches without a device read-back:
// bit 0 narrow kernel ran, bit 1 width-sorted first pass, bit 2 latency route (no first pass).  bbmsa_last_route has the counters too.
enum { BBMSA_ROUTE_NARROW = 1, BBMSA_ROUTE_SORTED = 2, BBMSA_ROUTE_LATENCY = 4 };
int bbmsa_last_route_flags(const bbmsa_ctx *c);

// msa_legacy.hip: persistent buffers, stream and the call combiner of a BBMSA_LEGACY_ONLY context (c->d_matrix / d_limits exist)
int bbmsa_legacy_create(bbmsa_ctx *c);
void bbmsa_legacy_destroy(bbmsa_ctx *c);
// rows per lane of the last matrix-materialising launch (0: none yet) and the set of values launched so far (bit r)
void bbmsa_legacy_rows_per_lane(bbmsa_ctx *c, int *last, int *mask);
