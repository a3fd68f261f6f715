// What the mapper's kernels (mapper.hip, mapper_final.h) and its host code (mapper_host.hip, mapper_output.hip) share: constants,
// the per-read records, the kernels' argument block Dev, the names of the counter words and of the events, and the kernels the host
// launches.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_view.h"
#include "bbmap_amd.h"
#include "scaffold.h"

namespace bbmapper {

typedef bbmap_msite Site;

constexpr int GAPBUFFER2 = 128, GAPLEN = 128, MINGAP = 256;                       // Shared.java:21-26
constexpr int TIP_MAX_TIPLEN = 8, OUTER_DIST_MULT = 14, OUTER_DIST_DIV = 32;      // AbstractMapThread.java:2987-2993
constexpr int MIN_TRIM_SINGLE = 3, MIN_TRIM_PAIRED = 2;                           // BBMapThread.java:62-63
constexpr int GAPPED_BIT = 1 << 30;
constexpr int DEAD_MARK = 0x7fffffff;

struct Settings {
    float minRatio, ratioPaired, ratioPreRescue;
    int slowAlignPadding, slowRescuePadding, extraPadding, tipSearchDist, maxPairDist, averagePairDist, maxRescueDist,
        maxRescueMismatches, maxTrimSitesToRetain, trimList, doRescue, alignColumns, clearzone3, maxIndel, expLimit, paired;
    int rescueSkip;             // rescue() returns at once: "mating is not working" (AbstractMapThread.java:1146; bbmap_set_adaptive)
    // the aligner class's points (MultiStateAligner11ts: jni/MultiStateAligner11tsJNI.c:18-98; MultiStateAligner9PacBio:
    // current/align2/MultiStateAligner9PacBio.java:2375-2407): POINTS_MATCH, POINTS_MATCH2, POINTS_SUB / SUB2 / SUB3,
    // min(POINTS_DEL, POINTS_INS - POINTS_MATCH2) of maxImperfectScore, and CLEARZONE1e = 2*MATCH2 - MATCH - SUB + 1
    // (AbstractMapThread.java:142)
    int ptsMatch, ptsMatch2, ptsSub, ptsSub2, ptsSub3, impDelta, clearzone1e;
    int msaMaxColumns;          // columns of the reference's MSA instance (realign_new's padding rules read msa.maxColumns)
    int finalStage;
    // the final stage's use of the aligner class: POINTS_SUBR, the insertion tiers of calcInsScore (INS, INS2 up to length 5, INS3 up
    // to 20, INS4 beyond) and the deletion tiers of calcDelScore (DEL, DEL2 / DEL3 / DEL4 / DEL5 at the same limits, GAP per 128)
    int ptsSubR, ptsIns, ptsIns2, ptsIns3, ptsIns4, ptsDel, ptsDel2, ptsDel3, ptsDel4, ptsDel5, ptsGap;
    // the mapping thread's tail (final_begin_kernel / final_end_kernel): 0 = BBMapThread's, 1 = BBMapThreadPacBio's; its clearzones
    // CLEARZONEP / CLEARZONE1 / 1b / 1c = (int)(CLEARZONE_RATIO* x POINTS_MATCH2), CLEARZONE_LIMIT1e (BBMapThread only)
    int finalPolicy, czP, cz1, cz1b, cz1c, czLimit1e;
    int chunkLoads;             // BBMAP_CHUNK_LOADS: the byte loops load eight words per stream ahead of their use (Words::next8)
};

struct SlowState {      // scoreSlow's loop state of one read
    int idx;            // site being worked on
    int phase;          // 0 = look at site idx, 1 = first fill in flight, 2 = wider refill in flight, 3 = finished
    int minMsaLimit;
    int pending;        // job index of the fill in flight (GAPPED_BIT for the gapped log)
    int oldJob;         // phase 2: the first fill
    int expectedLen;
    int minscore;
    int seq;            // fills issued for this read so far
};

struct PairResc {       // rescue(): per pair and pass
    int first, count;   // its searches in the rescue job list
    int maxMismatches, retainLimit, retainLimit2, findTip;
    int unpaired2;      // pass A remembers mate 2's unpaired count for pass B (BBMapThread.java:1075-1081 runs before both)
    int ran;            // this pass's `if(unpaired>0 && numSites>0)` block runs (its mergeDuplicateSites of the loose list included)
};

struct RescInfo { int pair, anchorSite, strand, job; };   // per rescue search; job = DP job index or -1

// The words of Dev.counters (64 on the device; the host reads all of them back into a pinned copy after a kernel).
enum {
    CNT_FILLS = 0,              // plain fills asked for (beyond the log's capacity once a read found no room)
    CNT_GAPPED_FILLS = 1,       // gapped fills, likewise
    CNT_NEXT_ACTIVE = 2,        // next active count: reads a round leaves on the active list
    CNT_OVERFLOWED = 3,         // overflowed reads: their site list did not fit max_sites
    CNT_RESCUE_SEARCHES = 4,    // rescue searches of the pass
    CNT_NO_SITE = 5,            // reads without site
    CNT_REFILLS = 6,            // refills: the second, wider fill of a site
    CNT_RESCUE_FILLS = 7,       // rescue fills
    CNT_FILLS_DROPPED = 8,      // fills ahead of time that were dropped
    CNT_CROSS_SCAFFOLD = 9,     // sites quickMap's tail removed for spanning two scaffolds
    CNT_CLASS_LONG = 10,        // reads on the long-path class list (begin_kernel's, then final_begin_kernel's)
    CNT_CLASS_SHORT = 11,       // reads on the short-path class list, the word behind it
    CNT_TIER_FOUND = 16,        // units collect_overflow_kernel found for the overflow tier
    CNT_TIER_RESOLVED = 17,     // overflowed reads the tier gave a list (mark_tier_kernel)
    CNT_POOL_UNITS = 20,        // pool units handed out (beyond the capacity once a request failed)
    CNT_POOL_AT_FAILURE = 21,   // units in use when the first request failed
    CNT_POOL_FAILED = 22,       // requests that failed
    CNT_LOCAL_READS = 24,       // reads that need toLocalAlignment
    CNT_LOCAL_UNITS = 25,       // pool units those may take
    // host staging words, in the pinned copy only: values on their way to the device words named
    CNT_STAGE_FILLS = 32, CNT_STAGE_GAPPED = 33,        // -> CNT_FILLS, CNT_GAPPED_FILLS (one 8-byte copy)
    CNT_STAGE_POOL = 34,                                // -> CNT_POOL_UNITS
    CNT_WORDS = 64
};
// The events of a batch: the stage boundaries of one context's pass (bbmap_stats.ms_*), quick rescue's bracket, the overflow tier's.
enum { EV_START, EV_PROBE_END, EV_BEGIN_END, EV_SCORE_END, EV_SLOW_END, EV_FINISH_END, EV_RESCUE_END, EV_FINAL_END,
       EV_QUICK_BEGIN, EV_QUICK_END, EV_TIER_BEGIN, EV_TIER_END, EV_COUNT };

struct Dev {
    Settings S;
    const bbidx_read *reads;
    const uint8_t *bases;
    long long minusDelta, nreads;
    const uint8_t *const *chromArr;
    const int *chromArrLen;
    const uint8_t *refsBase;
    const bbidx_site *psites; const int *pnsites; int maxSites;
    Site *ms; int *mcount; int cap;
    int *nearArr;
    SlowState *slow;
    const int *activeIn; int *activeOut; int nActiveIn;
    // Class lists (BBMAP_CLASS_ORDER, nullptr = off): the reads with work ahead of them ("long path": a site that is not perfect) in
    // [0, nreads), the others ("short path") in [nreads, 2 * nreads), CNT_CLASS_LONG / CNT_CLASS_SHORT entries.  begin_kernel writes
    // them for score_kernel and scoreSlow's first round, final_begin_kernel for genMatchString's first round: those launches take
    // their reads long list first, so that a wavefront holds one kind of read and does not last as long as its one slow lane.
    int *classList;
    int classSwap;              // BBMAP_CLASS_ORDER=2 (tests): every read goes to the OTHER list -- results must not depend on the class
    unsigned *counters;         // CNT_*
    bbmsa_job *jobs; bbmap_jobinfo *jinfo; const bbmsa_result *results; long long jobCap;
    bbmsa_job *gjobs; bbmsa_gaps *ggaps; bbmap_jobinfo *ginfo; const bbmsa_result *gresults; long long gjobCap;
    bbresc_job *rjobs; RescInfo *rinfo; const bbresc_result *rres; PairResc *pres; long long rescCap;
    Site *rsite;                // per rescue search: the SiteScore under construction
    int pass;                   // rescue pass: 0 = mate 1 anchors, 1 = mate 2 anchors
    int plainColumns;           // widest window the first DP context takes
    int fillAhead;              // scoreSlow rounds: fill the sites behind the one in flight ahead of time
    // the final alignment stage (mapper_final.h)
    struct FinalRead *fin; bbmap_final *finalOut;
    uint8_t *pool; long long poolUnits;         // match strings: bump-allocated in 4-byte units, counters[CNT_POOL_UNITS] = units in use
    const uint8_t *match, *gmatch; int matchStride, gmatchStride;
    bbscaf::Table scaf;         // the index's scaffold table when it has a chromosome of two or more scaffolds, else off == nullptr
};

// the final stage's per-read state (mapper_final.h)
struct FinalRead {
    // stream.Read's mapping fields
    int mapped, paired, ambiguous, perfect, rescued;
    int chrom, strand, start, stop, mapScore;
    int match;                  // pool reference of Read.match (0 = null), length in matchLen
    int matchLen;
    // genMatchString's state
    int pc;                     // where to resume (PC_*), PC_DONE when the read has finished
    int i;                      // loop index over the sites
    int best, scoreChanged, sorting, topObj_, pairedLost;
    int oldSlow, oldScoreS;     // the site's scores before its match string was made
    // genMatchStringForSite
    int oldScoreG, gstep;
    // realign_new
    int recur, padding, forbidIndels, fixXY, minValid;
    int scoreNoIndel, minLoc, maxLoc, old0, epl, epr, fillKind, minscore, pending, haveMax, cols3;
    int seq;                    // fills issued for this read so far (continues scoreSlow's / rescue's numbering)
    int needLocal;              // the end kernel: toLocalAlignment is due (second pass, with pool space reserved)
    int reservedI;
};

// ---- the kernels the host launches (defined in mapper.hip and mapper_final.h)
// score_kernel, rescue_prep_kernel and final_round_kernel come in two builds.  KARG = false reads the by-value argument as written;
// where its address is needed (a helper that takes `const Dev &` or `const Settings &` and is not inlined) the compiler then copies
// all of it to private memory, in every lane of every launch -- these three do.  KARG = true reads the same bytes where the launch
// put them, in the kernel-argument segment, through a reference: no copy.  DEV_KERNEL picks the build (bbmap_ctx.kernargDev,
// BBMAP_KERNARG_DEV).  The other Dev kernels keep their argument in SGPRs as they are and have one build (slow_round_kernel's first
// round took 2.0 ms with the reference against 0.8 by value: DESIGN 8, "the per-read kernels").
#define DEV_KERNEL(c, name) ((c)->kernargDev ? name<true> : name<false>)
__global__ void begin_kernel(const Dev D);
template <bool KARG> __global__ void score_kernel(const Dev D);
__global__ void slow_round_kernel(const Dev D);
__global__ void finish_kernel(const Dev D);
__global__ void rescue_plan_kernel(const Dev D);
template <bool KARG> __global__ void rescue_prep_kernel(const Dev D);
__global__ void rescue_finish_kernel(const Dev D);
__global__ void final_begin_kernel(const Dev D);
template <bool KARG> __global__ void final_round_kernel(const Dev D);
__global__ void final_end_kernel(const Dev D);
__global__ void final_local_kernel(const Dev D);
__global__ void revcomp_unprobed_kernel(const bbidx_read *reads, long long n, int k, const uint8_t *in, uint8_t *out);
__global__ void collect_overflow_kernel(const int *mcount, long long nunits, int paired, int *ids, unsigned *count);
__global__ void gather_reads_kernel(const bbidx_read *reads, const int *ids, int nunits, int paired, bbidx_read *sub, int *readIds);
__global__ void mark_tier_kernel(int *mcount, const int *tierCount, const int *readIds, int n, unsigned *resolved);
__global__ void pack_counts_kernel(const int *mcount, long long n, int *counts);
__global__ void pack_sites_kernel(const Site *ms, const int *mcount, const long long *offsets, long long n, int cap, long long packedCap, Site *packed);
__global__ void scaffold_coords_kernel(const bbscaf::Table T, const BatchView V, bbmap_scafrec *out);
__global__ void tier_index_kernel(const int *ids, long long n, long long nreads, int *tierIdx);

}  // namespace bbmapper
