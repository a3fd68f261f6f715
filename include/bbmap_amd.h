/*
 * bbmap_amd.h -- C ABI of libbbmap_amd.so, the MI355X (gfx950) replacement for the
 * native side of BBMap's `usejni=t` seed-and-extend path.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Every entry point names the
 * reference interface it replaces (paths relative to the reference checkout).
 * Return convention: 0 = ok, <0 = error (see BBMAP_E_*); the library never calls exit()
 * (the reference's native code does: jni/MultiStateAligner11tsJNI.c:130-132).
 *
 * The library REQUIRES a HIP device: there is no CPU fallback.  bbmsa_create() fails with
 * BBMAP_E_NODEVICE when no gfx950 device is usable.
 */
#ifndef BBMAP_AMD_H
#define BBMAP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (Still 6 with the configurable SAM stage: bbmap_sam_config, bbmap_samtags, bbmap_get_sam_records_cfg, bbmap_get_sam_cfg and
 * bbpipe_sam_records_device are additions; no earlier symbol, record or default changed, so no caller breaks.) */
#define BBMAP_AMD_ABI_VERSION 6

enum {
    BBMAP_OK = 0,
    BBMAP_E_NODEVICE = -1,   /* no HIP device / wrong architecture */
    BBMAP_E_ARG = -2,        /* bad argument (null pointer, negative size, shape beyond limits) */
    BBMAP_E_NOMEM = -3,      /* device or host allocation failed */
    BBMAP_E_HIP = -4,        /* a HIP runtime call failed; see bbmap_last_error() */
    BBMAP_E_SHAPE = -5       /* a job exceeds maxRows/maxColumns of the context */
};

/* Human-readable text of the last error on the calling thread. */
const char *bbmap_last_error(void);
int bbmap_abi_version(void);

/* =====================================================================================
 * MultiStateAligner11ts (affine-gap multi-state DP)
 *   replaces jni/MultiStateAligner11tsJNI.c (fillUnlimited :100-314, fillLimitedX :361-704)
 *   and fuses the Java-side walkers that read its `packed` matrix:
 *   current/align2/MultiStateAligner11tsJNI.java traceback2 :376-495, score2 :537-658,
 *   plus the call shape of current/align2/MSA.java fillAndScoreLimited :103-134.
 * ===================================================================================== */

/* job.flags: low 3 bits = fill mode, the rest are option bits */
enum {
    BBMSA_FILL_LIMITED_RAW   = 0, /* == C fillLimitedX(): minScore used as given, result[5]        */
    BBMSA_FILL_UNLIMITED_RAW = 1, /* == C fillUnlimited(): result[0..3]                             */
    BBMSA_FILL_LIMITED       = 2, /* == Java fillLimited(gaps==null): unlimited fallback gate +     */
                                  /*    minScore-=120 (MultiStateAligner11tsJNI.java:132-164)       */
    BBMSA_MODE_MASK          = 7,
    BBMSA_CLAMP_WINDOW = 1 << 3,  /* a=max(0,start), b=min(ref_len-1,end), MSA.java:104-105,118-121 */
    BBMSA_DO_SCORE     = 1 << 4,  /* run score2 on a non-null fill                                  */
    BBMSA_DO_TRACEBACK = 1 << 5,  /* run traceback2 on a non-null fill, write the match string      */
    BBMSA_NO_ITERATIONS = 1 << 6, /* the caller does not need result.iterations.  Accepted and without effect: until ABI 6 the     */
                                  /* library first tried such a job with a tighter minScore; fillLimitedX's pruning turned out not */
                                  /* to be admissible (a tighter bound can change a non-null result), so it never does now          */
    BBMSA_TRACE_KEEP_GAPS = 1 << 7, /* traceback: leave each gap symbol '-' of a gapped reference in the match string instead of expanding
                                    * it to 128 'D' (MultiStateAligner11tsJNI.java:481-493): the string then always fits rows + columns
                                    * bytes, and the caller expands it (a 16 kb deletion is 125 symbols, 16,000 'D') */
    BBMSA_INTERNAL_GAPPED = 1 << 8 /* set by the library on the jobs it derives for gapped references; never by callers */
};
/* the composite the mapper calls most: MSA.fillAndScoreLimited(read, ref, start, stop, minScore, null) */
#define BBMSA_FILL_AND_SCORE_LIMITED (BBMSA_FILL_LIMITED | BBMSA_CLAMP_WINDOW | BBMSA_DO_SCORE)

typedef struct bbmsa_job {
    int64_t read_off;     /* byte offset of read[0] inside the `reads` buffer                       */
    int64_t ref_off;      /* byte offset of ref[0] (the array refStartLoc/refEndLoc index into)     */
    int32_t read_len;     /* rows                                                                    */
    int32_t ref_len;      /* ref.length, used by BBMSA_CLAMP_WINDOW                                  */
    int32_t refStartLoc;
    int32_t refEndLoc;
    int32_t minScore;
    int32_t flags;
} bbmsa_job;              /* 40 bytes */

/* status values */
enum {
    BBMSA_ST_OK = 0,
    BBMSA_ST_NULL = 1,        /* the Java call would have returned null (below minScore)            */
    BBMSA_ST_BAD_SHAPE = 2    /* rows/columns outside the context limits: nothing was computed      */
};

typedef struct bbmsa_result {
    int32_t result[5];    /* {rows, maxCol, maxState, maxScore, belowMin} exactly as the C fills it  */
    int32_t status;
    int64_t iterations;   /* cells visited (what the C adds to iterationsLimited / ...Unlimited)     */
    int32_t score[8];     /* score2: {score,bestRefStart,bestRefStop,maxRow,maxCol,maxState,padL,padR} */
    int32_t score_len;    /* 0 (not run / null), 6 or 8                                              */
    int32_t match_len;    /* bytes of match string written (0 = none, -1 = slot too small)           */
    int32_t fill_kind;    /* 0 = limited fill ran, 1 = unlimited fill ran                            */
    int32_t columns;      /* columns actually aligned (after clamping)                               */
} bbmsa_result;           /* 80 bytes */

typedef struct bbmsa_ctx bbmsa_ctx;

typedef struct bbmsa_config {
    int32_t device;          /* HIP device ordinal                                                   */
    int32_t maxRows;         /* like MSA(maxRows_, maxColumns_), MSA.java:66-69; <= 640              */
    int32_t maxColumns;      /* <= 4096                                                              */
    int32_t bandwidth;       /* MSA.bandwidth (static in the reference, MSA.java:864)                */
    float   bandwidthRatio;  /* MSA.bandwidthRatio (MSA.java:865)                                    */
    int32_t reserved[3];     /* [0] lanes per job (0 = auto), [1] first-pass column buffer (0 = auto),
                              * [2] scoring scheme: BBMSA_SCHEME_11TS (0) or BBMSA_SCHEME_9PACBIO            */
} bbmsa_config;

/* Scoring schemes.  11ts: align2.MultiStateAligner11ts[JNI] (jni/MultiStateAligner11tsJNI.c:18-98), maxRows <= 640,
 * maxColumns <= 4096.  9PacBio: align2.MultiStateAligner9PacBio (current/align2/MultiStateAligner9PacBio.java:2359-2439:
 * 9 time bits, its own point values and barriers, column 0 as its constructor fills it), maxRows <= 6100,
 * maxColumns <= 8192: the strip-tiled wavefront kernel (banded fills: the one-job-per-thread kernel). */
#define BBMSA_SCHEME_11TS 0
#define BBMSA_SCHEME_9PACBIO 1
/* OR-ed into reserved[2]: a context for bbmsa_fill_submit / _collect / _packed only (what the per-call JNI symbols use, ONE per
 * process and MSA shape, shared by all mapping threads): persistent pinned + device staging for two batches of calls
 * (BBMSA_LEGACY_POOL_MB, default 64 MB each) and one scratch matrix, no batch buffers */
#define BBMSA_LEGACY_ONLY 0x100

int bbmsa_create(const bbmsa_config *cfg, bbmsa_ctx **out);
void bbmsa_destroy(bbmsa_ctx *ctx);

/* Device-resident batch: every pointer is a device pointer valid on cfg->device; the call only
 * enqueues work on `stream` (a hipStream_t passed as void*, NULL = default stream) and returns.
 * `match` receives one slot of `match_stride` bytes per job (may be NULL when no job asks for
 * BBMSA_DO_TRACEBACK). */
int bbmsa_align_batch_device(bbmsa_ctx *ctx, void *stream, int64_t n_jobs,
                             const bbmsa_job *jobs, const uint8_t *reads, const uint8_t *refs,
                             bbmsa_result *results, uint8_t *match, int32_t match_stride);

/* The same with the job count left on the device: the kernels read min(*n_jobs_dev, max_jobs) when they start (max_jobs =
 * capacity of jobs/results/match).  Lets a pipeline chain the site filter (which counts the jobs it writes) and the DP in
 * one stream without a host round trip. */
int bbmsa_align_batch_device_indirect(bbmsa_ctx *ctx, void *stream, const uint32_t *n_jobs_dev, int64_t max_jobs,
                                      const bbmsa_job *jobs, const uint8_t *reads, const uint8_t *refs,
                                      bbmsa_result *results, uint8_t *match, int32_t match_stride);

/* Host-buffer batch: copies in, runs, copies out, synchronises. */
int bbmsa_align_batch(bbmsa_ctx *ctx, int64_t n_jobs, const bbmsa_job *jobs,
                      const uint8_t *reads, int64_t reads_bytes,
                      const uint8_t *refs, int64_t refs_bytes,
                      bbmsa_result *results, uint8_t *match, int32_t match_stride);

/* Legacy per-call shape: ONE raw fill (mode = BBMSA_FILL_LIMITED_RAW or BBMSA_FILL_UNLIMITED_RAW) whose three score planes end up
 * in the caller's `packed` array exactly where the reference's native code leaves them
 * (state * (maxRows+1)*(maxColumns+1) + row * (maxColumns+1) + col; jni/MultiStateAligner11tsJNI.c:124-127, :707-812), so
 * that the unmodified Java score2 / traceback2 (current/align2/MultiStateAligner11tsJNI.java:376-658) can read them.  This
 * is what a drop-in Java_align2_MultiStateAligner11tsJNI_fill*JNI symbol calls.  The context must
 * have been created with BBMSA_LEGACY_ONLY; it may be shared by any number of threads, and should be: calls that arrive while
 * another is on the device are combined into one launch (one wavefront per fill), so throughput grows with the number of
 * calling threads.
 *   bbmsa_fill_submit   blocks until the fill has run and its planes sit in the context's pinned staging area; writes
 *                       result5 (result[0..4] of the native fill; [4] only for the limited fill) and INCREMENTS *iterations;
 *   bbmsa_fill_collect  copies the planes of that fill (rows 1..rows, columns 1..columns) into `packed`, and -- limited fill --
 *                       vertLimit[0..rows] / horizLimit[0..columns] as the native code leaves them (jni/...c:413-438); any of
 *                       the three may be NULL.  Pure memcpy: safe inside a JNI critical region.  Every successful submit must
 *                       be collected exactly once (the staging area is reused when its last fill has been collected);
 *   bbmsa_fill_packed   = submit + collect. */
typedef struct bbmsa_ticket {
    int32_t batch, slot;
    int64_t gen;             /* < 0: nothing to collect */
    int32_t rows, columns;
} bbmsa_ticket;
int bbmsa_fill_submit(bbmsa_ctx *ctx, const uint8_t *read, int32_t read_len, const uint8_t *ref, int32_t ref_len,
                      int32_t refStartLoc, int32_t refEndLoc, int32_t minScore, int32_t mode,
                      int32_t *result5, int64_t *iterations, bbmsa_ticket *ticket);
int bbmsa_fill_collect(bbmsa_ctx *ctx, bbmsa_ticket *ticket, int32_t *packed, int32_t *vertLimit, int32_t *horizLimit);
int bbmsa_fill_packed(bbmsa_ctx *ctx, const uint8_t *read, int32_t read_len, const uint8_t *ref, int32_t ref_len,
                      int32_t refStartLoc, int32_t refEndLoc, int32_t minScore, int32_t mode,
                      int32_t *result5, int64_t *iterations, int32_t *packed);
/* stats6: calls served, device batches launched, fills the wavefront kernel handed to the one-thread kernel; nanoseconds the
 * leaders spent in the wavefront pass (upload .. first synchronisation), in the hand-over pass, and waiting for collectors */
int bbmsa_legacy_stats(bbmsa_ctx *ctx, int64_t *stats6);

/* Gapped reference windows: job i is MSA.fillAndScoreLimited(read, ref, refStartLoc, refEndLoc, minScore, gaps)
 * (current/align2/MSA.java:103-134) for a SiteScore that carries a gap array.  When gaps[i].ngaps > 0 the library
 * builds the gapped reference (MultiStateAligner11tsJNI.makeGref, current/align2/MultiStateAligner11tsJNI.java:
 * 668-757: long gaps shrink to 64+rem bases, GAPC symbols, 64 bases), fills it as fillLimited(..., gaps) does
 * (:116-128), runs score(..., gapped=true) / traceback(..., gapped=true) (:362-372, :499-531) and translates
 * score[1], score[2] back to reference coordinates (:759-779).  Jobs with ngaps == 0 behave exactly as in
 * bbmsa_align_batch_device.  For gapped jobs the mode bits of job.flags select the Java fillLimited (any mode but
 * BBMSA_FILL_UNLIMITED_RAW) or fillUnlimited(read, ref, a, b, gaps) (:166-176; BBMSA_FILL_UNLIMITED_RAW), always with the
 * window clamp and score; BBMSA_DO_TRACEBACK is honoured.  The reference asserts gstart == 0 (:514); a job that
 * would break that, or whose gapped reference exceeds maxColumns + 2 bytes, gets BBMSA_ST_BAD_SHAPE. */
#define BBMSA_MAX_GAPS 16
typedef struct bbmsa_gaps { int32_t ngaps; int32_t gaps[BBMSA_MAX_GAPS]; } bbmsa_gaps;   /* 68 bytes */
int bbmsa_align_gapped_batch_device(bbmsa_ctx *ctx, void *stream, int64_t n_jobs, const bbmsa_job *jobs,
                                    const bbmsa_gaps *gaps, const uint8_t *reads, const uint8_t *refs,
                                    bbmsa_result *results, uint8_t *match, int32_t match_stride);
int bbmsa_align_gapped_batch_device_indirect(bbmsa_ctx *ctx, void *stream, const uint32_t *n_jobs_dev, int64_t max_jobs,
                                             const bbmsa_job *jobs, const bbmsa_gaps *gaps, const uint8_t *reads,
                                             const uint8_t *refs, bbmsa_result *results, uint8_t *match, int32_t match_stride);
int bbmsa_align_gapped_batch(bbmsa_ctx *ctx, int64_t n_jobs, const bbmsa_job *jobs, const bbmsa_gaps *gaps,
                             const uint8_t *reads, int64_t reads_bytes, const uint8_t *refs, int64_t refs_bytes,
                             bbmsa_result *results, uint8_t *match, int32_t match_stride);

/* Timing of the last bbmsa_align_batch_device launch sequence on this context, measured with
 * HIP events on the launch stream.  Valid after the stream has been synchronised. */
int bbmsa_last_kernel_ms(bbmsa_ctx *ctx, float *ms_fast, float *ms_slow);
/* The same per kernel: ms3 = {band kernel, wavefront kernel, generic kernel}. */
int bbmsa_last_kernel_ms3(bbmsa_ctx *ctx, float *ms3);
/* Which kernel took how many jobs of the last launch sequence: counts4 = {finished by the band kernel (a job over
 * 8 lanes, a band of 32 diagonals in registers), candidates it handed on because their window left the band, jobs given
 * to the wavefront kernel in total, jobs the wavefront kernel handed to the generic kernel}.  "Given to the wavefront kernel":
 * the jobs the band kernel did not try plus those it handed on; on a width-sorted launch that runs the band kernel
 * (BBMSA_SORT_WITH_BAND) the lengths of the sort's general and unlimited lists, so that the first three add up to the launch. */
int bbmsa_last_counts(bbmsa_ctx *ctx, int64_t *counts4);
/* Test hook for the width sort in front of a launch (BBMSA_SORT_BY_WIDTH, BBMSA_SORT_WITH_BAND): the job lists the last launch's
 * sort made -- lists3 holds 3 x n_jobs ints: the general list, the unlimited fills' list, the band kernel's candidates, each in
 * descending columns / 8; lens3 their lengths (entries past a length are not written).  n_jobs is the last launch's.  Fails when
 * that launch was not sorted.  Host only; waits for the launch sequence to finish. */
int bbmsa_debug_sorted_lists(bbmsa_ctx *ctx, int64_t n_jobs, int32_t *lists3, int64_t *lens3);
/* The route the last launch sequence took (host flags recorded at launch, then the device counters):
 * route8 = {band kernel ran (0/1), first pass in descending window width (0/1), latency route: no first pass, the
 * wide pass took every job (0/1), the context has a wide pass (0/1), job count read on the device (an _indirect entry, 0/1),
 * jobs the first pass handed on (9PacBio: the strip kernel to the generic kernel), jobs the wide pass handed to the generic
 * kernel, jobs the band kernel finished}.  Waits for the launch sequence to finish. */
int bbmsa_last_route(bbmsa_ctx *ctx, int64_t *route8);
/* How the wavefront kernel ran the unlimited fills (fillUnlimited: the raw mode, or MSA.fillLimited's gate) of the last launch
 * sequence, first and wide pass together: counts4 = {fills run by the kernel's build for unlimited fills (no limits, no prune
 * tests: a width-sorted launch sends it the unlimited fills that fit the first pass), unlimited fills run by the general build
 * (every other route, the wide pass, or BBMSA_UNLIMITED_LOOP=0 in the environment of bbmsa_create; with BBMSA_WIDE_UNLIMITED=1 the
 * latency route and the wide pass run a build that holds both loops, and their unlimited fills count under the first), wavefront steps (columns +
 * lanes in use - 1 per fill) of the unlimited fills, wavefront steps of all fills}.  A fill the first pass hands to the wide pass
 * counts there only.  The kernels count only in a context created with BBMSA_UNLIMITED_STATS=1 (or BBMAP_DP_COUNTS) in the
 * environment, since every fill pays atomics for it; otherwise the call fails.  Host only; waits for the launch sequence to
 * finish.  The 9PacBio scheme: zeros. */
int bbmsa_last_unlimited(bbmsa_ctx *ctx, int64_t *counts4);
/* Which build of the wavefront kernel the context launches: geo4 = {lanes per job, rows per lane of the first pass, columns of
 * the first pass's buffer, rows per lane of the wide pass (0: no wide pass)}.  A BBMSA_LEGACY_ONLY context launches one fill per
 * wavefront with the rows per lane its longest read of the launch asks for: geo4 = {64, rows per lane of the last launch (0: none
 * yet), maxColumns, bit r set for every rows-per-lane value r launched so far}.  The 9PacBio scheme has no such geometry: zeros. */
int bbmsa_geometry(bbmsa_ctx *ctx, int32_t *geo4);

/* =====================================================================================
 * BandedAligner (unit-cost edit distance in a diagonal band)
 *   replaces jni/BandedAlignerJNI.c (alignForward :123-239, alignForwardRC :241-355,
 *   alignReverse :357-470, alignReverseRC :472-585; JNI glue :588-757, header
 *   jni/align2_BandedAlignerJNI.h:17-41).  The reference ships two semantics that disagree
 *   (its Java class current/align2/BandedAlignerConcrete.java:100-551 is the live one,
 *   BandedAligner.java:18-22); the context selects which one is reproduced.
 * ===================================================================================== */
enum {
    BBBAND_FORWARD = 0, BBBAND_FORWARD_RC = 1, BBBAND_REVERSE = 2, BBBAND_REVERSE_RC = 3,
    BBBAND_DIR_MASK = 3,
    BBBAND_EXACT = 1 << 2       /* the `exact` argument: undefined bases only match themselves */
};
enum {
    BBBAND_SEMANTICS_JNI_C = 0,       /* big=999, width=min(maxWidth,2*maxEdits+1), off-centre penalty +i        */
    BBBAND_SEMANTICS_JAVA = 1         /* big=99999999, width also capped by 2*max(len)+2 and |1, penalty max(i,x) */
};

typedef struct bbband_job {
    int64_t query_off;    /* byte offsets into the `seqs` buffer */
    int64_t ref_off;
    int32_t query_len;
    int32_t ref_len;
    int32_t qstart;
    int32_t rstart;
    int32_t maxEdits;
    int32_t flags;        /* direction | BBBAND_EXACT */
} bbband_job;             /* 40 bytes */

typedef struct bbband_result {
    int32_t edits;        /* the function's return value */
    int32_t lastQueryLoc; /* returnVals[0..4] of the JNI call, jni/BandedAlignerJNI.c:604-630 */
    int32_t lastRefLoc;
    int32_t lastRow;
    int32_t lastEdits;
    int32_t lastOffset;
    int32_t status;       /* 0 ok, 2 bad shape (index outside its sequence) */
    int32_t reserved;
} bbband_result;          /* 32 bytes */

typedef struct bbband_ctx bbband_ctx;
typedef struct bbband_config {
    int32_t device;
    int32_t width;        /* constructor argument of BandedAligner: maxWidth = max(width,3)|1, <= 1023 */
    int32_t semantics;    /* BBBAND_SEMANTICS_* */
    int32_t reserved;
} bbband_config;

int bbband_create(const bbband_config *cfg, bbband_ctx **out);
void bbband_destroy(bbband_ctx *ctx);
int bbband_align_batch_device(bbband_ctx *ctx, void *stream, int64_t n_jobs, const bbband_job *jobs,
                              const uint8_t *seqs, bbband_result *results);
int bbband_align_batch(bbband_ctx *ctx, int64_t n_jobs, const bbband_job *jobs,
                       const uint8_t *seqs, int64_t seq_bytes, bbband_result *results);

/* BandedAligner's orchestration over the four directions (current/align2/BandedAligner.java:24-55), batched over
 * (query, ref) pairs held in one host buffer `seqs`; edits[i] = the method's return value for pair i.
 *   alignQuadruple(query, ref, maxEdits, exact)                        :39-48
 *   alignQuadrupleProgressive(query, ref, minEdits, maxEdits, exact)   :24-37  (minEdits >= 1, as every caller passes)
 *   alignDouble(query, ref, maxEdits, exact)                           :50-55 */
typedef struct bbband_pair { int64_t query_off, ref_off; int32_t query_len, ref_len; } bbband_pair;   /* 24 bytes */
int bbband_align_quadruple_batch(bbband_ctx *ctx, int64_t n_pairs, const bbband_pair *pairs, const uint8_t *seqs, int64_t seq_bytes,
                                 int32_t maxEdits, int32_t exact, int32_t *edits);
int bbband_align_quadruple_progressive_batch(bbband_ctx *ctx, int64_t n_pairs, const bbband_pair *pairs, const uint8_t *seqs,
                                             int64_t seq_bytes, int32_t minEdits, int32_t maxEdits, int32_t exact, int32_t *edits);
int bbband_align_double_batch(bbband_ctx *ctx, int64_t n_pairs, const bbband_pair *pairs, const uint8_t *seqs, int64_t seq_bytes,
                              int32_t maxEdits, int32_t exact, int32_t *edits);

/* =====================================================================================
 * k-mer index probe (align2.BBIndex.findAdvanced)
 *   The reference has NO native boundary for the index: BBIndex is pure Java.  This is the new seam
 *   SURVEY.md section 0/R3 proposes: AbstractIndex.findAdvanced(basesP, basesM, qual, baseScoresP,
 *   keyScoresP, offsets, id) -> ArrayList<SiteScore>  (current/align2/AbstractIndex.java:83; sole call
 *   site current/align2/AbstractMapThread.java:736), batched over reads.  The index itself
 *   (Block.sites/starts, current/align2/Block.java:162-165; AbstractIndex.COUNTS; the chromosome byte
 *   arrays) is uploaded once and stays resident in HBM.
 * ===================================================================================== */
/* Which of the reference's two index / mapper class families a context follows.  BBMAP: align2.BBIndex + BBMapThread + BBMap.setDefaults
 * + MultiStateAligner11ts (bbmap.sh).  PACBIO: align2.BBIndexPacBio + BBMapThreadPacBio + BBMapPacBio.setDefaults +
 * MultiStateAligner9PacBio (mapPacBio.sh).  BBIndexPacBio is BBIndex with other constants (current/align2/BBIndexPacBio.java:2461-2596:
 * k 12, MAX_INDEL 100 / MAX_INDEL2 800, Z_SCORE_MULT 25, INDEL_PENALTY KEY/8-1 and x25, HIT_FRACTION_TO_RETAIN .97, MIN_HIT_LISTS_TO_RETAIN
 * 12, SMALL_GENOME_LIST 80, MIN_SCORE_MULT .02, MIN_QSCORE_MULT(2) .005, DYNAMIC_SCORE_THRESH .64, MAX_HITS_REDUCTION_PERFECT 2,
 * clumpy-key constants 2800 / .8, FRACTION_GENOME_TO_EXCLUDE .005, the retry thresholds of find() 20/18/16/14 (:409-421)), reads of
 * up to 6000 bases and up to 2047 keys (:2394-2396), and its location-array score is MultiStateAligner9PacBio.calcAffineScore. */
enum { BBIDX_PROFILE_BBMAP = 0, BBIDX_PROFILE_PACBIO = 1 };

typedef struct bbidx_params {   /* the reference's mutable statics, BBIndex.java:3168-3305, AbstractIndex.java:100-160 */
    int32_t k, chromBits, minChrom, maxChrom;
    int32_t maxIndel, maxIndel2, minApproxHitsToKeep, kfilter;
    int32_t maxUsableLength, maxUsableLength2;
    int32_t maxHitsReduction2, maximumMaxHitsReduction, hitReductionDiv;
    int32_t quitAfterTwoPerfects, prescanQscore, trimByGreedy, slow;
    int32_t maxAverageListToSearch, maxAverageListToSearch2, maxShortestListToSearch;
    int64_t pointsPerSite;      /* Solver.POINTS_PER_SITE after analyzeIndex */
    int32_t profile;            /* BBIDX_PROFILE_*: the constants that are `static final` in the reference */
    int32_t reserved;
} bbidx_params;                 /* 96 bytes */

typedef struct bbidx_index_desc {   /* host pointers; everything is copied to the device by bbidx_create */
    bbidx_params params;
    int32_t nblocks;                /* blocks are index[baseChrom]; block b holds chromosomes b<<chromBits .. */
    int32_t nchroms;                /* chromosomes are numbered 1..nchroms */
    const int32_t *const *starts;   /* per block: 4^k + 1 ints */
    const int32_t *const *sites;    /* per block */
    const int64_t *numSites;        /* per block */
    const int32_t *counts;          /* AbstractIndex.COUNTS, 4^k ints */
    const int32_t *lengthHistogram; /* 1001 ints */
    const uint8_t *const *chromArr; /* [nchroms+1], entry 0 unused */
    const int32_t *chromArrLen;     /* array length of each chromosome */
    const int32_t *chromLengths;    /* Data.chromLengths[chrom] */
} bbidx_index_desc;

typedef struct bbidx_read {
    int64_t bases_off;      /* offset of basesP in `bases`; baseScoresP sits at the same offset in `baseScores` */
    int64_t keys_off;       /* offset (in ints) into `keyinfo`: offsets[nkeys] followed by keyScoresP[nkeys]   */
    int32_t len;
    int32_t nkeys;
} bbidx_read;               /* 24 bytes */

#define BBIDX_MAX_GAPS 16
typedef struct bbidx_site { /* stream.SiteScore as the probe emits it (current/stream/SiteScore.java:999-1011) */
    int32_t chrom, strand, start, stop, hits, score, perfect, semiperfect;
    int32_t ngaps;
    int32_t gaps[BBIDX_MAX_GAPS];
} bbidx_site;               /* 100 bytes */

enum { BBIDX_MAX_KEYS = 128, BBIDX_MAX_READ_LEN = 600 };          /* BBIDX_PROFILE_BBMAP (BBIndex keeps 256 keys, 600 bases) */
enum { BBIDX_PACBIO_MAX_KEYS = 2047, BBIDX_PACBIO_MAX_READ_LEN = 6016 };   /* BBIDX_PROFILE_PACBIO: HEAP_LENGTH 2047; reads are split at 6000 */

typedef struct bbidx_ctx bbidx_ctx;
int bbidx_create(int32_t device, const bbidx_index_desc *desc, bbidx_ctx **out);
void bbidx_destroy(bbidx_ctx *ctx);
/* Device-resident batch.  sites: n_reads x max_sites records; nsites[i] = sites found for read i (0 also for a read
 * shorter than k or without keys), -1 when max_sites was too small, or -2 when the probe declines the read:
 *  - for its size: more than BBIDX_MAX_KEYS keys or BBIDX_MAX_READ_LEN bases (BBIDX_PROFILE_BBMAP, kernels AUTO and LANE),
 *    more than BBIDX_PACBIO_MAX_KEYS keys or BBIDX_PACBIO_MAX_READ_LEN bases (BBIDX_PROFILE_PACBIO, and the LONG kernel on
 *    either profile);
 *  - the long-read kernel only: key offsets that are not ascending (a later key starts before an earlier one);
 *  - every kernel: the chromosomes minChrom..maxChrom lie in more than 32 index blocks (the prescan keeps 64 strand
 *    cycles): with minChrom 1, more than 32 chromosomes at chromBits 0, or 32 << chromBits or more at chromBits >= 1. */
int bbidx_find_batch_device(bbidx_ctx *ctx, void *stream, int64_t n_reads, const bbidx_read *reads,
                            const uint8_t *bases, const int8_t *baseScores, const int32_t *keyinfo,
                            bbidx_site *sites, int32_t max_sites, int32_t *nsites);
/* The same, and every probed read's reverse complement (AminoAcid.reverseComplementBases, which the mapper computes once
 * per read as basesM, current/align2/AbstractMapThread.java:643-655) is written to bases_rc_out at the read's offset: the
 * kernel has it in LDS anyway, which saves the separate bbpipe_revcomp_device pass.  Every read with nsites >= -1 and at
 * least k bases and one key is written.  Left untouched: reads shorter than k or without keys, and reads declined (-2) for
 * their size.  A read declined for its key order or for the 32-block limit may or may not have been written (the kernels
 * write the reverse complement before those checks); where it is, it is the correct one.  No byte outside the reads'
 * [bases_off, bases_off + len) ranges is written. */
int bbidx_find_batch_device_rc(bbidx_ctx *ctx, void *stream, int64_t n_reads, const bbidx_read *reads,
                               const uint8_t *bases, const int8_t *baseScores, const int32_t *keyinfo,
                               bbidx_site *sites, int32_t max_sites, int32_t *nsites, uint8_t *bases_rc_out);
int bbidx_find_batch(bbidx_ctx *ctx, int64_t n_reads, const bbidx_read *reads,
                     const uint8_t *bases, const int8_t *baseScores, int64_t bases_bytes,
                     const int32_t *keyinfo, int64_t keyinfo_ints,
                     bbidx_site *sites, int32_t max_sites, int32_t *nsites);

/* Work counters and HIP-event duration of the last bbidx_find_batch_device launch; valid once its
 * stream has been synchronised.  stats5 = {list entries consumed by the prescan, by the walk, extendScore calls,
 * reference bytes compared, site records written}. */
int bbidx_last_stats(bbidx_ctx *ctx, int64_t *stats5, float *kernel_ms);
/* What the last bbidx_find_batch_device launch ran, as the host chose it (waits for the launch): launch8 = {wave-kernel
 * groups, long-list variant (0/1), short-read instantiation (0/1), reads the wave kernel left to the per-lane kernel,
 * per-lane kernel groups, long-read kernel groups, the long kernel's LDS layout maxLen, its maxKeys}; 0 for a kernel that
 * did not run.  The environment variable BBIDX_MAX_GROUPS (read when a context is created; unset or 0 = no cap) clamps
 * every probe launch's grid, the mapper's included, so that each wavefront or lane probes many reads in turn. */
int bbidx_last_launch(bbidx_ctx *ctx, int64_t *launch8);

/* Index construction on the device: align2.IndexMaker4 (current/align2/IndexMaker4.java:303-421: count -> prefix sum ->
 * fill, lists in genome order) + BBIndex.analyzeIndex (current/align2/BBIndex.java:101-191: COUNTS, clumpy keys, length
 * histogram, MAX_USABLE_LENGTH) + the genome-size tuning of BBMap.loadIndex (current/align2/BBMap.java:367-381).
 * chromArr[1..nchroms] are host pointers to the chromosome byte arrays (entry 0 unused); chromBits < 0 = automatic
 * (BBMap.java:317-321).  The result is a ready-to-probe context; nothing but a few thousand histogram counters visits the
 * host. */
int bbidx_build(int32_t device, int32_t k, int32_t chromBits, int32_t nchroms,
                const uint8_t *const *chromArr, const int32_t *chromArrLen, bbidx_ctx **out);
/* The same for either profile (bbidx_build = BBIDX_PROFILE_BBMAP); k <= 0 takes the profile's default (13 / 12). */
int bbidx_build_profile(int32_t device, int32_t profile, int32_t k, int32_t chromBits, int32_t nchroms,
                        const uint8_t *const *chromArr, const int32_t *chromArrLen, bbidx_ctx **out);
/* The tunables a context works with (derived by bbidx_build, or as given to bbidx_create). */
int bbidx_get_params(bbidx_ctx *ctx, bbidx_params *out);
/* Copies one block's arrays back to the host (any pointer may be NULL): starts 4^k+1 ints, sites starts[4^k] ints
 * (sites_cap = capacity of the buffer), counts 4^k ints, lengthHistogram 1001 ints. */
int bbidx_export_block(bbidx_ctx *ctx, int32_t block, int32_t *starts, int32_t *sites, int64_t sites_cap,
                       int32_t *counts, int32_t *lengthHistogram);

/* Which probe kernel a context launches.  AUTO (default): one read per wavefront (registers + LDS), with the
 * one-read-per-lane kernel taking the reads that do not fit it (more than 64 keys).  LANE: the per-lane kernel
 * for every read (any shape up to BBIDX_MAX_KEYS / BBIDX_MAX_READ_LEN; kept as the cross-check). */
enum { BBIDX_KERNEL_AUTO = 0, BBIDX_KERNEL_LANE = 1,
       BBIDX_KERNEL_LONG = 2 };   /* the long-read kernel (up to 6016 bases, 2047 keys) for every read: what a BBIDX_PROFILE_PACBIO
                                   * context always runs; selectable on a BBMAP context as a third cross-check */
int bbidx_set_kernel(bbidx_ctx *ctx, int32_t kind);

/* Longest read of the batches to come (default BBIDX_MAX_READ_LEN).  Sizing hint, not a limit: the wavefront kernel keeps a
 * read's per-base arrays in LDS, and with reads of at most 160 bases it needs a third less of it and runs 8 waves per SIMD
 * instead of 6; reads longer than announced are still answered (by the per-lane kernel). */
int bbidx_set_max_read_len(bbidx_ctx *ctx, int32_t max_len);

/* Scaffold boundaries inside the chromosome arrays: Data.scaffoldLocs / scaffoldLengths / interScaffoldPadding (current/dna/Data.java),
 * as FastaToChromArrays2 packs FASTA records into chromosome arrays (current/dna/FastaToChromArrays2.java:432-524; Python:
 * bbmap_amd.reference.pack).  counts, locs and lengths have nchroms + 1 entries indexed by chromosome number (entry 0 unused, as in
 * bbidx_build's chromArr); chromosome c holds counts[c] scaffolds, starting at locs[c][i] (0-based, strictly ascending) with lengths
 * lengths[c][i].  nchroms must be the index's.  The table is copied to the device (CSR; a scaffold's global number, 0-based in FASTA
 * order, is its position in the concatenation of the chromosomes' lists) and belongs to the index context: every mapper that borrows
 * the index, its overflow tier included, uses it from its next batch on (do not call this while a batch runs).
 *   - counts == NULL clears the table.  A table whose chromosomes each hold one scaffold keeps the filter off (Data.isSingleScaffold
 *     is true when `array.length<2`): mapping is what it is without a table, and bbmap_get_scaffold_records still works.
 *   - With a chromosome of two or more scaffolds, quickMap's tail drops every probe site that spans two scaffolds, as
 *     removeOutOfBounds does when SAM is written (current/align2/AbstractMapThread.java:2444-2476); bbmap_stats.sites_cross_scaffold
 *     counts them.  Rescue and tip-deletion sites are not filtered (nor are they in the reference).
 *   - BBMAP_E_ARG, with the previous table left in force: nchroms other than the index's, a chromosome without scaffolds, a NULL row,
 *     starts that do not ascend strictly from 0, a length < 1 or a scaffold that reaches past its chromosome array (chromArrLen), or
 *     inter_scaffold_padding <= 0 while some chromosome holds two or more scaffolds. */
int bbidx_set_scaffolds(bbidx_ctx *ctx, int32_t nchroms, const int32_t *counts, const int32_t *const *locs,
                        const int32_t *const *lengths, int32_t inter_scaffold_padding);

/* =====================================================================================
 * The probe's per-read inputs: AbstractMapThread.quickMap up to its findAdvanced call
 *   (current/align2/AbstractMapThread.java:642-728): key error probabilities from the qualities (QualityTools.makeKeyProbs,
 *   current/align2/QualityTools.java:188-279), key placement (KeyRing.makeOffsets3, current/align2/KeyRing.java:396-506, with the
 *   density window of :663-676), key scores (QualityTools.makeKeyScores :125-133) and base scores (makeByteScoreArray :145-181).
 *   Float code on the mapping thread in the reference; its integer outputs are the probe's inputs.  Two forms with byte for byte the
 *   same output: host code, read by read (bbkeys_make, bbkeys_make_batch), and kernels over a batch that is already in device memory
 *   (bbkeys_make_batch_device: one read per lane, no libm on the device).
 * ===================================================================================== */
typedef struct bbkeys_config {
    int32_t k;                      /* KEYLEN */
    float keyDensity, maxKeyDensity, minKeyDensity;   /* BBMap.java:52-54 (1.9 / 3 / 1.5); BBMapPacBio.java:55-57 (3.5 / 4.5 / 2.8) */
    int32_t maxDesiredKeys;         /* 15 / 63 */
    int32_t minApproxHitsToKeep;    /* AbstractIndex.MIN_APPROX_HITS_TO_KEEP, 1 */
    int32_t semiperfectMode;        /* PERFECTMODE || SEMIPERFECTMODE */
    int32_t reserved;
} bbkeys_config;
int bbkeys_default_config(int32_t profile, bbkeys_config *cfg);
/* One read.  quality: numeric phred values (not ASCII), or NULL for a read without qualities.  Writes baseScores[len]; returns the
 * number of keys written to offsets[] / keyScores[] (cap entries each), 0 when quickMap would return without probing (read shorter
 * than k, mostly undefined, no usable key, all keys probably wrong), < 0 on a bad argument. */
int bbkeys_make(const bbkeys_config *cfg, const uint8_t *bases, const uint8_t *quality, int32_t len,
                int32_t *offsets, int32_t *keyScores, int32_t cap, int8_t *baseScores);
/* A batch: read i occupies bases[bases_off[i] .. + lens[i]) (qualities at the same offsets, or quality == NULL).  Fills reads[i],
 * keyinfo (offsets[nkeys] then keyScores[nkeys] per read, keys_off in ints) and baseScores; *keyinfo_used = ints written. */
int bbkeys_make_batch(const bbkeys_config *cfg, int64_t n_reads, const int64_t *bases_off, const int32_t *lens,
                      const uint8_t *bases, const uint8_t *quality, bbidx_read *reads, int32_t *keyinfo, int64_t keyinfo_cap,
                      int8_t *baseScores, int64_t *keyinfo_used);
/* bytes of device workspace bbkeys_make_batch_device needs for a batch of n_reads reads and total_bases bases (the sum of the reads'
 * len); < 0 on a bad argument */
int64_t bbkeys_device_workspace_bytes(const bbkeys_config *cfg, int64_t n_reads, int64_t total_bases);
/* Device form of bbkeys_make_batch.  reads[i].bases_off / .len are inputs, .keys_off / .nkeys outputs; reads, bases, quality (or
 * NULL), keyinfo, baseScores and workspace (256-byte aligned) are device pointers on the current device.  Enqueues on `stream` and
 * waits for it (the key total is needed on the host); *keyinfo_used (host) = ints written.  Writes baseScores over the reads'
 * [bases_off, bases_off + len) ranges only and keyinfo[0 .. *keyinfo_used) only; makes no device allocation.
 *   BBMAP_E_ARG before anything is launched: a bad argument, or a workspace smaller than n_reads alone demands.  The lengths live on
 *     the device, so the full test -- workspace_bytes >= bbkeys_device_workspace_bytes(cfg, n_reads, sum of len) -- follows once they
 *     have been summed: BBMAP_E_ARG with nothing but the workspace written.
 *   BBMAP_E_ARG when the keys need more than keyinfo_cap ints: keyinfo and reads are untouched (baseScores are written) and
 *     *keyinfo_used = the size needed, so the caller can retry.
 *   BBMAP_E_NODEVICE without a gfx950 device.  n_reads == 0: BBMAP_OK, *keyinfo_used = 0. */
int bbkeys_make_batch_device(const bbkeys_config *cfg, void *stream, int64_t n_reads, bbidx_read *reads,
                             const uint8_t *bases, const uint8_t *quality, int32_t *keyinfo, int64_t keyinfo_cap,
                             int8_t *baseScores, void *workspace, int64_t workspace_bytes, int64_t *keyinfo_used);

/* =====================================================================================
 * Quality trimming: qtrim= / trimq= / untrim=
 *   align2.TrimRead as the mapping thread applies it: TrimRead.trim before processRead (current/align2/AbstractMapThread.java:484-487)
 *   and, with untrim=t, TrimRead.untrim behind it (:518-521; bbmap_untrim_batch_device further down).  The trim stage restates
 *   TrimRead.trim(Read, ...) (current/align2/TrimRead.java:47-63): testOptimal (:264-324, a float32 running sum in read order),
 *   testRightWindow (:349-365), testLeft / testRight (:327-385), the N-only scans testLeftN / testRightN (:388-413) for a read without
 *   qualities, and the constructor's clamp to minLength (trim(int,int,int), :164-197: the excess comes off the left side first).
 *   A read is (bases_off, len) into a blob, so trimming moves no base: reads_out[i] = {bases_off + left, 0, len - left - right, 0}
 *   and trims[i] = {left, right}, both trims 0 when Java returns null or the clamp leaves nothing to trim.  The key stage
 *   (bbkeys_make_batch_device) then runs over reads_out.  Two forms with byte for byte the same output: host code (bbtrim_batch) and a
 *   kernel over a resident batch (bbtrim_batch_device: one read per lane, the error probability table handed to the kernel, no libm
 *   on the device).  Qualities above 126 are outside the domain, as in Java's table.
 *   Out of scope: trimBadSequence, trimFast / trimByAmount (BBDuk's callers), qtrim1 / qtrim2 and trimq lists, breakReads.
 * ===================================================================================== */
enum { BBTRIM_MODE_OPTIMAL = 0, BBTRIM_MODE_WINDOW = 1, BBTRIM_MODE_INTERVAL = 2 };
typedef struct bbtrim_config {
    int32_t mode;              /* TrimRead.optimalMode / windowMode / neither; tested in that order (TrimRead.java:51-61) */
    int32_t trimLeft, trimRight;
    int32_t trimq;             /* 0..126 */
    int32_t minLength;         /* TRIM_MIN_LENGTH */
    int32_t windowLength;      /* 4 */
    int32_t minGoodInterval;   /* 2 */
    float   optimalBias;       /* < 0: off; otherwise replaces PROB_ERROR[trimq] (TrimRead.java:265) */
} bbtrim_config;               /* 32 bytes */
typedef struct bbtrim_rec { int32_t left, right; } bbtrim_rec;
/* BBMap's: optimal mode, both sides off, trimq 6 (Parser.java:930), minLength 60 (AbstractMapper.java:2720), window 4, interval 2,
 * bias -1 */
int bbtrim_default_config(bbtrim_config *cfg);
/* Host form.  Read i occupies bases[reads_in[i].bases_off .. + len), its numeric phred qualities lie at the same offsets in
 * `quality` (NULL: reads without qualities).  reads_out must not alias reads_in.  BBMAP_E_ARG: a null argument, n_reads < 0,
 * aliasing, trimq outside 0..126, an unknown mode, windowLength < 1, minGoodInterval < 1, an optimalBias above 1 or NaN. */
int bbtrim_batch(const bbtrim_config *cfg, int64_t n_reads, const bbidx_read *reads_in, const uint8_t *bases,
                 const uint8_t *quality, bbidx_read *reads_out, bbtrim_rec *trims);
/* Device form: every pointer but cfg is a device pointer on the current device.  Enqueues one kernel on `stream`; makes no device
 * allocation and does not wait.  n_reads == 0: BBMAP_OK, nothing is launched. */
int bbtrim_batch_device(const bbtrim_config *cfg, void *stream, int64_t n_reads, const bbidx_read *reads_in,
                        const uint8_t *bases, const uint8_t *quality, bbidx_read *reads_out, bbtrim_rec *trims);

/* =====================================================================================
 * Merging overlapping read pairs: BBMerge's ratio-mode overlap search and the join
 *   Overlap search is BBMerge.mateByOverlap_ratioMode (current/jgi/BBMerge.java:1615-1639) over the two natives Java calls under
 *   usejni, mateByOverlapRatioJNI (flat weights) and mateByOverlapRatioJNI_WithQualities (jni/BBMergeOverlapper.c:127-402):
 *     rvector[4] = 0; the quality form runs when useQuality is set and the batch has qualities; the flat form runs when the quality
 *     form did not, or when withoutQuality is set and the quality form returned x < 0 or rvector[4] == 1; the record is the return
 *     value and rvector[2], rvector[4] of the last form that ran.
 *   The join is the overlapped branch of Read.joinRead(a, b, insert) (current/stream/Read.java:2804-2840), with and without
 *   qualities.  Mate 2 is handed over as it was sequenced: both stages reverse-complement it (and reverse its qualities) while they
 *   read it, as BBMerge does before the search (Read.reverseComplement, Read.java:1127-1131); no second copy of the batch is made.
 *   A read is (bases_off, len) into one blob; keys_off / nkeys are ignored; numeric phred qualities lie at the same offsets in
 *   `quality`.  Two forms with the same output on every input: host code (bbmerge_*_batch) and kernels over a resident batch
 *   (bbmerge_*_batch_device).  good and bad are float32 sums taken column by column in the reference's order; the natives' inner
 *   early exit is not reproduced, because the addends are not negative: a full column sum fails `bad <= badlimit` exactly when the
 *   truncated one does and equals it otherwise.
 *   These two entry points give the record of the natives.  BBMerge's answer for a pair -- the entropy-derived minOverlap, the normal
 *   mode, the composition of the two modes, efilter / pfilter and the return code -- is bbmerge_verdict_batch, further down.
 *   Out of scope everywhere: the `loose` branches, trim-on-failure, ecco, the Tadpole filters and extension, adapter detection and
 *   verification, preprocess and the qtrim retries, the no-overlap branch of joinRead (insert >= alen + blen), and JNI.
 * ===================================================================================== */
#define BBMERGE_MAX_READ_LEN 512
typedef struct bbmerge_config {
    int32_t minOverlap0, minOverlap, minInsert0, minInsert;   /* as handed to the natives: MIN_OVERLAPPING_BASES_0 - reduction, minOverlap -
                                                                 reduction, minInsert0, minInsert: 5, 8, 26, 35.  The natives clamp the first two
                                                                 themselves (minOverlap = max(4, minOverlap0, minOverlap), minOverlap0 = mid(4, ...)) */
    float   maxRatio, ratioMargin, ratioOffset, gIncr, bIncr; /* .09, 5.5, .55, .95, .95 */
    int32_t useQuality, withoutQuality;                       /* overlapUsingQuality 0, overlapWithoutQuality 1 */
    int32_t maxMergeQuality;                                  /* Read.MAX_MERGE_QUALITY, maxq=: 41 */
} bbmerge_config;              /* 48 bytes */
enum { BBMERGE_INFO_QUALITY = 1,      /* the quality form ran */
       BBMERGE_INFO_FLAT = 2,         /* the flat form ran */
       BBMERGE_INFO_SKIPPED = 256 };  /* not evaluated: a mate longer than BBMERGE_MAX_READ_LEN, or, where the quality form would run,
                                         a quality outside 0..70 (the domain of probCorrect): insert -1, bad 0, ambig 0 */
typedef struct bbmerge_rec {
    int32_t insert;            /* the native's return value: -1 or the insert size */
    int32_t bad;               /* rvector[2] */
    int32_t ambig;             /* rvector[4] */
    int32_t info;              /* BBMERGE_INFO_* */
} bbmerge_rec;                 /* 16 bytes */
/* BBMerge's defaults (BBMerge.java:2220-2221, :2278-2279, :2334-2346, :605-611) */
int bbmerge_default_config(bbmerge_config *cfg);
/* Host form.  Pair i is reads1[i] and reads2[i]; `quality` may be NULL (only the flat form can run).  BBMAP_E_ARG: a null argument,
 * n_pairs < 0, a NaN among the floats, ratioMargin < 1 (Java's assert), gIncr or bIncr < 0 (the full sums above need addends that are
 * not negative), minInsert0 or minInsert < 0 (an insert below 0 has no columns), maxMergeQuality outside 0..127.  minOverlap0 >
 * minOverlap is no error: the natives clamp. */
int bbmerge_overlap_batch(const bbmerge_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                          const uint8_t *bases, const uint8_t *quality, bbmerge_rec *recs);
/* Device form: every pointer but cfg is a device pointer on the current device.  Enqueues on `stream` (one wavefront per pair, once
 * for pairs whose mates fit 192 bases and once for the longer ones), makes no device allocation and does not wait.  n_pairs == 0:
 * BBMAP_OK, nothing is launched.  BBMAP_E_NODEVICE without a gfx950 device. */
int bbmerge_overlap_batch_device(const bbmerge_config *cfg, void *stream, int64_t n_pairs, const bbidx_read *reads1,
                                 const bbidx_read *reads2, const uint8_t *bases, const uint8_t *quality, bbmerge_rec *recs);
/* The join, host form.  insert[i] is the caller's decision (the usual rule: rec.insert > 0 && !rec.ambig ? rec.insert : 0).
 * merged[i].bases_off is an input and names a slot of at least alen + blen bytes in out_bases (and out_quality); merged[i].len is an
 * output: the insert, or 0 for insert <= 0 or insert >= alen + blen, and then nothing of the slot is written; keys_off and nkeys are
 * left alone.  Bytes of a slot beyond len are not written.  With quality == NULL out_quality may be NULL and joinRead's rules for
 * reads without qualities apply.  Only maxMergeQuality of cfg is used; BBMAP_E_ARG as above.  No length limit. */
int bbmerge_join_batch(const bbmerge_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                       const uint8_t *bases, const uint8_t *quality, const int32_t *insert, bbidx_read *merged,
                       uint8_t *out_bases, uint8_t *out_quality);
/* Device form of the join, one lane per output base: as bbmerge_overlap_batch_device. */
int bbmerge_join_batch_device(const bbmerge_config *cfg, void *stream, int64_t n_pairs, const bbidx_read *reads1,
                              const bbidx_read *reads2, const uint8_t *bases, const uint8_t *quality, const int32_t *insert,
                              bbidx_read *merged, uint8_t *out_bases, uint8_t *out_quality);

/* -------------------------------------------------------------------------------------
 * BBMerge's verdict per pair: what bbmerge.sh decides under its defaults, the strict / vstrict / ustrict / xstrict / fast presets
 * and their flags.  BBMerge.mateByOverlap (current/jgi/BBMerge.java:1741-1837) inside processReadPair_inner (:2044-2068):
 *   1. minOverlap per pair from entropy (calcMinOverlapFromEntropy :1696-1711, the branch without `loose`):
 *      max(minOverlapBases, calcMinOverlapByEntropyTail(mate 1), calcMinOverlapByEntropyHead(mate 2 reverse-complemented))
 *      (BBMergeOverlapper.java:860-934); useEntropy 0 gives minOverlapBases.
 *   2. Ratio mode (:1615-1639): the search of bbmerge_overlap_batch with minOverlap0 = minOverlapBases0 - ratioReduction and
 *      minOverlap = (the pair's minOverlap) - ratioReduction.  `ratio.minOverlap0` and `ratio.minOverlap` are NOT read here.
 *   3. Normal mode (mateByOverlap_normalMode :1641-1661, :1690-1693): up to qualIters passes (one without qualities) of
 *      BBMergeOverlapper.mateByOverlapJava_unrolled (BBMergeOverlapper.java:543-657) with minOverlap0 - i, minOverlap + i and
 *      minQuality - 2 i.  That is the form Java runs (its native is switched off, :68), and it differs from the native in one
 *      index: Java weighs a column by aprob[j] * bprob[i] (:591), jni/BBMergeOverlapper.c:73 by aprob[j] * bprob[j].  The Java is
 *      followed.  The inner early exit is not reproduced: a truncated column loop ends with bad = bestBad + margin + 1, which fails
 *      both `bad <= bestBad` and `bad < margin` (bestBad >= 0), so such an overlap never changes state, with full counts either.
 *   4. The composition of the two modes (:1765-1805) incl. requireRatioMatch, bestBad > maxMismatchesR (:1809), the early
 *      RET_AMBIG / RET_NO_SOLUTION (:1811-1814), efilter (:1817-1824, expectedMismatches, BBMergeOverlapper.java:667-724) and
 *      pfilter (:1826-1831, probability, :728-785) -- float32 sums and products in the reference's column order, the quotient in
 *      float32, the square root in double -- and the return code (:2061-2067).
 *   With useQuality 0 the pair counts as having no qualities in every stage (:1913-1916); the filters run only with qualities.
 *   Not built: the `loose` branches (:1664-1672, :1699-1704), trim-on-failure (:1674-1687; the config is trimonfailure=0), ecco,
 *   the Tadpole filters and extension, adapter verification, preprocess, the qtrim retries, minsecondratio (read by the Java ratio
 *   forms only).
 *   Deviation: a pair with a quality above 59 is skipped up front while a filter is on (Java throws once it reaches the filter:
 *   probCorrect2 has 60 entries), and one with a quality above 70 where the quality form or the normal mode would read probCorrect.
 * ------------------------------------------------------------------------------------- */
typedef struct bbmerge_verdict_config {
    bbmerge_config ratio;                                      /* the ratio search's numbers, minInsert0 / minInsert (also the normal
                                                                  mode's and the return code's) and maxMergeQuality */
    int32_t useEntropy, entropyK, minEntropyScore;             /* 1, 3 (1..5), 39 */
    int32_t minOverlapBases, minOverlapBases0, ratioReduction; /* MIN_OVERLAPPING_BASES 11, MIN_OVERLAPPING_BASES_0 8,
                                                                  MIN_OVERLAPPING_BASES_RATIO_REDUCTION 3 */
    int32_t useRatioMode, useNormalMode, requireRatioMatch;    /* 1, 0, 0 */
    int32_t maxMismatchesR;                                    /* MAX_MISMATCHES_R 20 */
    int32_t margin, maxMismatches, maxMismatches0;             /* normal mode: MISMATCH_MARGIN 2, MAX_MISMATCHES 3, MAX_MISMATCHES0 3 */
    int32_t minQuality, qualIters;                             /* normal mode: MIN_QUALITY 10, QUAL_ITERS 3 */
    int32_t useQuality;                                        /* BBMerge.useQuality 1 (ratio.useQuality is overlapUsingQuality) */
    int32_t useEfilter;                                        /* 1 */
    float   efilterRatio, efilterOffset, pfilterRatio;         /* 6, 0.05, 0.00004 */
    int32_t maxLength;                                         /* maxReadLength; 0 = no limit */
    int32_t reserved;
} bbmerge_verdict_config;      /* 136 bytes */
enum { BBMERGE_INFO_RATIO = 4,        /* the ratio mode ran */
       BBMERGE_INFO_NORMAL = 8,       /* the normal mode ran */
       BBMERGE_INFO_EFILTER = 16,     /* expectedMismatches was evaluated; otherwise `expected` is 0 */
       BBMERGE_INFO_PFILTER = 32 };   /* probability was evaluated; otherwise `probability` is 0 */
enum { BBMERGE_RET_NO_SOLUTION = -1, BBMERGE_RET_AMBIG = -2, BBMERGE_RET_SHORT = -4, BBMERGE_RET_LONG = -5 };
typedef struct bbmerge_verdict_rec {
    int32_t code;                      /* processReadPair_inner's return value: the insert, or BBMERGE_RET_* */
    int32_t minOverlap;                /* calcMinOverlapFromEntropy */
    int32_t insertRM, badRM, ambigRM;  /* mateByOverlap's locals; -1, 0, 0 where the ratio mode did not run */
    int32_t insertNM, badNM, ambigNM;  /* -1, 99999, 0 where the normal mode did not run */
    int32_t bad;                       /* bestBad as :1789-1805 composes it */
    float   expected, probability;     /* the filters' values (a NaN is the canonical one, 0x7fc00000) */
    int32_t info;                      /* BBMERGE_INFO_*; a SKIPPED pair has code -1, minOverlap 0, -1 0 0, -1 99999 0, bad 0 */
} bbmerge_verdict_rec;         /* 48 bytes */
#define BBMERGE_HIST_LEN 2000
typedef struct bbmerge_stats {
    int64_t pairs, merged, ambiguous, tooShort, tooLong, noSolution, skipped;   /* pairs = the sum of the other six */
    int64_t insertSum, insertMin, insertMax;                   /* over merged pairs; the caller starts insertMin at 999999999 */
    int64_t hist[BBMERGE_HIST_LEN];                            /* hist[min(insert, 1999)]++ per merged pair (:1406-1408) */
} bbmerge_stats;               /* 16080 bytes */
/* BBMerge's defaults: bbmerge_default_config and the table above */
int bbmerge_default_verdict_config(bbmerge_verdict_config *cfg);
/* Host form; arguments as bbmerge_overlap_batch.  `stats` may be NULL; otherwise the call ADDS this batch to it (a skipped pair
 * counts in pairs and skipped only).  BBMAP_E_ARG: what bbmerge_overlap_batch refuses, entropyK outside 1..5, qualIters < 1,
 * maxMismatches0 < 0, maxMismatches0 < maxMismatches, margin > maxMismatches, neither mode on, a NaN among the three floats.
 * minOverlapBases, minOverlapBases0, ratioReduction, minEntropyScore and minQuality take any value and are clamped where the
 * reference clamps them: the ratio natives raise their two overlaps to at least 4, the normal mode starts at overlap
 * max(min(max(1, minOverlapBases0 - i), minOverlap + i), 0) and takes minprob from probCorrect[mid(1, minQuality - 2 i, 41)], and
 * a score the scan never reaches gives len + 1; no value leads outside a pair's alen + blen inserts. */
int bbmerge_verdict_batch(const bbmerge_verdict_config *cfg, int64_t n_pairs, const bbidx_read *reads1, const bbidx_read *reads2,
                          const uint8_t *bases, const uint8_t *quality, bbmerge_verdict_rec *recs, bbmerge_stats *stats);
/* Device form: as bbmerge_overlap_batch_device (one wavefront per pair, two length classes, no allocation, no wait, n_pairs == 0
 * launches nothing).  `stats` is device memory that the caller has initialised; a third kernel counts the records into it: a
 * thread counts in registers, a workgroup sums in LDS (its histogram too), then vector atomics add the workgroup's sums. */
int bbmerge_verdict_batch_device(const bbmerge_verdict_config *cfg, void *stream, int64_t n_pairs, const bbidx_read *reads1,
                                 const bbidx_read *reads2, const uint8_t *bases, const uint8_t *quality, bbmerge_verdict_rec *recs,
                                 bbmerge_stats *stats);

/* =====================================================================================
 * Batch helpers (device-resident) used by the mapper below; also callable on their own.
 * ===================================================================================== */
/* bases_out[read] = reverse complement of bases_in[read] (AminoAcid.reverseComplementBases) */
int bbpipe_revcomp_device(void *stream, int64_t n_reads, const bbidx_read *reads,
                          const uint8_t *bases_in, uint8_t *bases_out);

/* Paired-read rescue scan: AbstractMapThread.quickRescue(bases, chrom, strand, loc, searchDist, searchRight, idealStart,
 * maxAllowedMismatches, POINTS_MATCH, POINTS_MATCH2) (current/align2/AbstractMapThread.java:2300-2391), batched.  `reads`
 * holds the mate's bases already on the strand to search; chromosome c occupies refs[chrom_off[c] .. + chrom_len[c]) and
 * chrom_min_index[c] is ChromosomeArray.minIndex.  result.found: 1 = a SiteScore (start, stop, score; mismatches is what
 * the reference parks in ss.slowScore; perfect/semiperfect from SiteScore.setPerfect), 0 = null, -2 = read longer than
 * 600.  use_affine selects the reference's USE_AFFINE_SCORE score formula (:2376-2380). */
typedef struct bbresc_job {
    int64_t read_off;
    int32_t read_len, chrom, loc, searchDist, idealStart, maxAllowedMismatches;
    int32_t flags;            /* bit 0: searchRight */
    int32_t reserved;
} bbresc_job;                 /* 40 bytes */
typedef struct bbresc_result { int32_t found, start, stop, score, mismatches, perfect, semiperfect, maxContig; } bbresc_result;   /* 32 bytes */
int bbpipe_quick_rescue_device(void *stream, int64_t n_jobs, const bbresc_job *jobs, const uint8_t *reads,
                               const int64_t *chrom_off, const int32_t *chrom_len, const int32_t *chrom_min_index,
                               const uint8_t *refs, bbresc_result *results,
                               int32_t points_match, int32_t points_match2, int32_t use_affine, int32_t base_hit_score);


/* =====================================================================================
 * Mapper control flow around the two hot kernels, device-resident.
 *   The part of align2.BBMapThread.processRead / processReadPair (current/align2/BBMapThread.java:389-490, :943-1098)
 *   that decides WHICH probe sites are aligned, with which window and minScore, in which order, and which rescue searches
 *   run, kept on the device so that a read batch stays in HBM from the probe to the last alignment:
 *     quickMap tail      AbstractMapThread.java:736-751 (findAdvanced; removeOutOfBounds :2444-2476)
 *     pairing + trimming BBMapThread.java:736-940 pairSiteScoresInitial, :140-249 trimList (Tools.java:654-674, :1113-1161)
 *     scoreNoIndels      AbstractMapThread.java:762-856;  findTipDeletions :1075-1141, :2178-2292
 *     scoreSlow          BBMapThread.java:252-386 -- the exact per-read SEQUENCE: every site's minScore follows the previous
 *                        sites' results (minMsaLimit, :376) and a fill that asks for more padding is repeated wider (:312-335),
 *                        so the DP runs in rounds (round j = the j-th fill of every read that still has one)
 *     mergeDuplicateSites Tools.java:697-759
 *     rescue / slowRescue AbstractMapThread.java:1144-1306 (quickRescue :2303-2404), mate 1 as anchor, then mate 2
 *   Configuration: bbmap.sh defaults (BBMap.setDefaults, BBMap.java:45-65), reads without qualities.
 *     the final stage    BBMapThread.java:492-732 / :1116-1356 (cfg.finalStage): final pairing (pairSiteScoresFinal), the ambiguity
 *                        policy, genMatchString -> genMatchStringForSite -> realign_new (AbstractMapThread.java:860-1068,
 *                        TranslateColorspaceRead.java:229-653: up to three fillLimited and one fillUnlimited per call, again in rounds),
 *                        fixXY / clipTipIndels / toLocalAlignment, applyClearzone3 and the tip penalty -> bbmap_final per read
 *   Adaptive state of the Java mapper (DYNAMIC_INSERT_LENGTH, the "mating is not working" skip of rescue()): opt-in through
 *   bbmap_set_adaptive, driven by the run statistics (bbmap_add_run_stats), batch by batch and per context.
 *   Not carried over: the non-default output policies (ambiguous=toss/random/all, secondary alignments, identity / edit filters,
 *   local alignment).
 *   Scaffolds: with a table set (bbidx_set_scaffolds) quickMap's tail drops sites that span two scaffolds, and
 *   bbmap_get_scaffold_records gives SamLine's scaffold coordinates, and bbmap_get_sam_records the rest of SamLine's constructor
 *   (FLAG, POS / PNEXT / TLEN, MAPQ, CIGAR with the `N` operator under an intron limit, NM, AM, MD and the values of the further
 *   optional tags); names, SEQ / QUAL text and file I/O stay with the host.
 *   Added product: every successful fill also returns its traceback string (as the quickmatch=t branch obtains it,
 *   BBMapThread.java:345, without fixXY / clipTipIndels); site state follows the default (quickmatch=f) flow.
 * ===================================================================================== */
typedef struct bbmap_msite {       /* stream.SiteScore, current/stream/SiteScore.java:999-1011 */
    int32_t chrom, strand, start, stop, hits;
    int32_t quickScore, score, slowScore, pairedScore;
    int32_t perfect, semiperfect, rescued;
    int32_t ngaps;                 /* 0 = gaps == null */
    int32_t gaps[BBMSA_MAX_GAPS];
    int32_t match_job;             /* fill whose result (limits, traceback string) this site carries: index into the job log,
                                    * bit 30 set = the gapped log; -1 = none */
    int32_t reserved[2];
} bbmap_msite;                     /* 128 bytes */

#define BBMAP_NSITES_OVERFLOW (-1)
#define BBMAP_NSITES_MATE_OVERFLOW (-2)
#define BBMAP_NSITES_IN_TIER (-3)
#define BBMAP_MAX_SITES_LIMIT 4096

typedef struct bbmap_jobinfo {     /* one entry per fill, parallel to the job / result arrays */
    int32_t read;                  /* read the fill belongs to */
    int32_t seq;                   /* its position in that read's sequence of fillAndScoreLimited calls; -1 = a fill issued ahead
                                    * of time that the sequence turned out not to contain (ignore it) */
    int32_t kind;                  /* 0 scoreSlow fill, 1 scoreSlow wider refill, 2 slowRescue; final stage (realign_new,
                                    * current/align2/TranslateColorspaceRead.java:370, :413, :450, :457): 3 first fill, 4 padded refill,
                                    * 5 third fill, 6 fillUnlimited */
    int32_t site;                  /* list position of the site when the fill was issued */
} bbmap_jobinfo;                   /* 16 bytes */

typedef struct bbmap_config {
    int32_t device;
    int32_t paired;                /* 0: processRead per read; 1: processReadPair, reads 2p and 2p+1 are mates */
    int32_t max_reads;             /* capacity in reads (not pairs) */
    int32_t max_read_len;          /* <= 600 (BBIDX_PROFILE_BBMAP), <= 6016 (BBIDX_PROFILE_PACBIO: maxReadLength() = ALIGN_ROWS - 1 = 6019,
                                    * current/align2/BBMapThreadPacBio.java:28,70; pieces are cut at 6000) */
    int32_t max_sites;             /* per-read capacity of the probe output and of the mapper's site list (<= 4096); reads that
                                    * need more go to the overflow tier */
    float   minRatio;              /* MINIMUM_ALIGNMENT_SCORE_RATIO (0.56) */
    int32_t slowAlignPadding;      /* 4 */
    int32_t slowRescuePadding;     /* 8 */
    int32_t extraPadding;          /* 10 */
    int32_t tipSearchDist;         /* TIP_DELETION_SEARCH_RANGE, 100; 0 switches findTipDeletions off */
    int32_t maxPairDist;           /* 32000 */
    int32_t averagePairDist;       /* INITIAL_AVERAGE_PAIR_DIST, 100 */
    int32_t maxRescueDist;         /* 1200 */
    int32_t maxRescueMismatches;   /* 32 */
    int32_t maxTrimSitesToRetain;  /* 800 */
    int32_t trimList;              /* 1 */
    int32_t doRescue;              /* 1 */
    int32_t alignColumns;          /* BBIndex.ALIGN_COLUMNS, 3000 */
    int32_t clearzone3;            /* PENALIZE_AMBIG ? 800 : 0 */
    int32_t msaMaxColumns;         /* columns of the MSA instance (3000 in the reference): limit of the second DP context */
    int32_t fastCols;              /* column limit of the first DP context, which takes the ordinary windows (0 = 256); wider
                                    * windows and gapped references go to the second context (the "gapped" log) */
    int32_t jobsPerRead;           /* STARTING capacity of the job log = jobsPerRead * max_reads (0 = 3); the logs grow on demand.
                                    * < 0: exactly -jobsPerRead entries in each log to start with (tests of the growth path) */
    int32_t finalStage;            /* 1 (default, BBIDX_PROFILE_BBMAP): the whole of processRead / processReadPair -- after rescue the final
                                    * pairing, the ambiguity policy, genMatchString -> genMatchStringForSite -> realign_new (the fills that
                                    * produce the printed start / stop / score and the match string), clipping and the score penalties;
                                    * 0: stop after the rescue stage (the site lists as scoreSlow and rescue leave them).
                                    * BBIDX_PROFILE_PACBIO defaults to 0: the stage is opt-in there.  1 runs it with the profile's own
                                    * mapping thread, BBMapThreadPacBio.java:497-670 / :1088-1290 (its clearzone steps, no CLEARZONE1e
                                    * block, the fixed CLEARZONE3) and MultiStateAligner9PacBio's points.
                                    * 2: the stage with BBMapThread's tail whatever the profile (the profile's aligner points).  Exists
                                    * for parity tests: the CPU oracle restates BBMapThread's tail only. */
    int32_t reserved[4];           /* [0] != 0: strictly one fill per read and round (no fills ahead of time; for tests)
                                    * [1] overflow tier: reads it can hold per batch (0 = 4096, < 0 = no tier)
                                    * [2] overflow tier: its max_sites (0 = 1024)
                                    * [3] BBIDX_PROFILE_*: which mapper / aligner classes are followed (must equal the index's) */
} bbmap_config;

/* What BBMap prints for a read: stream.Read's mapping fields when processRead / processReadPair return (current/stream/Read.java;
 * set by genMatchString, current/align2/AbstractMapThread.java:946-959, and the policy behind it).  Filled when cfg.finalStage. */
typedef struct bbmap_final {
    int32_t mapped;                /* Read.mapped() */
    int32_t chrom, strand, start, stop;   /* -1, 0, -1, -1 when not mapped */
    int32_t mapScore;
    int32_t paired, ambiguous, perfect, rescued;
    int32_t match_len;             /* length of Read.match (long format: m S N D I X Y C), 0 = null */
    int32_t nsites;                /* sites left in the read's list (the list itself: bbmap_output.sites), or the overflow flags */
    int64_t match_off;             /* byte offset of the string in bbmap_output.final_match (valid when match_len > 0) */
    int32_t reserved[2];
} bbmap_final;                     /* 64 bytes */

typedef struct bbmap_output {      /* device pointers, valid until the next bbmap_map_batch_device / bbmap_destroy */
    const bbmap_msite *sites;      /* n_reads x cap */
    const int32_t *nsites;         /* per read: sites in its list, or BBMAP_NSITES_OVERFLOW (-1: the list did not fit max_sites and
                                    * the overflow tier could not take the read either: not mapped), BBMAP_NSITES_MATE_OVERFLOW
                                    * (-2: its mate's list did not fit), BBMAP_NSITES_IN_TIER (-3: mapped by the overflow tier, see
                                    * bbmap_get_overflow_output) */
    int32_t cap;
    int32_t match_stride, gmatch_stride;
    int32_t reserved;
    int64_t n_jobs, n_gapped_jobs; /* fills in the two logs */
    const bbmsa_job *jobs;   const bbmsa_result *results;  const bbmap_jobinfo *jobinfo;  const uint8_t *match;
    const bbmsa_job *gjobs;  const bbmsa_result *gresults; const bbmap_jobinfo *gjobinfo; const uint8_t *gmatch;
    const bbmsa_gaps *ggaps;
    /* the final alignment stage (cfg.finalStage): one record per read and the pool its match strings live in.  A site that was given a
     * match string of its own refers to it in the same pool: sites[].reserved[0] = byte offset / 4 + 1 (0 = none),
     * reserved[1] & 0x7fffffff = its length (bit 31 is reserved and 0 on output; expanded gaps and long reads make strings longer than
     * 65,535 bytes).  NULL / 0 when the stage is off. */
    const bbmap_final *final;
    const uint8_t *final_match;
    int64_t final_match_bytes;     /* bytes of the pool in use */
    int64_t n_final_fills;         /* fills the stage issued (they are in the two logs, kinds 3..6) */
} bbmap_output;

typedef struct bbmap_stats {
    /* reads_overflowed: reads whose list fitted neither max_sites nor the overflow tier (left unmapped, flagged) */
    int64_t reads, reads_overflowed, reads_without_site, fills, gapped_fills, refills, rescue_scans, rescue_fills, rounds;
    int64_t fills_dropped;         /* fills issued ahead of time that the reference's sequence turned out not to contain (dropped;
                                    * their log entries keep seq = -1) */
    float ms_probe, ms_begin, ms_score, ms_slow, ms_finish, ms_rescue, ms_total;
    float ms_dp_narrow, ms_dp_wave, ms_dp_generic, ms_dp_gapped, ms_quick_rescue;
    int64_t probe_stats[5];        /* bbidx_last_stats of the probe launch */
    int64_t reads_reprobed;        /* reads the overflow tier mapped (pairs count both mates); fills etc. above include the tier's */
    float ms_overflow;             /* the overflow tier's whole pass (included in ms_total) */
    float log_growths;             /* times a fill log had to grow during the batch (the logs start at jobsPerRead entries per read) */
    float ms_dp_wave_max;          /* the longest single wavefront-kernel pass of the plain DP context in the batch (round 1's, as a rule);
                                    * ms_dp_wave is the sum over all rounds and rescue passes */
    float ms_final;                /* the final alignment stage (included in ms_total) */
    int64_t final_fills, final_rounds, final_local;   /* its fills, rounds, reads that went through toLocalAlignment */
    int64_t dp_narrow_launches;    /* DP launches that ran the band kernel (bbmsa_last_route: route8[0]) */
    int64_t dp_sorted_launches;    /* DP launches whose first pass took the jobs widest first (route8[1]) */
    int64_t sites_cross_scaffold;  /* probe sites quickMap's tail removed for spanning two scaffolds (bbidx_set_scaffolds; 0 without a
                                    * table).  The overflow tier's pass adds its own: a pair one of whose mates overflowed the probe is
                                    * counted there only; a read the tier maps again because rescue outgrew its list counts in both. */
} bbmap_stats;

typedef struct bbmap_ctx bbmap_ctx;
int bbmap_default_config(bbmap_config *cfg);
/* bbmap.sh's defaults (BBMap.setDefaults, current/align2/BBMap.java:45-65) or mapPacBio.sh's (BBMapPacBio.setDefaults,
 * current/align2/BBMapPacBio.java:47-69: minRatio 0.46, padding 8 / 16, tip search 15, 7600 columns, single-ended) */
int bbmap_default_config_profile(int32_t profile, bbmap_config *cfg);
/* The context borrows `index` (which must outlive it) and owns two DP contexts (plain and gapped-reference), the overflow tier
 * (a second, small set of the same) and every intermediate buffer.  One batch at a time per context, from one thread at a time; the
 * call itself uses two internal streams and a helper thread (the overflow tier's pass runs beside the main one) and has joined
 * them when it returns.  Two contexts over the same index must not map at the same time (the probe keeps its queue and counters
 * in the index context). */
/* Side effect on the borrowed index context: its quitAfterTwoPerfects tunable is set to !cfg->paired, as BBMap does with the index
 * class's static (`if(paired){BBIndex.QUIT_AFTER_TWO_PERFECTS=false;}`, current/align2/BBMap.java:434). */
int bbmap_create(bbidx_ctx *index, const bbmap_config *cfg, bbmap_ctx **out);
void bbmap_destroy(bbmap_ctx *ctx);
/* AVERAGE_PAIR_DIST for the batches to come.  The reference's mapping threads move it as they see pairs (DYNAMIC_INSERT_LENGTH:
 * `if(numMated>1000 && r.paired()){AVERAGE_PAIR_DIST=(int)(innerLengthSum*1f/numMated);}`, current/align2/BBMapThread.java:1307-1309,
 * per thread); a host that carries that running value sets it here between batches (cfg.averagePairDist is only the initial value,
 * INITIAL_AVERAGE_PAIR_DIST).  It enters pairSiteScoresInitial / Final and the rescue search (:1086, :1093). */
int bbmap_set_average_pair_dist(bbmap_ctx *ctx, int32_t average_pair_dist);
/* Maps a batch that is resident on the device.  reads[i].bases_off addresses the plus strand inside `bases`; the call writes
 * every read's reverse complement at bases_off + minus_delta (also a read's that the probe leaves alone for having no key: rescue
 * may still place it beside its mate).  In paired mode the mates of a pair (reads 2p, 2p + 1) may differ in length.  Enqueues on `stream` and waits for it: the call returns when the
 * batch is done (the rounds of scoreSlow need the job counts on the host). */
int bbmap_map_batch_device(bbmap_ctx *ctx, void *stream, int64_t n_reads, const bbidx_read *reads, uint8_t *bases,
                           int64_t minus_delta, const int8_t *baseScores, const int32_t *keyinfo);
int bbmap_get_output(bbmap_ctx *ctx, bbmap_output *out);
/* The final alignment stage ALONE over site lists the caller provides (a host that runs its own pairing / rescue policy, or a test
 * that wants lists the mapper would rarely produce): sites = n_reads x cfg.max_sites records, nsites[r] = sites of read r, as
 * bbmap_map_batch_device leaves them after rescue with finalStage = 0 (sorted as processRead / processReadPair leave them; scores
 * set).  `bases` holds the plus strands and, at + minus_delta, the reverse complements (the caller's: bbpipe_revcomp_device writes
 * them).  Results as after bbmap_map_batch_device: bbmap_get_output (the two fill logs hold this call's fills only, numbered from
 * 0 per read; sites / nsites are the lists after the stage), bbmap_get_final.  No overflow tier is involved. */
int bbmap_final_batch_device(bbmap_ctx *ctx, void *stream, int64_t n_reads, const bbidx_read *reads, uint8_t *bases, int64_t minus_delta,
                             const bbmap_msite *sites, const int32_t *nsites);
/* Host-buffer form, for a host that owns no device memory (the JNI glue, jni/hip_glue.c: Java cannot allocate HBM).  bases holds the
 * plus strands only (bases_bytes bytes, baseScores the same length; both required).  The call uploads the batch into device
 * buffers the context keeps, maps it as bbmap_map_batch_device does and returns the site lists without their empty slots:
 * read r has nsites_out[r] sites at sites_out[offsets_out[r] ...] -- or nsites_out[r] = BBMAP_NSITES_OVERFLOW /
 * BBMAP_NSITES_MATE_OVERFLOW when even the overflow tier could not hold its list.  offsets_out has n_reads + 1 entries.  Lists
 * the overflow tier produced are appended behind the others.  *total_out = records produced; records beyond sites_cap are not
 * written (call again with a larger array).  The fill logs stay on the device (bbmap_get_output). */
int bbmap_map_batch(bbmap_ctx *ctx, int64_t n_reads, const bbidx_read *reads, const uint8_t *bases, int64_t bases_bytes,
                    const int8_t *baseScores, const int32_t *keyinfo, int64_t keyinfo_ints, int32_t *nsites_out,
                    int64_t *offsets_out, bbmap_msite *sites_out, int64_t sites_cap, int64_t *total_out);
/* The overflow tier's results for the last batch: n_reads = 0 when no read needed it.  Tier read i is read read_ids[i] of the
 * batch (ascending; pairs keep their two mates adjacent); `out` is laid out like the main output with the tier's own cap, and its
 * job logs number the reads 0..n_reads-1 in tier order. */
typedef struct bbmap_overflow_output {
    int64_t n_reads;
    const int32_t *read_ids;       /* device pointer */
    bbmap_output out;
} bbmap_overflow_output;
int bbmap_get_overflow_output(bbmap_ctx *ctx, bbmap_overflow_output *out);
/* The last batch's final records on the host, overflow tier included (a read the tier mapped gets the tier's record): out[n_reads];
 * the match strings are packed into match_out in read order and out[r].match_off is rewritten to the string's offset THERE.
 * *match_bytes = bytes the strings take; strings that do not fit match_cap are not written (call again with a larger buffer).
 * match_out may be NULL (records only).  BBMAP_E_ARG when the context runs without the final stage. */
int bbmap_get_final(bbmap_ctx *ctx, int64_t n_reads, bbmap_final *out, uint8_t *match_out, int64_t match_cap, int64_t *match_bytes);
/* TrimRead.untrim (current/align2/TrimRead.java:415-508) over the last batch, which was mapped from reads that bbtrim_batch_device
 * trimmed: reads_untrimmed / trims are that stage's reads_in / trims (device arrays of n_reads entries; reads_untrimmed must stay in
 * place, it becomes the batch's read array).  For a read with left + right > 0, lt / rt = left / right, swapped on the minus strand
 * of the record (of the site): the final record gets perfect = 0 and, when mapped, start -= lt, stop += rt; its match string becomes
 * lt x 'C' + string + rt x 'C'; every site of its list gets start -= lt, stop += rt with its own strand, perfect = semiperfect = 0
 * and its own string padded the same way.  The overflow tier's records, lists and strings likewise (tier read i = batch read
 * read_ids[i]).  A read with left + right == 0 is untouched.  One divergence: an unmapped record keeps start = stop = -1.
 * The strings grow, so they move: a sizing pass, a device-wide scan, an emit pass (one wavefront per read) into a second pool of the
 * context's, then the pools are swapped -- every string has a new offset afterwards, and strings that shared bytes have copies of
 * their own.  The reverse complements of the full reads are written again at bases_off + minus_delta.  Everything that reads the
 * batch afterwards (bbmap_get_output, bbmap_get_final, bbmap_get_scaffold_records, bbmap_get_sam_records, bbmap_add_coverage,
 * bbmap_add_read_hist) sees the untrimmed reads, as in Java, where those steps come after :521.  calcStatistics runs inside
 * processRead, before untrim: call bbmap_add_run_stats before this, it refuses a batch that has been untrimmed.
 * Enqueues on `stream` and waits for it once per context (the new pool's size).  BBMAP_E_ARG: the context runs without the final
 * stage, no batch has been mapped, or the batch has been untrimmed already. */
int bbmap_untrim_batch_device(bbmap_ctx *ctx, void *stream, const bbidx_read *reads_untrimmed, const bbtrim_rec *trims);
/* SamLine's coordinate block (current/stream/SamLine.java:120-187, :267-268) for every final record of the last batch, overflow tier
 * included: which scaffold a read landed on and where.  A record that still spans two scaffolds (Data.isSingleScaffold) is unmapped and
 * its mate unpaired, as SamLine does.  Unmapped after that rule: scaffold = -1 and every coordinate 0. */
enum { BBMAP_SCAF_MAPPED = 1,          /* mapped after the single-scaffold rule */
       BBMAP_SCAF_PAIRED = 2,          /* paired after it */
       BBMAP_SCAF_INBOUNDS = 4,        /* inbounds: mapped, start >= 0 and stop < scaflen */
       BBMAP_SCAF_SAME_SCAFFOLD = 8 }; /* sameScaf: both mates mapped on the same scaffold */
typedef struct bbmap_scafrec {
    int32_t scaffold;              /* global scaffold number (0-based, FASTA order; see bbidx_set_scaffolds) */
    int32_t start, stop;           /* a1 / b1: the record's start / stop relative to the scaffold's start (0-based; may lie in the pad) */
    int32_t pos, end;              /* pos0 / pos1: 1-based, leading / trailing clips and clipped leading indels removed, pos >= 1,
                                    * end <= scaflen */
    int32_t scaflen;
    int32_t flags;                 /* BBMAP_SCAF_* */
    int32_t reserved;
} bbmap_scafrec;                   /* 32 bytes */
/* Runs the coordinate kernel over the last batch's final records, enqueued on `stream`: *out = a device array of n_reads records
 * (read order), valid once the stream has reached it and until the next batch.  Uses the index's scaffold table as it is now (set it
 * before the batch).  BBMAP_E_ARG when the context runs without the final stage or the index has no scaffold table. */
int bbmap_get_scaffold_records(bbmap_ctx *ctx, void *stream, const bbmap_scafrec **out);
/* The fields of a SAM line for every final record of the last batch: the rest of stream.SamLine's constructor
 * (current/stream/SamLine.java:82-413) behind the coordinate block above -- makeFlag (:2134-2151), the POS / PNEXT / TLEN table and its
 * sign rule (:220-253, :349-354), RNAME / RNEXT (:164, :315), toMapq (:1703-1722), the CIGAR (toCigar14 :679-750, toCigar13 :600-663 and
 * the `len=` / `lenM` shortcut :269-301), the default tags XT:A:R / NM / AM (makeOptionalTags :1481-1549) and MD (makeMdTag :1361-1445).
 * bbmap_get_sam_records / bbmap_get_sam run at the reference's defaults: INTRON_LIMIT = Integer.MAX_VALUE (no `N` operator, no dropped
 * deletion), MAKE_NM_TAG and MAKE_AM_TAG on, every other tag off.  bbmap_get_sam_records_cfg / bbmap_get_sam_cfg take a bbmap_sam_config
 * (below): the intron limit and the tag switches.  Fixed in both: SOFT_CLIP = true, PENALIZE_AMBIG = true; primary alignments only.
 * Strings live in one text blob, packed in read order without gaps: per read its CIGAR, then its MD value (without "MD:Z:"). */
enum { BBMAP_SAM_CIGAR13 = 1,          /* SamLine.VERSION <= 1.3: M instead of = and X (default: 1.4) */
       BBMAP_SAM_MD = 2 };             /* MAKE_MD_TAG (off by default, as in the reference) */
enum { BBMAP_SAM_TAG_XT = 1 };         /* bbmap_samrec.tags bit 0: XT:A:R */
typedef struct bbmap_samrec {
    int32_t flag, mapq;
    int32_t rname;                 /* global scaffold number; -1 = `*` */
    int32_t rnext;                 /* global scaffold number; -1 = `*`, -2 = `=` */
    int32_t pos, pnext, tlen;
    int32_t nm;                    /* -1 = no NM tag */
    int32_t am;                    /* -1 = no AM tag */
    int32_t tags;                  /* BBMAP_SAM_TAG_* */
    int64_t cigar_off;             /* byte offset in the text blob */
    int32_t cigar_len;             /* 0 = `*` */
    int32_t md_len;                /* 0 = no MD tag */
    int64_t md_off;
} bbmap_samrec;                    /* 64 bytes */
/* Runs bbmap_get_scaffold_records and then the SAM kernels (sizing pass, device-wide scan, emit pass) on `stream`: *recs = a device
 * array of n_reads records (read order), *text = the blob; both valid once the stream has reached them and until the next batch.
 * *text_bytes = the blob's size (may be NULL); the call waits for the stream once, between the scan and the emit pass, because that size
 * is also what the blob is allocated by.  The batch's own reads and bases are the ones the context remembers from bbmap_map_batch_device
 * / bbmap_final_batch_device (they must still be in place): the read length enters MAPQ, AM and the shortcut CIGAR, and MD compares
 * an `N` column's read base with the reference.  BBMAP_E_ARG as bbmap_get_scaffold_records (no final stage, no batch, no scaffold
 * table; a table of one scaffold per chromosome is fine), or unknown flag bits. */
int bbmap_get_sam_records(bbmap_ctx *ctx, void *stream, int32_t flags, const bbmap_samrec **recs, const uint8_t **text,
                          int64_t *text_bytes);
/* Host form, mirroring bbmap_get_final: out[n_reads] and the blob (text_out may be NULL: records only).  *text_bytes = bytes the blob
 * takes; when it does not fit text_cap nothing of it is written (call again with a larger buffer).  Two copies, no re-packing. */
int bbmap_get_sam(bbmap_ctx *ctx, int64_t n_reads, int32_t flags, bbmap_samrec *out, uint8_t *text_out, int64_t text_cap,
                  int64_t *text_bytes);
/* The configurable form: `intronlen=`, `xstag=` and the `...tag=t` switches (Parser.java:686-744; the statics at SamLine.java:2400-2422).
 *   intronLimit  SamLine.INTRON_LIMIT (Parser.java:715-717 sets it without a clamp; < 0 is BBMAP_E_ARG here).  One run of `D` meets three
 *                thresholds, all the reference's: count > limit prints `N` instead of `D` (toCigar14 :725 / :738, toCigar13 :641 / :654; the
 *                count is the CIGAR's, without columns inside a soft-clipped stretch), is left out of NM (:1529, :1535) and of MD
 *                (makeMdTag :1380 -- which then never resets `dels`, so every later deletion of that line is left out of MD as well);
 *                count < limit makes the run count against the identity (Read.identityFlat, Read.java:1557); count >= max(limit, 1)
 *                makes it a splice (Read.countErrors, Read.java:2200-2217).
 *   tags         BBMAP_SAM_MAKE_* bits: which optional tags makeOptionalTags (:1481-1684) adds.  NM and AM land in bbmap_samrec as
 *                before; the others in bbmap_samtags.  MD stays in `flags`.  BBMAP_SAM_NO_TAGS: no tag at all, XT and MD included (:1482).
 * Not carried over: SOFT_CLIP = false, PENALIZE_AMBIG = false, secondary lines, the Tophat tags, the custom X1-X7 tags, X0, X9 and RG. */
enum { BBMAP_SAM_MAKE_NM = 1,            /* MAKE_NM_TAG (default on) */
       BBMAP_SAM_MAKE_AM = 2,            /* MAKE_AM_TAG (default on) */
       BBMAP_SAM_MAKE_SM = 4,            /* MAKE_SM_TAG: SM:i:<mapq> (:1548) */
       BBMAP_SAM_MAKE_XM = 8,            /* MAKE_XM_TAG (:1565-1581) */
       BBMAP_SAM_MAKE_XS = 16,           /* MAKE_XS_TAG: XS:A:+/- on a mapped line whose CIGAR holds an N (makeXSTag :1346-1359) */
       BBMAP_SAM_XS_SECONDSTRAND = 32,   /* XS_SECONDSTRAND (`xstag=ss`): inverts XS */
       BBMAP_SAM_MAKE_NH = 64,           /* MAKE_NH_TAG: NH:i:1 (:1599-1605; no secondary output) */
       BBMAP_SAM_MAKE_STOP = 128,        /* MAKE_STOP_TAG: YS:i (makeStopTag :1316-1319) */
       BBMAP_SAM_MAKE_LENGTH = 256,      /* MAKE_LENGTH_TAG: YL:Z:a,b (makeLengthTag :1321-1324) */
       BBMAP_SAM_MAKE_IDENTITY = 512,    /* MAKE_IDENTITY_TAG: YI:f (makeIdentityTag :1326-1330) */
       BBMAP_SAM_MAKE_SCORE = 1024,      /* MAKE_SCORE_TAG: YR:i:<mapScore> (:1613) */
       BBMAP_SAM_MAKE_INSERT = 2048,     /* MAKE_INSERT_TAG: X8:Z:<insertSizeMapped(false)> for a read with a mate (:1615-1619) */
       BBMAP_SAM_MAKE_BOUNDS = 4096,     /* MAKE_BOUNDS_TAG: XB:Z (:1673-1681) */
       BBMAP_SAM_NO_TAGS = 8192 };       /* NO_TAGS */
typedef struct bbmap_sam_config {
    int32_t flags;                 /* BBMAP_SAM_CIGAR13 | BBMAP_SAM_MD */
    int32_t intronLimit;           /* INT32_MAX = none */
    int32_t tags;                  /* BBMAP_SAM_MAKE_* | BBMAP_SAM_XS_SECONDSTRAND | BBMAP_SAM_NO_TAGS */
    int32_t reserved[5];           /* 0 */
} bbmap_sam_config;                /* 32 bytes */
/* flags 0, no intron limit, NM and AM: what bbmap_get_sam_records does. */
int bbmap_sam_default_config(bbmap_sam_config *cfg);
/* The further tags of one line, as values (the host prints them); parallel to bbmap_samrec.  All 0 for an unmapped line (:1483-1484). */
typedef struct bbmap_samtags {
    int32_t present;               /* BBMAP_SAM_MAKE_* bits of SM XM XS NH STOP LENGTH IDENTITY SCORE INSERT BOUNDS: tags this line carries */
    int32_t xs;                    /* +1 / -1 */
    int32_t nh, sm, xm;
    int32_t ys;
    int32_t yl_query, yl_ref;      /* YL:Z:yl_query,yl_ref */
    int32_t yi_good, yi_bad;       /* identityFlat's good / bad after the `n` folding (Read.java:1586-1588): f = good / (float)max(good + bad, 1) */
    int32_t yi_perfect;            /* 1: the line prints YI:f:100 (:1327), good / bad are 0 */
    int32_t yr;
    int32_t x8;
    int32_t xb;                    /* this read's letter I / O / U, and in bits 8-15 the mate's (0 without a mate) */
    int32_t introns;               /* N operators in this line's CIGAR */
    int32_t splices;               /* Read.countErrors(INTRON_LIMIT)[5] (Read.java:2189-2240) of a mapped record with a match string,
                                    * whatever the tag switches: splices > 0 is what readCountSplice1 / 2 count
                                    * (AbstractMapThread.java:1528, :1679), the table's "Splice Rate" line.  Handed out here because
                                    * bbmap_runstats has no room for it. */
} bbmap_samtags;                   /* 64 bytes */
/* bbmap_get_sam_records under a configuration: the same kernels, *tags = a second device array of n_reads records (tags may be NULL:
 * not made).  With bbmap_sam_default_config's values *recs and *text are bbmap_get_sam_records', byte for byte.  BBMAP_E_ARG as there,
 * or intronLimit < 0, or unknown flag / tag bits. */
int bbmap_get_sam_records_cfg(bbmap_ctx *ctx, void *stream, const bbmap_sam_config *cfg, const bbmap_samrec **recs,
                              const bbmap_samtags **tags, const uint8_t **text, int64_t *text_bytes);
/* Host form, mirroring bbmap_get_sam; tags_out may be NULL. */
int bbmap_get_sam_cfg(bbmap_ctx *ctx, int64_t n_reads, const bbmap_sam_config *cfg, bbmap_samrec *out, bbmap_samtags *tags_out,
                      uint8_t *text_out, int64_t text_cap, int64_t *text_bytes);
/* The raw form over device arrays the caller owns: reads (len, bases_off) and `bases` (the reads as they came in), one final record per
 * read with its string in `pool` at match_off, one bbmap_scafrec per read (bbmap_get_scaffold_records' layout; the caller may write it
 * by hand), sites = n_reads x cap records with nsites[r] in use (read for XM only: both may be NULL without BBMAP_SAM_MAKE_XM),
 * chrom_arr[c] / chrom_arr_len[c] = chromosome c's array as ChromosomeArray holds it (device array of device pointers; read for MD only).
 * paired: reads 2p and 2p + 1 are mates.  max_read_len bounds reads[].len (<= 6016).  Outputs: recs, tags (may be NULL), `text` of
 * text_cap bytes, *text_bytes_dev (a device word) = the bytes the blob needs.  When the blob does not fit nothing is written at or behind
 * text_cap, and the records still carry the true lengths and offsets.  workspace: bbpipe_sam_records_workspace_bytes(n_reads,
 * max_read_len) bytes of device memory.  Enqueues the sizing pass, the scan and the emit pass on `stream` and does not wait. */
int64_t bbpipe_sam_records_workspace_bytes(int64_t n_reads, int32_t max_read_len);
int bbpipe_sam_records_device(void *stream, int64_t n_reads, int32_t paired, const bbmap_sam_config *cfg, int32_t max_read_len,
                              const bbidx_read *reads, const uint8_t *bases, const bbmap_final *finals, const uint8_t *pool,
                              const bbmap_scafrec *scaf, const bbmap_msite *sites, const int32_t *nsites, int32_t cap,
                              const uint8_t *const *chrom_arr, const int32_t *chrom_arr_len, bbmap_samrec *recs, bbmap_samtags *tags,
                              uint8_t *text, int64_t text_cap, int64_t *text_bytes_dev, void *workspace, int64_t workspace_bytes);
int bbmap_last_stats(bbmap_ctx *ctx, bbmap_stats *out);

/* =====================================================================================
 * Run statistics and the adaptive state they drive
 *   AbstractMapThread.calcStatistics1 / calcStatistics2 (current/align2/AbstractMapThread.java:1478-1641, :1644-1770; called from
 *   BBMapThread.java:730, :1359-1360) with calcCorrectness (:2615-2689) and Read.countErrors: the counters behind the table BBMap prints
 *   at the end of a run, summed on the device over the final records, the match-string pool and the site lists after the final stage
 *   (run_stats.hip).  Also the insert-size histogram (AbstractMapThread.java:524, ReadStats.addToInsertHistogram(r, false),
 *   current/align2/ReadStats.java:578-592, with Read.insertSizeMapped, current/stream/Read.java:2618-2670): mate 1 of paired pairs,
 *   x = min(MAXINSERTLEN, insert), counted when x > 0, BBMAP_INSERT_HIST_BINS = MAXINSERTLEN + 1 bins (ReadStats.java:1313).
 *   Fixed at the reference's defaults: AMBIGUOUS_TOSS = false, OUTPUT_PAIRED_ONLY = false.  The splice counter (readCountSplice) is left
 *   out: SamLine.INTRON_LIMIT stays at Integer.MAX_VALUE, so it can never move.  The host's: perfectHit (`topScore==maxPossibleQuickScore`)
 *   and lowQualityReadsDiscarded / lowQualityBasesDiscarded need quickMap's return value, which the mapper does not keep; consequently
 *   an unmapped read always counts as noHit.  `elements>0` (a read's list is not empty) selects the mapped branch, as in the reference;
 *   a read flagged BBMAP_NSITES_OVERFLOW / _MATE_OVERFLOW has no list.
 * ===================================================================================== */
enum { BBMAP_INSERT_HIST_BINS = 40001 };
enum { BBMAP_RUNSTATS_MAX_WAVES = 8192 };   /* wavefronts of the statistics kernel's persistent grid (one read per wavefront and turn) */
typedef struct bbmap_runstats {
    /* mate 1: calcStatistics1 (every read of a single-ended run counts as mate 1) */
    int64_t mappedRetained1;                    /* AbstractMapThread.java:1533 / :1683 */
    int64_t mappedRetainedBases1;               /* :1534 / :1684 */
    int64_t ambiguousBestAlignment1;            /* :1484-1485 / :1647-1648 (AMBIGUOUS_TOSS = false: ambiguous and mapped) */
    int64_t ambiguousBestAlignmentBases1;       /* :1486 / :1649 */
    int64_t matchCountM1;                       /* :1517 / :1669; Read.countErrors, current/stream/Read.java:2189-2240: `m` */
    int64_t matchCountS1;                       /* :1518 / :1670: `S` */
    int64_t matchCountD1;                       /* :1519 / :1671: `D` */
    int64_t matchCountI1;                       /* :1520 / :1672: `I`, `X` and `Y` */
    int64_t matchCountN1;                       /* :1521 / :1673: `N` and `C` */
    int64_t readCountS1;                        /* :1523 / :1675 */
    int64_t readCountD1;                        /* :1524 / :1676 */
    int64_t readCountI1;                        /* :1525 / :1677 */
    int64_t readCountN1;                        /* :1527 / :1678 */
    int64_t readCountE1;                        /* :1529 / :1680 */
    int64_t rescuedP1;                          /* :1535-1537 / :1685-1687 */
    int64_t rescuedM1;                          /* :1539 / :1689 */
    int64_t perfectMatch1;                      /* :1565-1566 / :1693-1694: `r.perfect() || (maxSwScore>0 && r.topSite().slowScore==maxSwScore)`, maxSwScore = maxQuality(len) */
    int64_t perfectMatchBases1;                 /* :1567 / :1695 */
    int64_t perfectHitCount1;                   /* :1574-1575 / :1702-1703 */
    int64_t semiPerfectHitCount1;               /* :1578-1579 / :1706-1707 */
    int64_t semiperfectMatch1;                  /* :1583 / :1711 */
    int64_t semiperfectMatchBases1;             /* :1584 / :1712 */
    int64_t siteSum1;                           /* :1605 / :1733 */
    int64_t topSiteSum1;                        /* :1606 / :1734 (calcCorrectness :2645) */
    int64_t uniqueHit1;                         /* :1609 / :1737 */
    int64_t noHit1;                             /* :1639 / :1766 (every unmapped read: see above) */
    int64_t firstSiteCorrectP1;                 /* :1587 / :1715 (calcCorrectness :2663-2666, isCorrectHit :2692-2700) */
    int64_t firstSiteCorrectM1;                 /* :1588 / :1716 */
    int64_t firstSiteCorrectPaired1;            /* :1589 / :1717 */
    int64_t firstSiteCorrectSolo1;              /* :1590 / :1718 */
    int64_t firstSiteCorrectRescued1;           /* :1591 / :1719 */
    int64_t firstSiteIncorrect1;                /* :1593 / :1721 */
    int64_t firstSiteCorrectLoose1;             /* :1600 / :1728 (isCorrectHitLoose :2712-2719 with thresh + 20, :2664) */
    int64_t firstSiteIncorrectLoose1;           /* :1602 / :1730 */
    int64_t truePositiveP1;                     /* :1613 / :1741 */
    int64_t truePositiveM1;                     /* :1614 / :1742 */
    int64_t totalCorrectSites1;                 /* :1615 / :1743 */
    int64_t correctUniqueHit1;                  /* :1619 / :1747 */
    int64_t correctMultiHit1;                   /* :1621 / :1749 */
    int64_t correctLowHit1;                     /* :1624 / :1752 */
    int64_t falsePositive1;                     /* :1629 / :1757 */
    int64_t readsUsed1;                         /* :3029-3030: reads taken from the input */
    int64_t basesUsed1;                         /* :494, :504-505 */
    /* mate 2: calcStatistics2 (every read of a single-ended run counts as mate 1) */
    int64_t mappedRetained2;                    /* AbstractMapThread.java:1533 / :1683 */
    int64_t mappedRetainedBases2;               /* :1534 / :1684 */
    int64_t ambiguousBestAlignment2;            /* :1484-1485 / :1647-1648 (AMBIGUOUS_TOSS = false: ambiguous and mapped) */
    int64_t ambiguousBestAlignmentBases2;       /* :1486 / :1649 */
    int64_t matchCountM2;                       /* :1517 / :1669; Read.countErrors, current/stream/Read.java:2189-2240: `m` */
    int64_t matchCountS2;                       /* :1518 / :1670: `S` */
    int64_t matchCountD2;                       /* :1519 / :1671: `D` */
    int64_t matchCountI2;                       /* :1520 / :1672: `I`, `X` and `Y` */
    int64_t matchCountN2;                       /* :1521 / :1673: `N` and `C` */
    int64_t readCountS2;                        /* :1523 / :1675 */
    int64_t readCountD2;                        /* :1524 / :1676 */
    int64_t readCountI2;                        /* :1525 / :1677 */
    int64_t readCountN2;                        /* :1527 / :1678 */
    int64_t readCountE2;                        /* :1529 / :1680 */
    int64_t rescuedP2;                          /* :1535-1537 / :1685-1687 */
    int64_t rescuedM2;                          /* :1539 / :1689 */
    int64_t perfectMatch2;                      /* :1565-1566 / :1693-1694: `r.perfect() || (maxSwScore>0 && r.topSite().slowScore==maxSwScore)`, maxSwScore = maxQuality(len) */
    int64_t perfectMatchBases2;                 /* :1567 / :1695 */
    int64_t perfectHitCount2;                   /* :1574-1575 / :1702-1703 */
    int64_t semiPerfectHitCount2;               /* :1578-1579 / :1706-1707 */
    int64_t semiperfectMatch2;                  /* :1583 / :1711 */
    int64_t semiperfectMatchBases2;             /* :1584 / :1712 */
    int64_t siteSum2;                           /* :1605 / :1733 */
    int64_t topSiteSum2;                        /* :1606 / :1734 (calcCorrectness :2645) */
    int64_t uniqueHit2;                         /* :1609 / :1737 */
    int64_t noHit2;                             /* :1639 / :1766 (every unmapped read: see above) */
    int64_t firstSiteCorrectP2;                 /* :1587 / :1715 (calcCorrectness :2663-2666, isCorrectHit :2692-2700) */
    int64_t firstSiteCorrectM2;                 /* :1588 / :1716 */
    int64_t firstSiteCorrectPaired2;            /* :1589 / :1717 */
    int64_t firstSiteCorrectSolo2;              /* :1590 / :1718 */
    int64_t firstSiteCorrectRescued2;           /* :1591 / :1719 */
    int64_t firstSiteIncorrect2;                /* :1593 / :1721 */
    int64_t firstSiteCorrectLoose2;             /* :1600 / :1728 (isCorrectHitLoose :2712-2719 with thresh + 20, :2664) */
    int64_t firstSiteIncorrectLoose2;           /* :1602 / :1730 */
    int64_t truePositiveP2;                     /* :1613 / :1741 */
    int64_t truePositiveM2;                     /* :1614 / :1742 */
    int64_t totalCorrectSites2;                 /* :1615 / :1743 */
    int64_t correctUniqueHit2;                  /* :1619 / :1747 */
    int64_t correctMultiHit2;                   /* :1621 / :1749 */
    int64_t correctLowHit2;                     /* :1624 / :1752 */
    int64_t falsePositive2;                     /* :1629 / :1757 */
    int64_t readsUsed2;                         /* :3029-3030: reads taken from the input */
    int64_t basesUsed2;                         /* :494, :504-505 */
    /* pair level, calcStatistics1 */
    int64_t bothUnmapped;                       /* :1490, :1493 */
    int64_t bothUnmappedBases;                  /* :1491, :1494 */
    int64_t numMated;                           /* :1543 */
    int64_t numMatedBases;                      /* :1544: len1 + len2 with `len2=(r2==null ? 0 : r.length())` (:1481), which is mate 1's length: 2 * len1 per pair */
    int64_t badPairs;                           /* :1561 */
    int64_t badPairBases;                       /* :1562: 2 * len1, as numMatedBases */
    int64_t innerLengthSum;                     /* :1557, after the MAX_PAIR_DIST / MIN_PAIR_DIST (-160) clamp of :1555-1556 (:2974-2975) */
    int64_t outerLengthSum;                     /* :1558 */
    int64_t insertSizeSum;                      /* :1559 */
    int64_t reserved;
} bbmap_runstats;                  /* 96 x 8 = 768 bytes */
/* calcCorrectness' `original` for a read: r.originalSite of a synthetic read.  chrom < 0: no truth for that read (site 0 is its own
 * original, :2623-2627). */
typedef struct bbmap_truth { int32_t chrom, strand, start, stop; } bbmap_truth;   /* 16 bytes */
/* The raw form over device arrays the caller owns: reads (len is used), one final record per read with its string in `pool` at
 * match_off, sites = n_reads x cap records with nsites[r] of them in use (<= 0: an empty list).  paired: reads 2p and 2p + 1 are
 * mates.  scheme (BBMSA_SCHEME_*) gives maxQuality(len) for the perfectMatch rule; thresh is calcCorrectness' THRESH (CORRECT_THRESH,
 * current/align2/AbstractMapper.java:2651, default 0); MAX_PAIR_DIST is 32000.  truth: one record per read, or NULL.  counters (device,
 * ADDED to; zero it first) and ihist (device, BBMAP_INSERT_HIST_BINS entries, added to; may be NULL: no histogram).  Enqueues on
 * `stream`. */
int bbpipe_run_stats_device(void *stream, int64_t n_reads, int32_t paired, int32_t scheme, int32_t thresh, const bbidx_read *reads,
                            const bbmap_final *finals, const uint8_t *pool, const bbmap_msite *sites, const int32_t *nsites, int32_t cap,
                            const bbmap_truth *truth, bbmap_runstats *counters, int64_t *ihist);
/* Adds the last batch (bbmap_map_batch_device or bbmap_final_batch_device), overflow tier included, to the context's running counters
 * and histogram; enqueues on `stream`.  truth: a device array of one record per read of the batch, or NULL.  The context's own
 * scoring scheme and cfg.maxPairDist are used, thresh is 0.  BBMAP_E_ARG: the context runs without the final stage, no batch has been
 * mapped, or this batch has been counted already (a second call changes nothing). */
int bbmap_add_run_stats(bbmap_ctx *ctx, void *stream, const bbmap_truth *truth);
/* Waits for the stream of the last accumulation (the only work that writes the counters; not for the whole device) and copies the
 * running counters; ihist_out: BBMAP_INSERT_HIST_BINS entries, or NULL.  That stream must still exist. */
int bbmap_get_run_stats(bbmap_ctx *ctx, bbmap_runstats *out, int64_t *ihist_out);
/* Zeroes counters and histogram behind the last accumulation, on its stream, and waits for that stream (which must still exist). */
int bbmap_reset_run_stats(bbmap_ctx *ctx);
/* The mapper's adaptive state: the two rules of the reference that read these counters.  flags = 0 (default): nothing changes.
 *   BBMAP_ADAPT_INSERT_LENGTH  DYNAMIC_INSERT_LENGTH (current/align2/BBMapThread.java:1307-1309): after a batch that held a paired read,
 *     if numMated > 1000, the average pair distance for the batches to come becomes (int)(innerLengthSum*1f/numMated) -- Java's
 *     arithmetic: long -> float, float division, truncation -- set as bbmap_set_average_pair_dist sets it (the overflow tier follows).
 *     "Held a paired read" is tested as "numMated moved", which is the same thing (numMated counts exactly the pairs whose mate 1 is
 *     paired(), AbstractMapThread.java:1542-1543).  Deviation: inner lengths clamp at -160, so the quotient can be negative and Java
 *     would store it; bbmap_set_average_pair_dist takes no negative distance, so a negative quotient leaves the value as it was.
 *   BBMAP_ADAPT_RESCUE_SKIP    the "mating is not working" return of rescue() (AbstractMapThread.java:1146): a batch starts with
 *     rescue()'s body skipped when `mappedRetained2>1000 && numMated*20L<mappedRetained2` holds on the running counters (the sort,
 *     removeLowQualitySitesPaired and mergeDuplicateSites around the call, BBMapThread.java:1083-1095, still run).
 * With either bit set bbmap_map_batch_device adds the batch to the counters itself at its end, with the array given by
 * bbmap_set_truth for that one batch (else none); an explicit bbmap_add_run_stats for that batch is then refused as a second count.
 * Cost: with BBMAP_ADAPT_RESCUE_SKIP every bbmap_map_batch_device begins by waiting for the stream of the last accumulation and
 * copying the counters back (768 bytes); with BBMAP_ADAPT_INSERT_LENGTH it ends with the same wait and copy on its own stream.
 * The stream of the last accumulation is a handle the caller gave in an earlier call: it must still exist at every later
 * bbmap_map_batch_device under BBMAP_ADAPT_RESCUE_SKIP, bbmap_get_run_stats, bbmap_reset_run_stats and bbmap_get_adaptive_state.
 * Granularity: the reference moves this state pair by pair and per mapping thread; here it moves batch by batch and per context.
 * With batches of one pair the two are the same sequence. */
enum { BBMAP_ADAPT_INSERT_LENGTH = 1, BBMAP_ADAPT_RESCUE_SKIP = 2 };
int bbmap_set_adaptive(bbmap_ctx *ctx, int32_t flags);
/* Truth records (device, one per read) for the NEXT batch's own accumulation under bbmap_set_adaptive; forgotten after that batch,
 * an empty one (n_reads = 0) included. */
int bbmap_set_truth(bbmap_ctx *ctx, const bbmap_truth *truth);
/* averagePairDist as the batches to come will use it; rescueSkipped = 1 when the next batch would start with rescue skipped (the
 * rule on the running counters, BBMAP_ADAPT_RESCUE_SKIP set; waits for the stream of the last accumulation, as bbmap_get_run_stats
 * does).  Either pointer may be NULL. */
int bbmap_get_adaptive_state(bbmap_ctx *ctx, int32_t *averagePairDist, int32_t *rescueSkipped);
/* =====================================================================================
 * Coverage: covstats= / covhist= / basecov= / bincov=
 *   The tail of AbstractMapThread.run (current/align2/AbstractMapThread.java:552-558) feeds every read to a jgi.CoveragePileup
 *   (created in BBMap.java:401-409): CoveragePileup.processRead (current/jgi/CoveragePileup.java:784-813) -> ScaffoldCoordinates.
 *   setFromIndex (current/stream/ScaffoldCoordinates.java:37-56) -> addCoverage (:600-663) / addCoverageIgnoringDeletions (:665-722)
 *   -> CoverageArray2/3.incrementRange (current/dna/CoverageArray2.java:145-164, CoverageArray3.java:155-174).  Here a batch is added
 *   on the device from its final records, match strings and reads (coverage.hip), and a finalize call turns the running state into
 *   what writeStats (:991-1106), writeHist (:1113-1132), writeCoveragePerBase (:1143-1177), writeCoveragePerBaseBinned2 (:1276-1315),
 *   standardDeviation (:1405-1438) and standardDeviationBinned (:1349-1402) read: depths, per-scaffold integers, the depth histogram
 *   and bin sums.  Every figure is an integer; the float columns are the host's (bbmap_amd/coverage.py).
 *   A read counts when it is mapped and Data.isSingleScaffold(chrom, start, stop) holds; its scaffold is
 *   scaffoldIndex(chrom, (start + stop) / 2), start and stop become scaffold-relative and are clamped to [0, length - 1].  Java's
 *   assertions are off in a BBMap run: a record wholly left of its scaffold moves basehits by stop - start + 1 (negative) and no depth.
 *   Flags:
 *     default                       INCLUDE_DELETIONS = true, what bbmap.sh always runs: +1 on [start, stop], basehits += stop - start + 1
 *     BBMAP_COV_START_ONLY          startcov=t: +1 at start only (wins over EXCLUDE_DELETIONS, :626).  A start at or past the scaffold's
 *                                   end adds no depth (Java: the extra slot for start == length, an exception beyond).
 *     BBMAP_COV_EXCLUDE_DELETIONS   the class's delcov=f path (pileup.sh); bbmap.sh's own command line never reaches it, it is opt-in
 *                                   here: the match string is walked from the CLAMPED start, m / S / N cover a base, D skips one,
 *                                   I / X / Y / C do nothing; a record without a string adds the read counters and no depth.
 *     BBMAP_COV_STRANDED            strand-1 reads go to a second array (the per-scaffold read counters are shared, as in writeStats)
 *     BBMAP_COV_32BIT               depths saturate at Integer.MAX_VALUE instead of 65,535, histogram bins 0..1,000,000 instead of
 *                                   0..65,535
 *   Every increment is +1, so saturating at read-out, min(count, cap), equals CoverageArray's cap per increment.
 *   Layout: global scaffold s (FASTA order, as in bbmap_scafrec) owns length[s] + 1 slots at covoff[s] (the class's arrays have
 *   length + 1 elements too; the extra one is always 0 here and takes part in Median_fold and Std_Dev as it does there).
 *   Out of scope: physcov, secondary-site coverage (USE_SECONDARY; BBMap passes secondary=f, BBMap.java:403), bitset mode, normcov /
 *   normcovo, rpkm=, the low-coverage window column (USE_WINDOW), twocolumn, the concise and delta-only basecov forms, and a JNI native
 *   for BBMapHIP.
 * ===================================================================================== */
enum { BBMAP_COV_START_ONLY = 1, BBMAP_COV_EXCLUDE_DELETIONS = 2, BBMAP_COV_STRANDED = 4, BBMAP_COV_32BIT = 8 };
enum { BBMAP_COV_MAX_WAVES = 8192 };        /* wavefronts of the accumulate kernel's persistent grid (one read per wavefront and turn) */
enum { BBMAP_COV_SCAN_TILE = 2048 };        /* slots per workgroup of the prefix sum (tile sums, scan, apply) */
enum { BBMAP_COV_STATS_CHUNK = 65536 };     /* slots per workgroup of the passes that only read the depths: statistics, the long median's counts */
enum { BBMAP_COV_MEDIAN_SHORT = 65536 };    /* scaffolds up to this length take the one-workgroup median, longer ones the many-workgroup one */
enum { BBMAP_COV_HIST_LDS_BINS = 1024 };    /* depths below this are counted in a workgroup's LDS sub-histogram first */
enum { BBMAP_COV_LDS_SCAFFOLDS = 512 };     /* tables of up to this many scaffolds: the accumulate kernel sums a workgroup's per-scaffold counters in LDS */
typedef struct bbmap_covstrand {
    int64_t covered;               /* positions < length with depth > 0 */
    int64_t median;                /* element length / 2 of the length + 1 slots sorted descending (writeStats :1033-1042) */
    int64_t max;
    int64_t sumDepth;              /* over positions < length, of the saturated depths */
    uint64_t sumSqLo, sumSqHi;     /* the same of their squares, a 128-bit integer */
} bbmap_covstrand;                 /* 48 bytes */
typedef struct bbmap_covrec {
    int64_t length;
    int64_t basehits, readhits, readhitsMinus, fraghits;   /* Scaffold's counters (:612-632, :719) */
    int64_t readBases[4];          /* A C G T of the counted reads (basecount[0..3], charToNum: jgi/AssemblyStats2.java:1667-1683) */
    int64_t refBases[4];           /* A C G T of the scaffold's own bases (ChromosomeArray.calcGC, current/dna/ChromosomeArray.java:204-209) */
    bbmap_covstrand strand[2];     /* [1] is filled under BBMAP_COV_STRANDED */
} bbmap_covrec;                    /* 200 bytes */
typedef struct bbmap_covtotals { int64_t readsProcessed, mappedReads, mappedBases, refBases; } bbmap_covtotals;   /* 32 bytes */
typedef struct bbmap_cov_view {    /* device pointers, valid until the next bbmap_cov_finalize, bbmap_reset_coverage or bbmap_destroy */
    int32_t flags, nscaf;
    int32_t binsize, depth_bytes;  /* bytes per depth: 2 (uint16) or 4 (int32) */
    int64_t slots;                 /* covoff[nscaf] */
    int64_t hist_bins;             /* 65,536 or 1,000,001 */
    int64_t nbins;                 /* binoff[nscaf] */
    const int64_t *covoff;         /* [nscaf + 1] */
    const void *depth[2];          /* [slots] each; [1] NULL without BBMAP_COV_STRANDED */
    const bbmap_covrec *recs;      /* [nscaf] */
    const int64_t *hist[2];        /* [hist_bins] each: positions < length of EVERY scaffold by min(depth, hist_bins - 1) (writeStats leaves
                                      out the scaffolds no read touched, whose arrays it never made: the host subtracts their lengths
                                      from bin 0) */
    const int64_t *binoff;         /* [nscaf + 1]: scaffold s has ceil(length / binsize) bins, the last one short */
    const int64_t *bins[2];        /* [nbins] each: sums of the depths of a bin's positions */
    const bbmap_covtotals *totals;
} bbmap_cov_view;
/* Host-side layout arithmetic: covoff (nscaf + 1 entries, covoff[s + 1] = covoff[s] + lengths[s] + 1) and, when binsize > 0 and
 * binoff is given, binoff (nscaf + 1 entries).  Either output may be NULL.  BBMAP_E_ARG: a length < 1, nscaf < 0, binsize < 0. */
int bbpipe_coverage_layout(int32_t nscaf, const int32_t *lengths, int32_t binsize, int64_t *covoff, int64_t *binoff);
/* Bytes of device workspace bbpipe_coverage_finalize_device needs for a table of nscaf scaffolds and `slots` slots (< 0: bad argument). */
int64_t bbpipe_coverage_workspace_bytes(int32_t nscaf, int64_t slots);
/* The raw accumulate over device arrays the caller owns: reads (bases_off and len are used) with their plus-strand `bases`, one
 * final record per read with its string in `pool` at match_off; paired: every read has a mate (fraghits moves by 1, else by 2).  The
 * scaffold table as bbidx_set_scaffolds lays it out: scaf_off[nchroms + 2] (chromosome c's scaffolds are scaf_off[c] .. scaf_off[c + 1],
 * c from 1), scaf_loc / scaf_len by global scaffold number, pad = interScaffoldPadding.  covoff as bbpipe_coverage_layout gives it for
 * scaf_len; diff0 / diff1: int32[slots] difference arrays (diff1 only under BBMAP_COV_STRANDED), recs[nscaf] and totals are ADDED to
 * (zero them first).  A mapped record whose chromosome is not 1..nchroms is not counted.  Enqueues on `stream`. */
int bbpipe_coverage_add_device(void *stream, int64_t n_reads, int32_t paired, int32_t flags, const bbidx_read *reads, const uint8_t *bases,
                               const bbmap_final *finals, const uint8_t *pool, int32_t nchroms, int32_t nscaf, const int32_t *scaf_off,
                               const int32_t *scaf_loc, const int32_t *scaf_len, int32_t pad, const int64_t *covoff, int32_t *diff0,
                               int32_t *diff1, bbmap_covrec *recs, bbmap_covtotals *totals);
/* The raw finalize over the same arrays: a snapshot (the difference arrays and the counters in recs are only read; accumulation may go
 * on afterwards).  Writes depth0 / depth1 (uint16[slots], or int32[slots] under BBMAP_COV_32BIT), length / refBases / strand[] of every
 * record (refgc: int64[nscaf][4], or NULL for zeros), hist0 / hist1 (65,536 or 1,000,001 entries) and, when binsize > 0, bins0 / bins1
 * at binoff.  totals->refBases is set.  workspace: bbpipe_coverage_workspace_bytes.  Enqueues on `stream`. */
int bbpipe_coverage_finalize_device(void *stream, int32_t flags, int32_t nscaf, int64_t slots, const int32_t *scaf_len, const int64_t *covoff,
                                    const int32_t *diff0, const int32_t *diff1, void *depth0, void *depth1, bbmap_covrec *recs,
                                    const int64_t *refgc, int64_t *hist0, int64_t *hist1, int32_t binsize, const int64_t *binoff,
                                    int64_t nbins, int64_t *bins0, int64_t *bins1, bbmap_covtotals *totals, void *workspace,
                                    int64_t workspace_bytes);
/* Allocates the coverage state for the index's scaffold table as it is now (4 + 2 or 4 bytes per slot and strand) and counts the
 * reference's bases per scaffold.  A second call with the same flags over the same table changes nothing.  BBMAP_E_ARG: the context
 * runs without the final stage, the index has no scaffold table, unknown flag bits, or coverage is enabled already with other flags
 * or over a table that bbidx_set_scaffolds has replaced since. */
int bbmap_cov_enable(bbmap_ctx *ctx, int32_t flags);
/* Adds the last batch, overflow tier included; enqueues on `stream`.  BBMAP_E_ARG: coverage is not enabled, no batch has been mapped,
 * this batch has been counted already (a second call changes nothing), or the scaffold table has been replaced. */
int bbmap_add_coverage(bbmap_ctx *ctx, void *stream);
/* Runs the finalize kernels on `stream` behind everything added so far; binsize 0 = no bins.  *out is filled at once, its arrays are
 * complete when `stream` has run. */
int bbmap_cov_finalize(bbmap_ctx *ctx, void *stream, int32_t binsize, bbmap_cov_view *out);
/* Host form: finalizes on the null stream, waits, and copies records (nscaf_cap >= nscaf), totals and histogram(s) (hist_cap entries
 * per strand, all or nothing) always, depths and bins only into buffers that hold them (depth_cap bytes / bins_cap entries per strand;
 * the strands follow each other).  *view_out (optional) reports the sizes that were needed; its pointers are the device's. */
int bbmap_get_coverage(bbmap_ctx *ctx, int32_t binsize, bbmap_covrec *recs_out, int64_t nscaf_cap, bbmap_covtotals *totals_out,
                       int64_t *hist_out, int64_t hist_cap, void *depth_out, int64_t depth_cap, int64_t *bins_out, int64_t bins_cap,
                       bbmap_cov_view *view_out);
/* Zeroes everything accumulated (the reference's base counts stay); waits for the stream of the last accumulation.  The batch the
 * context still holds counts as not added again: a bbmap_add_coverage for it is accepted. */
int bbmap_reset_coverage(bbmap_ctx *ctx);

/* =====================================================================================
 * Read histograms: mhist= / qhist= / bqhist= / qchist= / bhist= / qahist= / ehist= / indelhist= / lhist= / gchist= / idhist=
 *   align2.ReadStats as AbstractMapThread.run feeds it (current/align2/AbstractMapThread.java:478-482 before mapping, :523-529
 *   after it): addToMatchHistogram2 (current/align2/ReadStats.java:516-576), addToQualityAccuracy (:336-387), addToErrorHistogram
 *   (:395-399), addToIndelHistogram (:472-508), addToIdentityHistogram (:446-452, Read.identityFlat, current/stream/Read.java:
 *   1529-1596), addToQualityHistogram2 / addToBQualityHistogram / addToQCountHistogram (:273-328), addToBaseHistogram2 (:648-664),
 *   addToLengthHistogram (:407-411), addToGCHistogram (:413-438, usePairGC, Read.gc :2530-2542).  Accumulated on the device from
 *   the batch's reads, their numeric phred qualities, the final records and their match strings (read_hist.hip); every figure is a
 *   64-bit integer, so the result does not depend on the order of the adds; the float columns and the text are the host's
 *   (bbmap_amd/readstats.py).  `mate` is the read's index within its pair (reads 2p + 1 of a paired batch are mate 1).
 *   One flag bit per COLLECT_* switch of the class; a group that is not selected takes no memory and is not counted.
 *   Stated deviations: a mapped read without a match string takes no part in the match histogram (Java counts its bases as N /
 *   other); the quality-accuracy walk stops when rpos reaches the read's length (Java would throw on a string that overruns its
 *   read) and a quality above 98 counts in bin 98; a quality above 126 counts in bin 126; the error histogram has
 *   BBMAP_RH_MAX_POS + 1 bins and a larger count lands in the last one (Java's list grows); the float sums behind qhist= (qualSum,
 *   qualSumDouble) are not kept, the host derives them from the position x quality table, so BBMAP_RH_QUALITY always keeps that
 *   table.  Reads longer than BBMAP_RH_MAX_POS (the library maps none) are counted up to that position.
 *   Out of scope: aqhist= (a per-read float32 sum in read order through log10: the host holds the qualities it read and can do it
 *   there), timehist=, ihist= (bbmap_get_run_stats' histogram), ID_BINS_AUTO / GC_BINS_AUTO / GC_PLOT_X, the SamLine branches
 *   of pairnum, and JNI natives for BBMapHIP.  With qtrim and untrim=f Java counts qhist / bhist / lhist / gchist on the read BEFORE
 *   trimming (:478-482) while the context holds the trimmed reads: a host that wants those files calls bbpipe_read_hist_add_device
 *   for those groups with the untrimmed read array itself.
 * ===================================================================================== */
enum { BBMAP_RH_MATCH = 1,         /* mhist=: matchSum subSum delSum insSum nSum clipSum otherSum, [7][2][BBMAP_RH_MAXLEN] */
       BBMAP_RH_QUALITY = 2,       /* qhist= / bqhist= / qchist=: qualLength [2][MAXLEN], bqualHist [2][MAXLEN][127], qcountHist [2][127] */
       BBMAP_RH_BASE = 4,          /* bhist=: baseHist [2][5][BBMAP_RH_MAX_POS], slot 0 = N or other, 1-4 = A C G T */
       BBMAP_RH_ACCURACY = 8,      /* qahist=: qualMatch qualSub qualIns qualDel, [4][99] */
       BBMAP_RH_INDEL = 16,        /* indelhist=: insHist [1001], delHist [1000], delHist2 [10001] */
       BBMAP_RH_ERROR = 32,        /* ehist=: [BBMAP_RH_MAX_POS + 1] */
       BBMAP_RH_LENGTH = 64,       /* lhist=: [BBMAP_RH_MAX_POS + 1] */
       BBMAP_RH_GC = 128,          /* gchist=: gcHist [101], then gcMaxReadLen */
       BBMAP_RH_IDENTITY = 256,    /* idhist=: idHist [101], idBaseHist [101], then idMaxReadLen */
       BBMAP_RH_ALL = 511 };
enum { BBMAP_RH_MAXLEN = 6000, BBMAP_RH_MAXINSLEN = 1000, BBMAP_RH_MAXDELLEN = 1000, BBMAP_RH_MAXDELLEN2 = 1000000, BBMAP_RH_GC_BINS = 100,
       BBMAP_RH_ID_BINS = 100 };   /* ReadStats.java:1312-1321 */
enum { BBMAP_RH_MAX_POS = 6016 };          /* the library's longest read (BBIDX_PACBIO_MAX_READ_LEN): positions of bhist, bins of lhist / ehist */
enum { BBMAP_RH_QUAL_BINS = 127, BBMAP_RH_ACC_BINS = 99, BBMAP_RH_DEL2_BINS = BBMAP_RH_MAXDELLEN2 / 100 + 1 };
/* the accumulate kernel's tiles: what a workgroup counts in its LDS (32-bit counters) before it adds to the state */
enum { BBMAP_RH_MAX_BLOCKS = 256 };        /* workgroups of the persistent grid (16 wavefronts each, one pair or single read per wavefront and turn) */
enum { BBMAP_RH_CHUNK_UNITS = 2048 };      /* pairs (single reads) a workgroup counts between two flushes of its LDS counters */
enum { BBMAP_RH_POS_TILE = 256 };          /* positions below this: the per-position arrays of mhist / bhist / qualLength / bqualHist */
enum { BBMAP_RH_QUAL_TILE = 44 };          /* qualities below this (and positions below the tile): bqualHist's LDS sub-table */
enum { BBMAP_RH_ERR_LDS_BINS = 256, BBMAP_RH_LEN_LDS_BINS = 512, BBMAP_RH_DEL2_LDS_BINS = 64 };
typedef struct bbmap_readhist_view {       /* device pointers into one block of `words` int64; NULL for a group that is not selected */
    int32_t flags, reserved;
    int64_t words;
    const int64_t *state;                  /* the block: every pointer below is state + an offset that depends on flags only */
    const int64_t *match;                  /* [7][2][MAXLEN]: match, sub, del, ins, N, clip, other */
    const int64_t *qual_length;            /* [2][MAXLEN]: reads by min(len, MAXLEN) - 1 (the writer turns it into a suffix sum) */
    const int64_t *bqual;                  /* [2][MAXLEN][127] */
    const int64_t *qcount;                 /* [2][127], over ALL bases of a read */
    const int64_t *base;                   /* [2][5][MAX_POS] */
    const int64_t *accuracy;               /* [4][99]: match, sub, ins, del */
    const int64_t *ins, *del, *del2;       /* [1001], [1000], [10001] */
    const int64_t *error;                  /* [MAX_POS + 1] */
    const int64_t *length;                 /* [MAX_POS + 1] */
    const int64_t *gc;                     /* [101], then gcMaxReadLen (0 = nothing counted; the class starts at 1) */
    const int64_t *identity;               /* idHist [101], idBaseHist [101], then idMaxReadLen */
} bbmap_readhist_view;
/* Bytes of the state for these groups (< 0: unknown flag bits). */
int64_t bbpipe_read_hist_bytes(int32_t flags);
/* Where the arrays of a state block lie (pure arithmetic, no device call). */
int bbpipe_read_hist_view(int32_t flags, const void *state, bbmap_readhist_view *out);
/* The raw form over device arrays the caller owns: reads (bases_off, len), the bases blob in plus-strand form, quality laid out like
 * bases (numeric phred, one byte per base) or NULL (the quality-dependent histograms then do not move), one final record per read
 * with its long-format string in `pool` at match_off.  paired: reads 2p and 2p + 1 are mates.  ADDS to `state`
 * (bbpipe_read_hist_bytes(flags) bytes; zero it first).  Enqueues on `stream`. */
int bbpipe_read_hist_add_device(void *stream, int64_t n_reads, int32_t paired, int32_t flags, const bbidx_read *reads, const uint8_t *bases,
                                const uint8_t *quality, const bbmap_final *finals, const uint8_t *pool, void *state);
/* Allocates the zeroed state.  A second call with the same flags changes nothing.  BBMAP_E_ARG: the context runs without the final
 * stage, unknown flag bits or none, or the histograms are enabled already with other flags. */
int bbmap_hist_enable(bbmap_ctx *ctx, int32_t flags);
/* Adds the last batch, overflow tier included; enqueues on `stream`.  quality: a device array laid out like the batch's bases, or
 * NULL.  BBMAP_E_ARG: not enabled, no batch has been mapped, or this batch has been added already. */
int bbmap_add_read_hist(bbmap_ctx *ctx, void *stream, const uint8_t *quality);
/* The state as it is on the device (not synchronised: order your reads behind the stream of the last accumulation). */
int bbmap_get_read_hist_view(bbmap_ctx *ctx, bbmap_readhist_view *out);
/* Host copy: waits for the stream of the last accumulation (which must still exist) and copies the block into out (cap_words int64;
 * nothing is copied into a buffer that is too small).  *view_out (optional): the device view; an array's offset in `out` is its
 * pointer minus view_out->state. */
int bbmap_get_read_hist(bbmap_ctx *ctx, int64_t *out, int64_t cap_words, bbmap_readhist_view *view_out);
/* Zeroes the state behind the last accumulation, on its stream, and waits for that stream.  The batch the context still holds
 * counts as not added again.  Only the stream of the LAST add is known: adds between two resets (and before a host copy) go on
 * one stream, or the caller orders them. */
int bbmap_reset_read_hist(bbmap_ctx *ctx);

/* =====================================================================================
 * Reference-set binning: scafstats= / refstats= and the stream assignment of bbsplit.sh
 *   align2.BBSplitter.printReads as AbstractMapThread.writeList calls it (current/align2/AbstractMapThread.java:608-610) on lists
 *   that capSiteList has cut to MAX_SITESCORES_TO_PRINT sites (:496, :510-511, :1309-1315; 5 in BBMap.java:62, 100 in
 *   BBMapPacBio.java:65): printReadsAndProcessAmbiguous (current/align2/BBSplitter.java:641-757), addToScafCounts (:782-820),
 *   getSets (:824-864), getScaffolds (:867-933), toListNames (:1033-1048).  The scaffold of a read or a site is
 *   Data.scaffoldIndex(chrom, (start + stop) / 2) (current/stream/Read.java:3304-3316, current/stream/SiteScore.java:367-377,
 *   current/dna/Data.java:1091-1108); no single-scaffold rule applies and a read is mapped when bbmap_final.mapped says so.
 *   Names stay with the host (bbmap_amd/refsplit.py): it turns the scaffold names `sets$name` into one 64-bit mask of reference sets
 *   per scaffold (scaf_sets; several bits for a comma-separated prefix) and one key index per scaffold (scaf_key; scaffolds whose
 *   names share the part behind the first `$` share a key, :882-887).  Sets of names become ORs of masks, containsAll / equals
 *   become mask arithmetic.  At most 64 reference sets (BBMAP_SPLIT_MAX_SETS): more are refused with BBMAP_E_ARG.
 *   The device's site lists are not truncated: the stage looks at the first min(nsites, maxSites) entries of a list.
 *   A mapped, ambiguous read whose list is empty cannot occur in the reference (the cap is at least 1); here it yields no key and
 *   no set.  A scaffold or chromosome number outside the tables yields none either.
 *   Out of scope: AMBIGUOUS2_RANDOM (the reference throws, :694-695; refused here), more than 64 sets, BBSplit's reference merging
 *   and its file streams, bamscript=.  The text of the two files is the host's (scafstats_lines / refstats_lines restate
 *   printCounts, :1157-1189).
 * ===================================================================================== */
enum { BBMAP_SPLIT_SCAF_STATS = 1, /* the per-key counters (scafstats=) */
       BBMAP_SPLIT_SET_STATS = 2,  /* the per-set counters (refstats=) */
       BBMAP_SPLIT_RECORDS = 4,    /* one bbmap_splitrec per read */
       BBMAP_SPLIT_LISTS = 8,      /* the stream lists (they are built from the records) */
       BBMAP_SPLIT_ALL = 15 };
enum { BBMAP_AMBIG2_UNSET = 0, BBMAP_AMBIG2_FIRST = 1, BBMAP_AMBIG2_SPLIT = 2, BBMAP_AMBIG2_TOSS = 3, BBMAP_AMBIG2_RANDOM = 4,
       BBMAP_AMBIG2_ALL = 5 };     /* BBSplitter.java:1203-1208 */
enum { BBMAP_SPLIT_MAX_SETS = 64 };
/* the assign kernel's tiles: a workgroup (256 lanes, one read per lane) combines equal keys in an open-addressed LDS table of
 * BBMAP_SPLIT_LDS_SLOTS slots (key -> four 64-bit partial sums; slot of a key = ((uint32)key * 2654435761u) >> 22, linear probing,
 * at most BBMAP_SPLIT_MAX_PROBES slots are tried, then the add goes to the state directly) and adds every slot that moved to the state
 * once per chunk of BBMAP_SPLIT_CHUNK_READS reads */
enum { BBMAP_SPLIT_LDS_SLOTS = 1024, BBMAP_SPLIT_MAX_PROBES = 8, BBMAP_SPLIT_CHUNK_READS = 4096, BBMAP_SPLIT_MAX_BLOCKS = 1024 };
enum { BBMAP_SPLIT_LIST_BLOCK = 256 };     /* units per workgroup of the two list passes */
typedef struct bbmap_split_config {
    int32_t flags;                 /* BBMAP_SPLIT_* */
    int32_t ambiguous2;            /* BBMAP_AMBIG2_* */
    int32_t clearzone;             /* CLEARZONE1() of the mapping thread (BBMapThread.java:78,114,124: 200; BBMapThreadPacBio.java:75,111,121:
                                    * 220); bbmap_split_enable: 0 = the context's own */
    int32_t maxSites;              /* MAX_SITESCORES_TO_PRINT, >= 1; bbmap_split_enable: 0 = the profile's (5 / 100) */
    int32_t nsets;                 /* 0 .. 64 (0: no prefixes, no sets) */
    int32_t nkeys;                 /* >= 0 */
    int32_t reserved[2];
} bbmap_split_config;              /* 32 bytes */
enum { BBMAP_SPLITREC_AMBIG_SETS = 1,      /* the read (pair) is ambiguous between reference sets (:661-663) */
       BBMAP_SPLITREC_AMBIG_READ = 2,      /* the read counts in scafstats' ambiguous columns (mapped and Read.ambiguous()) */
       BBMAP_SPLITREC_MAPPED = 4 };
typedef struct bbmap_splitrec {    /* the mates of a pair carry the same three masks */
    uint64_t primary_mask;         /* sets whose stream the read (pair) goes to (splitTable, :701-710) */
    uint64_t ambig_mask;           /* sets whose AMBIGUOUS stream it goes to (splitTableA, :712-721; only AMBIG2_SPLIT fills it) */
    int32_t flags;                 /* BBMAP_SPLITREC_* */
    int32_t key;                   /* key of the scaffold of the read's own record, -1 = not mapped (or outside the tables) */
    uint64_t stats_mask;           /* sets whose refstats counters the read (pair) moved (:723-754), whether or not they are kept */
} bbmap_splitrec;                  /* 32 bytes */
/* The counter state: int64 words -- [0] totalReads (readsUsed1 + readsUsed2, AbstractMapper.java:1858-1862: every add puts its n_reads
 * there), [1..3] zero, then per key and then per set four words: unambiguous reads, unambiguous bases, ambiguous reads, ambiguous
 * bases (SetCount.mappedReads / mappedBases / ambiguousReads / ambiguousBases, :1149-1153). */
enum { BBMAP_SPLIT_STATE_HEAD = 4 };
/* Bytes of the state (< 0: bad argument). */
int64_t bbpipe_refsplit_state_bytes(int32_t nkeys, int32_t nsets);
/* The raw form over device arrays the caller owns: reads (len is used), one final record per read, site lists of cap_stride
 * records per read with nsites[r] entries in use (a negative count is an empty list; BBMAP_NSITES_OVERFLOW / _MATE_OVERFLOW: the read is
 * not mapped whatever its record says), the scaffold table as bbidx_set_scaffolds lays it out (see bbpipe_coverage_add_device),
 * scaf_sets / scaf_key by global scaffold number (key indices outside 0 .. nkeys - 1 and set bits from nsets up are ignored).
 * paired: reads 2p and 2p + 1 are mates.  ADDS to `state` (zero it first; may be NULL without the two STATS flags); writes
 * records_out[n_reads] (may be NULL without BBMAP_SPLIT_RECORDS / _LISTS).  BBMAP_E_ARG: unknown flag bits, AMBIG2_RANDOM or an unknown
 * mode, nsets > 64, maxSites < 1.  Enqueues on `stream`. */
int bbpipe_refsplit_add_device(void *stream, int64_t n_reads, int32_t paired, const bbmap_split_config *cfg, const bbidx_read *reads,
                               const bbmap_final *finals, const bbmap_msite *sites, const int32_t *nsites, int32_t cap_stride,
                               int32_t nchroms, const int32_t *scaf_off, const int32_t *scaf_loc, int32_t pad, const uint64_t *scaf_sets,
                               const int32_t *scaf_key, void *state, bbmap_splitrec *records_out);
/* The stream lists of a batch from its records: a CSR table of 2 x nsets rows, rows 0 .. nsets - 1 the sets' streams (primary_mask),
 * rows nsets .. 2 nsets - 1 their ambiguous streams (ambig_mask).  set_off[2 nsets + 1] (int64), units[set_off[row] .. set_off[row + 1])
 * = the units of that row in read-list order (strictly ascending); a unit is named by the index of its read, a pair by that of its
 * first mate (r1, :708 / :719).  A stable partition without atomics: per-workgroup counts, a device-wide scan, a placing pass.
 * Entries beyond units_cap are not written (compare set_off[2 nsets] with units_cap).  Enqueues on `stream`. */
int64_t bbpipe_refsplit_lists_workspace_bytes(int64_t n_reads, int32_t paired, int32_t nsets);
int bbpipe_refsplit_lists_device(void *stream, int64_t n_reads, int32_t paired, int32_t nsets, const bbmap_splitrec *records, void *workspace,
                                 int64_t workspace_bytes, int64_t *set_off, int32_t *units, int64_t units_cap);
/* Allocates the zeroed state for the index's scaffold table as it is now.  scaf_sets / scaf_key: HOST arrays, one entry per scaffold
 * (global number).  cfg->clearzone == 0 / cfg->maxSites == 0 select the context's own.  A second call with the same configuration and
 * tables' generation changes nothing.  BBMAP_E_ARG: the context runs without the final stage, the index has no scaffold table, a bad
 * configuration (as above), or the stage is enabled already with another configuration. */
int bbmap_split_enable(bbmap_ctx *ctx, const bbmap_split_config *cfg, const uint64_t *scaf_sets, const int32_t *scaf_key);
/* Adds the last batch, overflow tier included (a read the tier mapped takes the tier's record and list), with the batch's current read
 * lengths; enqueues on `stream`.  BBMAP_E_ARG: not enabled, no batch has been mapped, this batch has been added already, or the
 * scaffold table has been replaced. */
int bbmap_add_split(bbmap_ctx *ctx, void *stream);
/* Device pointer to the records of the last batch added (n_reads of them; valid until the next add).  BBMAP_E_ARG without
 * BBMAP_SPLIT_RECORDS or before the first add. */
int bbmap_get_split_records(bbmap_ctx *ctx, const bbmap_splitrec **out);
/* The stream lists of the last batch added, built on `stream` (the call waits for it once: the total sizes the unit array): device
 * views, valid until the next add or call.  BBMAP_E_ARG without BBMAP_SPLIT_LISTS or before the first add. */
int bbmap_get_split_lists_device(bbmap_ctx *ctx, void *stream, const int64_t **set_off, const int32_t **units, int64_t *total);
/* Host form (null stream): set_off_out[2 nsets + 1] always, the units only into a buffer that holds them; *total_out = units. */
int bbmap_get_split_lists(bbmap_ctx *ctx, int64_t *set_off_out, int32_t *units_out, int64_t units_cap, int64_t *total_out);
/* Host copy of the state (cap_words >= 4 + 4 nkeys + 4 nsets, else BBMAP_E_ARG); waits for the stream of the last add. */
int bbmap_get_split_stats(bbmap_ctx *ctx, int64_t *out, int64_t cap_words);
/* Zeroes the state behind the last add and waits.  The batch the context still holds counts as not added again. */
int bbmap_reset_split(bbmap_ctx *ctx);

/* The last batch's site lists without their empty slots, for a host that copies them back: counts (n_reads + 1 ints), offsets
 * (n_reads + 1 int64: exclusive prefix sums, offsets[n_reads] = total) and packed (packed_cap records) are device buffers of the
 * caller's; read r's counts[r] sites are packed[offsets[r] ...] (0 for a read without a list, a flagged one, or one the overflow
 * tier mapped).  Enqueues on `stream`; records beyond packed_cap are not written (compare offsets[n_reads] with packed_cap). */
int bbmap_pack_sites_device(bbmap_ctx *ctx, void *stream, int64_t n_reads, int32_t *counts, int64_t *offsets, bbmap_msite *packed,
                            int64_t packed_cap);
/* synchronous device-to-host copy of (part of) an output array */
int bbmap_copy_to_host(void *dst, const void *src_device, int64_t bytes);

/* device tables of an index context: chromArr[c] (device pointer to chromosome c's bytes), chromArrLen[c]; host copies */
int bbidx_get_chrom_table(bbidx_ctx *ctx, int32_t *nchroms, const uint8_t **chromArr_host_copy, int32_t *chromArrLen_host_copy, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
