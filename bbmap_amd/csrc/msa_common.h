// Shared constants/types for the MultiStateAligner11ts HIP kernels (gfx950).
// Score/time cell encoding and point values follow jni/MultiStateAligner11tsJNI.c:18-98.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bbmap_amd.h"

namespace bbmsa {

constexpr int kScoreOffset = 11;
constexpr int kTimeMask = 0x7FF;
constexpr int kScoreMask = (int)0xFFFFF800;
constexpr int kMaxTime = 2047;

#define BBMSA_PT(x) ((x) * 2048)
constexpr int P_MATCH = BBMSA_PT(70), P_MATCH2 = BBMSA_PT(100);
constexpr int P_SUB = BBMSA_PT(-127), P_SUBR = BBMSA_PT(-147), P_SUB2 = BBMSA_PT(-51), P_SUB3 = BBMSA_PT(-25);
constexpr int P_INS = BBMSA_PT(-395), P_INS2 = BBMSA_PT(-39), P_INS3 = BBMSA_PT(-23), P_INS4 = BBMSA_PT(-8);
constexpr int P_DEL = BBMSA_PT(-472), P_DEL2 = BBMSA_PT(-33), P_DEL3 = BBMSA_PT(-9), P_DEL4 = BBMSA_PT(-1),
              P_DEL5 = BBMSA_PT(-1);
constexpr int P_DEL_REF_N = BBMSA_PT(-10), P_GAP = BBMSA_PT(-2);
constexpr int kBadOff = (-(((1 << 20) - 1) - 2000) - 1) * 2048;   // BADoff
constexpr int kMinOffScore = (-(((1 << 20) - 1) - 2000)) * 2048;  // MINoff_SCORE
constexpr int kNegInf = -(1 << 30);   // "no limit" for the unlimited fill; never reached by any score
constexpr int kGapLen = 128;

constexpr int kTableLen = 3072;       // upper bound of the delC / insC LDS tables: index time (<2048) + rows (<=640)
// A context's tables only need min(longer side + 2, 2048) + maxRows + 8 entries: a streak (time) never exceeds the longer
// matrix side + 1 (and is clamped below 2048), the "still needed" indel length never exceeds the rows.  Ints of LDS in front of the per-job areas:
__host__ __device__ inline int lds_table_ints(int tableLen) { return 2 * tableLen + 320; }   // + delExt[128], insExt[32], subExt[8] (padded to 192), mTab[32][4]

// Ints of LDS one job of the wavefront kernel takes behind the tables: horizLimit + ONE per column (an int), the window's reference
// bytes (one byte per column; until round 4 an int2 per column held both: 8 bytes, which kept the second DP context's 640-column
// jobs at two blocks per CU) and the reversed match string.
__host__ __device__ inline int lds_job_ints(int fastCols, int tmpBytes) { return (fastCols + 2) + ((fastCols + 2 + 3) >> 2) + ((tmpBytes + 3) >> 2); }

// closed forms of calcDelScoreOffset (jni/...c:316-336) and of the cumulative
// POINTSoff_INS_ARRAY_C table (MultiStateAligner11tsJNI.java:1582-1601)
__host__ __device__ inline int calc_del_off(int len) {
    if (len <= 0) return 0;
    int s = P_DEL;
    if (len > 80) { s += ((len - 80 + 3) / 4) * P_DEL5; len = 80; }
    if (len > 20) { s += (len - 20) * P_DEL4; len = 20; }
    if (len > 5) { s += (len - 5) * P_DEL3; len = 5; }
    if (len > 1) s += (len - 1) * P_DEL2;
    return s;
}
__host__ __device__ inline int calc_ins_cum_off(int len) {
    if (len <= 0) return 0;
    long long s = P_INS;
    int n = len;
    if (n > 20) { s += (long long)(n - 20) * P_INS4; n = 20; }
    if (n > 5) { s += (long long)(n - 5) * P_INS3; n = 5; }
    if (n > 1) s += (long long)(n - 1) * P_INS2;
    return s < kMinOffScore ? kMinOffScore : (int)s;
}

// dna/AminoAcid.java:614-624 + :365-367: A,C,G,T,U in either case are "fully defined".
__host__ __device__ inline bool fully_defined(int b) {
    const int u = b & ~32;   // fold case
    return b < 128 && (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U');
}

// ---- scoring schemes.  The wavefront and band kernels are written for the 11ts constants above; the generic kernel is
// a template over one of these, so that the PacBio parameter set runs through the same literal statement.
struct Scheme11ts {      // jni/MultiStateAligner11tsJNI.c:18-98
    static constexpr int OFF = kScoreOffset, TMASK = kTimeMask, SMASK = kScoreMask, MAXT = kMaxTime;
    static constexpr int MATCH = P_MATCH, MATCH2 = P_MATCH2, SUB = P_SUB, SUBR = P_SUBR, SUB2 = P_SUB2, SUB3 = P_SUB3;
    static constexpr int INS = P_INS, INS2 = P_INS2, INS3 = P_INS3, INS4 = P_INS4;
    static constexpr int DEL = P_DEL, DEL2 = P_DEL2, DEL3 = P_DEL3, DEL4 = P_DEL4, DEL5 = P_DEL5;
    static constexpr int DEL_REF_N = P_DEL_REF_N, GAP = P_GAP;
    static constexpr int BAR_I1 = 2, BAR_D1 = 3;
    static constexpr int BADOFF = kBadOff;
    __host__ __device__ static inline int del_off(int len) { return calc_del_off(len); }
    __host__ __device__ static inline int ins_cum_off(int len) { return calc_ins_cum_off(len); }
    __host__ __device__ static inline int col0(int row) { return calc_ins_cum_off(row); }   // ...JNI.java:101-112
};
struct Scheme9PacBio {   // current/align2/MultiStateAligner9PacBio.java:2359-2439
    static constexpr int OFF = 9, TMASK = 0x1FF, SMASK = (int)0xFFFFFE00, MAXT = 511;
#define BBMSA_PB(x) ((x) * 512)
    static constexpr int MATCH = BBMSA_PB(90), MATCH2 = BBMSA_PB(100);
    static constexpr int SUB = BBMSA_PB(-137), SUBR = BBMSA_PB(-157), SUB2 = BBMSA_PB(-49), SUB3 = BBMSA_PB(-25);
    static constexpr int INS = BBMSA_PB(-205), INS2 = BBMSA_PB(-42), INS3 = BBMSA_PB(-23), INS4 = BBMSA_PB(-8);
    static constexpr int DEL = BBMSA_PB(-292), DEL2 = BBMSA_PB(-37), DEL3 = BBMSA_PB(-17), DEL4 = BBMSA_PB(-2), DEL5 = BBMSA_PB(-1);
    static constexpr int DEL_REF_N = BBMSA_PB(-10), GAP = BBMSA_PB(-2);
    static constexpr int BAR_I1 = 1, BAR_D1 = 1;
    static constexpr int BADOFF = (-(((1 << 22) - 1) - 2000) - 1) * 512;
#undef BBMSA_PB
    __host__ __device__ static inline int del_off(int len) {            // calcDelScoreOffset, ...9PacBio.java:2254-2275
        if (len <= 0) return 0;
        int s = DEL;
        if (len > 80) { s += ((len - 80 + 3) / 4) * DEL5; len = 80; }
        if (len > 20) { s += (len - 20) * DEL4; len = 20; }
        if (len > 5) { s += (len - 5) * DEL3; len = 5; }
        if (len > 1) s += (len - 1) * DEL2;
        return s;
    }
    __host__ __device__ static inline int ins_cum_off(int len) {        // calcInsScoreOffset, :2295-2310
        if (len <= 0) return 0;
        int s = INS;
        if (len > 20) { s += (len - 20) * INS4; len = 20; }
        if (len > 5) { s += (len - 5) * INS3; len = 5; }
        if (len > 1) s += (len - 1) * INS2;
        return s;
    }
    // column 0 as the constructor fills it (:91-98): its tiers switch at row 5 and row 20, one row earlier than
    // calcInsScoreOffset's, so it is its own closed form
    __host__ __device__ static inline int col0(int row) {
        if (row <= 0) return 0;
        int s = INS;
        if (row >= 20) { s += (row - 19) * INS4; row = 19; }
        if (row >= 5) { s += (row - 4) * INS3; row = 4; }
        if (row >= 2) s += (row - 1) * INS2;
        return s;
    }
};

// Which fill a job gets.  halfband: jni/...c:392-393 (0 = the context has no band).
__host__ __device__ inline int fill_halfband(int rows, int columns, int bandwidth, float bandwidthRatio) {
    if (bandwidth < 1 && bandwidthRatio <= 0.0f) return 0;
    const int bwA = bandwidth < 1 ? 9999999 : bandwidth;
    const int bwB = bandwidthRatio <= 0.0f ? 9999999 : 8 + (int)((float)rows * bandwidthRatio);     // (one rounded multiply: nothing to contract)
    return max(min(bwA, bwB), columns - rows + 8) / 2;
}
// The raw modes say it themselves; BBMSA_FILL_LIMITED goes through MSA.fillLimited's gate (MultiStateAligner11tsJNI.java:137-144),
// which turns a fill into fillUnlimited when there is no score to prune by, when the matrix is tiny, or when the window is much
// wider than the read and no band narrows it.  (A limited fill of that mode runs with minScore - 120: the caller's business.)
// `columns` is the clamped window's.  The wavefront kernel and the width sort in front of it share this; the band, generic and strip
// kernels have their own copies.
__host__ __device__ inline bool fill_is_limited(int flags, int minScore, int rows, int columns, int halfband) {
    const int mode = flags & BBMSA_MODE_MASK;
    if (mode == BBMSA_FILL_UNLIMITED_RAW) return false;
    if (mode == BBMSA_FILL_LIMITED_RAW) return true;
    return !(minScore < 1 || (columns + rows < 90) ||
             ((halfband < 1 || halfband * 3 > columns) && (columns > rows + min(170, rows + 20))));
}

// The band kernel's candidate rule (msa_fill_band.hip), shared with the width sort in front of it (msa_sort.hip), which gives the
// candidates a list of their own: a limited fill (through the Java gate for BBMSA_FILL_LIMITED, which then runs with
// minScore - 120) of a shape the band kernel accepts, whose slack maxQuality(rows) - minScore is at most maxSlack points.
// `columns` is the clamped window's; the context has no band (halfband == 0).  A candidate is always a limited fill.
__host__ __device__ inline bool band_is_candidate(int flags, int minScore, int rows, int columns, int maxRows, int maxColumns, int bandRows, int maxSlack) {
    const int mode = flags & BBMSA_MODE_MASK;
    if (!(rows >= 16 && columns >= rows && rows <= maxRows && rows <= bandRows && columns <= maxColumns && mode != BBMSA_FILL_UNLIMITED_RAW)) return false;
    int tmin = minScore;
    if (mode == BBMSA_FILL_LIMITED) {                         // the Java gate, MultiStateAligner11tsJNI.java:137-144 (halfband == 0)
        if (tmin < 1 || (columns + rows < 90) || (columns > rows + min(170, rows + 20))) return false;
        tmin -= 120;
    }
    // candidates are chosen by slack alone; no tighter bound is ever substituted (tests/test_oracle_final.py)
    return (70 + 100 * (rows - 1)) - tmin <= maxSlack;
}

// number of jobs of a launch: a host value, or a counter a previous kernel of the same stream left on the device
__device__ inline long long job_count(long long njobs, const unsigned int *njobs_dev) {
    if (!njobs_dev) return njobs;
    const long long n = (long long)__hip_atomic_load(njobs_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return n < njobs ? n : njobs;
}

// The words of a context's d_counters, zeroed in front of every launch.  The host hands them out by these names; the band kernel and
// the wavefront kernel write theirs relative to a base pointer (NarrowParams::stats, FillParams::unl_stats), whose offsets have names
// of their own below.  The legacy service's private block (msa_legacy.hip) has the first three.
constexpr int kCounterWords = 32, kCounterBytes = kCounterWords * 4;
enum CounterSlot {
    CNT_FAST_QUEUE = 0,         // first pass's work queue (9PacBio: the strip kernel's)
    CNT_SLOW_COUNT = 1,         // jobs the first pass handed on (9PacBio: the strip kernel to the generic kernel)
    CNT_GENERIC_QUEUE = 2,
    CNT_BAND_QUEUE = 3,
    CNT_LIST_COUNT = 4,         // length of the first pass's list: the band kernel appends to it, the width sort starts it
    CNT_BAND_DONE = 5,          // jobs the band kernel finished
    CNT_BAND_HANDED = 6,        // candidates that left the band
    CNT_WIDE_SLOW_COUNT = 7,    // jobs the wide pass handed on
    CNT_WIDE_QUEUE = 8,
    CNT_UNL_RAN_UNL = 9,        // unlimited fills the prune-free loop ran
    CNT_UNL_RAN_GENERAL = 10,   // unlimited fills the general loop ran
    CNT_UNL_LIST_COUNT = 11,    // length of a width-sorted launch's list of unlimited fills
    CNT_UNL_QUEUE = 12,         // the unlimited build's work queue
    CNT_UNL_STEPS = 13,         // wavefront steps (columns + lanes in use - 1) of the unlimited fills
    CNT_ALL_STEPS = 14,         // ... of all fills
    CNT_CAND_COUNT = 15,        // length of a width-sorted launch's list of band candidates
    CNT_SORTED_COUNT = 16,      // length of its general list as the sort left it (before the band kernel's hand-overs)
    CNT_WAVE_STEPS = 17,        // steps the wavefronts ran (a wavefront steps as its longest job)
};
constexpr int CNT_BAND_STATS = 5, CNT_UNL_STATS = 9;               // what NarrowParams::stats / FillParams::unl_stats point at
enum BandStat { BAND_STAT_DONE = 0, BAND_STAT_HANDED = 1 };
enum UnlStat { UNL_STAT_RAN_UNL = 0, UNL_STAT_RAN_GENERAL = 1, UNL_STAT_STEPS = 4, UNL_STAT_ALL_STEPS = 5, UNL_STAT_WAVE_STEPS = 8 };
static_assert(CNT_BAND_DONE == CNT_BAND_STATS + BAND_STAT_DONE && CNT_BAND_HANDED == CNT_BAND_STATS + BAND_STAT_HANDED, "band kernel's counters");
static_assert(CNT_UNL_RAN_UNL == CNT_UNL_STATS + UNL_STAT_RAN_UNL && CNT_UNL_RAN_GENERAL == CNT_UNL_STATS + UNL_STAT_RAN_GENERAL &&
              CNT_UNL_STEPS == CNT_UNL_STATS + UNL_STAT_STEPS && CNT_ALL_STEPS == CNT_UNL_STATS + UNL_STAT_ALL_STEPS &&
              CNT_WAVE_STEPS == CNT_UNL_STATS + UNL_STAT_WAVE_STEPS, "wavefront kernel's counters");
constexpr bool counter_slots_distinct() {         // every name a word of its own, inside the block
    constexpr int all[] = {CNT_FAST_QUEUE, CNT_SLOW_COUNT, CNT_GENERIC_QUEUE, CNT_BAND_QUEUE, CNT_LIST_COUNT, CNT_BAND_DONE, CNT_BAND_HANDED,
                           CNT_WIDE_SLOW_COUNT, CNT_WIDE_QUEUE, CNT_UNL_RAN_UNL, CNT_UNL_RAN_GENERAL, CNT_UNL_LIST_COUNT, CNT_UNL_QUEUE,
                           CNT_UNL_STEPS, CNT_ALL_STEPS, CNT_CAND_COUNT, CNT_SORTED_COUNT, CNT_WAVE_STEPS};
    unsigned seen = 0;
    for (int s : all) { if (s < 0 || s >= kCounterWords || ((seen >> s) & 1u)) return false; seen |= 1u << s; }
    return true;
}
static_assert(counter_slots_distinct(), "two counter names share a word, or one lies outside d_counters");

struct FillParams {
    const bbmsa_job *jobs;
    const uint8_t *reads;
    const uint8_t *refs;
    bbmsa_result *results;
    uint8_t *match;
    long long njobs;
    const unsigned int *njobs_dev; // when set, the job count is read from here on the device (njobs = capacity)
    unsigned int *queue;          // work-queue head (zeroed before launch)
    unsigned int *dirbuf;         // traceback direction nibbles, one slot per resident job
    long long dir_slot_dwords;
    const int *list;              // job indices to process (NULL = all njobs), filled by the band kernel or the width sort
    const unsigned int *list_count;
    int priority;                 // s_setprio for the launch's wavefronts (0..3): the one-job-per-block passes are a dependent chain per job
                                  // and share their SIMDs with the throughput passes of the other stream
    int *slow_list;               // jobs the fast kernel hands to the generic kernel
    unsigned int *slow_count;
    int match_stride;
    int lanesPerJob;              // 16, 32 or 64
    int fastCols;                 // LDS capacity (columns) per job in the fast kernel
    int tmpBytes;                 // LDS bytes per job for the reversed match string
    int tableLen;                 // entries of the delC / insC tables (see lds_table_ints)
    int maxRows, maxColumns;      // context limits (MSA(maxRows_, maxColumns_))
    int bandwidth;
    float bandwidthRatio;
    unsigned int *unl_stats;      // bbmsa_last_unlimited's counters, indexed by UnlStat; NULL: not counted
    // matrix-materialising mode (the legacy per-call JNI shape, msa_legacy.hip; kernels instantiated with MAT only): job j's three
    // score planes go to planes + plane_off[j], each rows x columns ints (state-major; rows 1..rows, columns 1..columns of the matrix), its
    // vertLimit[0..rows] / horizLimit[0..columns] to limits + limits_off[j] (rows + 1 ints, then columns + 1)
    int *planes;
    const long long *plane_off;
    int *limits;
    const long long *limits_off;
};

// the band kernel in front of the first pass (msa_fill_band.hip): a job over 8 lanes, 16 jobs per wave.  (The name is its
// predecessor's, the one-job-per-lane narrow-window kernel, as are the switches and counters of the host side.)
struct NarrowParams {
    const bbmsa_job *jobs;
    const uint8_t *reads;
    const uint8_t *refs;
    bbmsa_result *results;
    uint8_t *match;
    long long njobs;
    const unsigned int *njobs_dev; // see FillParams
    unsigned int *queue;          // work-queue head (zeroed before launch)
    int *fast_list;               // jobs left to the wavefront kernel
    unsigned int *fast_count;
    unsigned int *stats;          // indexed by BandStat: jobs finished here, candidates that left the band (handed on)
    int match_stride;
    int maxRows, maxColumns;
    int bandwidth;
    float bandwidthRatio;
    int maxSlack;                 // candidate filter: maxQuality(rows) - minScore (points) at most this
    unsigned int *dirbuf32;       // per resident wave: (bandRows + 1) x 2 jobs x 64 lanes dwords of records
    int tableLen;                 // entries of the delC / insC tables (see lds_table_ints)
    int bandRows;                 // longest read it takes (its LDS areas and record slots are sized for it)
    const int *list;              // the jobs to try (the width sort's candidates); NULL = every job of the launch
    const unsigned int *list_count;   // the list's length, on the device (read when the kernel starts)
};

struct GenericParams {
    const bbmsa_job *jobs;
    const uint8_t *reads;
    const uint8_t *refs;
    bbmsa_result *results;
    uint8_t *match;
    const int *list;              // job indices to process (NULL = all)
    const unsigned int *list_count;
    long long njobs;
    const unsigned int *njobs_dev; // see FillParams
    int *matrix;                  // per-thread-slot 3*(maxRows+1)*(maxColumns+1) ints
    int *limits;                  // per-thread-slot vertLimit/horizLimit
    unsigned int *queue;
    int match_stride;
    int maxRows, maxColumns;
    int bandwidth;
    float bandwidthRatio;
};

}  // namespace bbmsa
