// Coverage on the device (include/bbmap_amd.h, bbmap_cov_* / bbpipe_coverage_*): the launches of coverage.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_view.h"
#include "bbmap_amd.h"
#include "scaffold.h"

namespace bbcov {

enum { WAVES_PER_BLOCK = 4, TB = 64 * WAVES_PER_BLOCK, MAX_BLOCKS = BBMAP_COV_MAX_WAVES / WAVES_PER_BLOCK };
enum { TILE = BBMAP_COV_SCAN_TILE, PER_THREAD = TILE / TB };               // the prefix sum: 8 consecutive slots per thread
enum { CHUNK = BBMAP_COV_STATS_CHUNK };                     // slots per workgroup of the passes that only read the depths (statistics, median counts)
enum { MEDIAN_SHORT = BBMAP_COV_MEDIAN_SHORT, HIST_LDS = BBMAP_COV_HIST_LDS_BINS };
enum { LDS_SCAF = BBMAP_COV_LDS_SCAFFOLDS };                  // tables of up to this many scaffolds keep a workgroup's per-scaffold counters in LDS
// bbmap_covrec as the kernels address it, in 64-bit words: length, the N_ACC counters a read moves, refBases, the two strands
enum { REC_WORDS = 25, ACC_BASE = 1, N_ACC = 8, REF_BASE = 9, STRAND_BASE = 13, STRAND_WORDS = 6 };
enum { A_basehits, A_readhits, A_readhitsMinus, A_fraghits, A_readBases };
enum { S_covered, S_median, S_max, S_sumDepth, S_sumSqLo, S_sumSqHi };
static_assert(sizeof(bbmap_covrec) == 8 * REC_WORDS && sizeof(bbmap_covstrand) == 8 * STRAND_WORDS, "bbmap_covrec is 25 words");
static_assert(sizeof(bbmap_covtotals) == 32, "bbmap_covtotals is 4 words");

struct AddArgs {
    BatchView V;
    int flags;
    bbscaf::Table T; int nscaf;
    const long long *covoff;
    int *diff[2];
    unsigned long long *recs, *totals;
};
hipError_t launch_add(const AddArgs &a, hipStream_t stream);

struct FinArgs {
    int flags, nscaf; long long slots;
    const int *len; const long long *covoff;
    const int *diff[2]; void *depth[2];
    unsigned long long *recs; const long long *refgc;
    unsigned long long *hist[2];
    int binsize; const long long *binoff; long long nbins; unsigned long long *bins[2];
    unsigned long long *totals;
    void *ws;
};
inline long long hist_bins(int flags) { return flags & BBMAP_COV_32BIT ? 1000001 : 65536; }         // writeStats' histmax + 1 (:1009)
long long workspace_bytes(int nscaf, long long slots);
hipError_t launch_finalize(const FinArgs &a, hipStream_t stream);
// A / C / G / T of every scaffold's own bases in the index's chromosome arrays -> refgc[nscaf][4] (zeroed here)
hipError_t launch_refgc(const bbscaf::Table &T, int nscaf, const uint8_t *const *chromArr, long long *refgc, hipStream_t stream);

}  // namespace bbcov
