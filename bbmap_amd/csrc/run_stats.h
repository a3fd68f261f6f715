// Run statistics on the device (include/bbmap_amd.h, bbmap_add_run_stats / bbpipe_run_stats_device): the launch of run_stats.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_view.h"
#include "bbmap_amd.h"

namespace bbrunstats {

// bbmap_runstats as the kernel addresses it: PER_MATE counters of mate 1, the same of mate 2, then the pair-level ones.
enum { PER_MATE = 43, PAIR_BASE = 2 * PER_MATE, PAIR_LEVEL = 9, N_COUNTERS = 96 };
enum { WAVES_PER_BLOCK = 4, MAX_BLOCKS = BBMAP_RUNSTATS_MAX_WAVES / WAVES_PER_BLOCK };
static_assert(sizeof(bbmap_runstats) == 8 * N_COUNTERS, "bbmap_runstats is 96 counters");
static_assert(PER_MATE + PAIR_LEVEL <= 64, "one lane per counter a read can move");

struct Args {
    BatchView V;                                            // (bases are not read)
    const bbmap_truth *truth;                               // nullptr = no read has a truth record
    int ptsMatch, ptsMatch2;                                // MSA.maxQuality(len) = ptsMatch + (len - 1) * ptsMatch2
    int thresh, maxPairDist;
};

hipError_t launch(const Args &a, unsigned long long *counters, unsigned long long *ihist, hipStream_t stream);

}  // namespace bbrunstats
