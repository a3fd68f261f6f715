// SAM record fields on the device (include/bbmap_amd.h, bbmap_get_sam_records_cfg / bbpipe_sam_records_device): the launches of
// sam_records.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "batch_view.h"
#include "bbmap_amd.h"

namespace bbsam {

struct Args {
    BatchView V;                                            // (the site lists are read for XM only)
    const bbmap_scafrec *scaf;                              // bbmap_get_scaffold_records' output for the same batch
    const uint8_t *const *chromArr; const int *chromArrLen;
    const float *mapqMax; int mapqMaxLen;                   // 1.5f * (float)log2(length) + 36 by read length, [0, mapqMaxLen]
    int flags;                                              // BBMAP_SAM_CIGAR13 | BBMAP_SAM_MD
    int intronLimit;                                        // SamLine.INTRON_LIMIT
    int tags;                                               // BBMAP_SAM_MAKE_* | BBMAP_SAM_XS_SECONDSTRAND | BBMAP_SAM_NO_TAGS
    long long textCap;                                      // bytes of the text blob: the emit pass writes nothing behind them
};

// mapqMax[len] as SamLine.toMapq computes it (current/stream/SamLine.java:1718, Tools.log2 current/align2/Tools.java:2304-2317)
void fill_mapq_max(float *table, int maxLen);
// Sizing pass: every fixed-size field of recs[r], the string lengths, counts[r] = bytes of read r's strings; tags: null, or where the
// further tags' values go.
hipError_t launch_size(const Args &a, bbmap_samrec *recs, bbmap_samtags *tags, int *counts, hipStream_t stream);
// Emit pass: offsets = exclusive prefix sums of counts; writes the strings and the records' offsets.
hipError_t launch_emit(const Args &a, bbmap_samrec *recs, const long long *offsets, uint8_t *text, hipStream_t stream);

}  // namespace bbsam
