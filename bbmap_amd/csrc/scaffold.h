// Scaffold boundaries inside a chromosome array (include/bbmap_amd.h, bbidx_set_scaffolds / bbmap_get_scaffold_records).
//
// FastaToChromArrays2 packs many FASTA records (scaffolds) into one chromosome array, 300 N apart (MID_PADDING,
// current/dna/FastaToChromArrays2.java:432-524), and the mapper consults the per-chromosome table of scaffold starts in two places:
//   removeOutOfBounds drops every probe site that spans two scaffolds (AbstractMapThread.java:2444-2476, Data.isSingleScaffold,
//   current/dna/Data.java:1112-1140), and SamLine turns a final record into scaffold-relative coordinates, unmapping a record that
//   still spans two (current/stream/SamLine.java:120-187).
// Device layout (CSR over the chromosome numbers): chromosome c's scaffolds are loc[off[c] .. off[c+1]) / len[...], starts strictly
// ascending; the position in loc is the scaffold's global number (FASTA order).
#pragma once
#include <hip/hip_runtime.h>

#include "bbmap_amd.h"

namespace bbscaf {

struct Table {
    const int *off;             // [nchroms + 2]; nullptr = no table (isSingleScaffold is true everywhere)
    const int *loc, *len;
    int pad;                    // Data.interScaffoldPadding
    int nchroms;
};

// Arrays.binarySearch(array, key) and the insert-point rule that Data.scaffoldIndex (:1091-1108) and isSingleScaffold (:1117-1128)
// share: the exact hit, else max(0, insertPoint - 1) -- with strictly ascending starts, the last start <= key (0 when none is).
__device__ inline int last_at_or_below(const int *a, int n, int key) {
    int lo = 0, hi = n;                                     // #(a[i] <= key) lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a[mid - 1] <= key) lo = mid; else hi = mid - 1;
    }
    return lo > 0 ? lo - 1 : 0;
}

// Data.isSingleScaffold (current/dna/Data.java:1112-1140), per thread.
__device__ inline bool is_single_scaffold(const Table &T, int chrom, int loc1, int loc2) {
    if (chrom < 1 || chrom > T.nchroms) return true;
    const int b = T.off[chrom], n = T.off[chrom + 1] - b;
    if (n < 2) return true;                                 // array==null || array.length<2
    const int *a = T.loc + b;
    const int scaf = last_at_or_below(a, n, loc1 + T.pad);
    if (scaf == n - 1) return true;
    const int lowerBound = a[scaf] - T.pad, upperBound = a[scaf + 1];
    if (loc2 < lowerBound || loc1 > upperBound) return false;      // "a random read generated in the start or stop padding"
    return loc2 < upperBound;
}

// The same search for a whole wavefront (a, n, key wave-uniform; every lane active): each lane tests one of 64 evenly spaced pivots
// and a ballot narrows the range to one stride, so a table of n starts costs about log64(n) rounds of one gather each instead of
// log2(n) dependent loads.  Returns #(a[i] <= key).
__device__ inline int wave_count_le(const int *a, int n, int key) {
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = n;                                     // #(a[i] <= key) lies in [lo, hi]
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6;
        const int p = lo + (lane + 1) * step - 1;           // pivots lo + step - 1, lo + 2 step - 1, ... (the last one reaches hi - 1)
        const int k = __popcll(__ballot(p < hi && a[p] <= key));     // pivots are ascending: the true ones are a prefix
        const int nlo = lo + k * step;
        hi = min(hi, lo + (k + 1) * step - 1);
        lo = nlo;
    }
    const int p = lo + lane;
    return lo + __popcll(__ballot(p < hi && a[p] <= key));
}
__device__ inline int wave_last_at_or_below(const int *a, int n, int key) {
    const int c = wave_count_le(a, n, key);
    return c > 0 ? c - 1 : 0;
}

}  // namespace bbscaf
