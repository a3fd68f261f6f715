// Read.insertSizeMapped(r1, r2, false) (current/stream/Read.java:2618-2670) for a read with a mate: run statistics' insert-size
// histogram (run_stats.hip) and the X8 tag (sam_records.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace bbinsert {

struct Mate { int strand, start, stop, chrom, len; };
__device__ inline int insert_unstranded(Mate r1, Mate r2) {                                       // :2643-2670
    if (r1.start > r2.start) { const Mate t = r1; r1 = r2; r2 = t; }
    if (r1.start == r1.stop || r2.start == r2.stop) return 0;
    if (r1.chrom != r2.chrom) return 0;
    const int a = r1.len, b = r2.len;
    if (r1.start < r2.start) {
        const int mid = r2.start - r1.stop - 1;
        if (-mid >= a + b) return 0;
        return mid + a + b;
    }
    return a < b ? a : b;
}
__device__ inline int insert_plus_left(Mate r1, Mate r2) {                                        // :2629-2641
    if (r1.strand > r2.strand) { const Mate t = r1; r1 = r2; r2 = t; }
    if (r1.strand == r2.strand || r1.start > r2.stop) return insert_unstranded(r2, r1);
    if (r1.chrom != r2.chrom) return 0;
    if (r1.start == r1.stop || r2.start == r2.stop) return 0;
    const int a = r1.len, b = r2.len;
    const int mid = r2.start - r1.stop - 1;
    if (-mid >= a + b) return insert_unstranded(r1, r2);
    return mid + a + b;
}
__device__ inline int insert_size_mapped(const Mate &r1, const Mate &r2) {                         // :2622-2626 (both mapped, ignoreStrand false)
    return r1.strand == r2.strand ? insert_unstranded(r1, r2) : insert_plus_left(r1, r2);
}

}  // namespace bbinsert
