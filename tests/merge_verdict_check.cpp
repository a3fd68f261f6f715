// TEST INFRASTRUCTURE ONLY.  The normal mode's search restated line by line, for tests/merge_verdict_check.py, which compiles this
// file into a shared library: BBMergeOverlapper.mateByOverlapJava_unrolled (current/jgi/BBMergeOverlapper.java:543-657), the form
// BBMerge runs (its native is switched off at :68), WITH the inner early exit `bad <= badlim` of :586 that the library leaves out.
// The column weight is the Java's aprob[j] * bprob[i] (:591); jni/BBMergeOverlapper.c:73 has aprob[j] * bprob[j].
// Plain C++, nothing of the library is included.  The numbers at the right are the reference's lines.
#include <stdint.h>

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }
static int mid(int x, int y, int z) { return x < y ? (x < z ? imin(y, z) : x) : (y < z ? imin(x, z) : y); }

static const float probCorrect[] = {                                                                                       // :946-949
    0.000f, 0.251f, 0.369f, 0.499f, 0.602f, 0.684f, 0.749f, 0.800f, 0.842f, 0.874f, 0.900f, 0.921f, 0.937f, 0.950f, 0.960f, 0.968f,
    0.975f, 0.980f, 0.984f, 0.987f, 0.990f, 0.992f, 0.994f, 0.995f, 0.996f, 0.997f, 0.997f, 0.998f, 0.998f, 0.999f, 0.999f, 0.999f,
    0.999f, 0.999f, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};

// aqual == NULL or bqual == NULL: a pair without qualities.  aprob / bprob: scratch of at least max(alen, blen) floats.
// columns_out (may be NULL): the number of columns the inner loop visited, to show that the early exit is taken.
extern "C" int32_t chk_mate_by_overlap_java(const int8_t *abases, int alen, const int8_t *bbases, int blen, const int8_t *aqual, const int8_t *bqual,
                                            float *aprob, float *bprob, int32_t *rvector, int minOverlap0, const int minOverlap,
                                            const int minInsert0, int margin, const int maxMismatches0, const int maxMismatches, const int minq,
                                            int64_t *columns_out) {
    minOverlap0 = imin(imax(1, minOverlap0), minOverlap);                                                                  // :546
    margin = imax(margin, 0);                                                                                              // :548
    int bestOverlap = -1;                                                                                                  // :555
    int bestGood = -1;                                                                                                     // :556
    int bestBad = maxMismatches0;                                                                                          // :557
    bool ambig = false;                                                                                                    // :559
    const int maxOverlap = alen + blen - imax(minOverlap, minInsert0);                                                     // :560
    int64_t columns = 0;
    if (aqual != 0 && bqual != 0) {                                                                                        // :563
        for (int i = 0; i < alen; i++) { aprob[i] = probCorrect[aqual[i]]; }                                               // :564
        for (int i = 0; i < blen; i++) { bprob[i] = probCorrect[bqual[i]]; }                                               // :565
    } else {
        for (int i = 0; i < alen; i++) { aprob[i] = 0.98f; }                                                               // :567
        for (int i = 0; i < blen; i++) { bprob[i] = 0.98f; }                                                               // :568
    }
    const float minprob = probCorrect[mid(1, minq, 41)];                                                                   // :571
    for (int overlap = imax(minOverlap0, 0); overlap < maxOverlap; overlap++) {                                            // :573
        int good = 0, bad = 0;                                                                                             // :576
        int istart = (overlap <= alen ? 0 : overlap - alen);                                                               // :578
        int jstart = (overlap <= alen ? alen - overlap : 0);                                                               // :579
        {
            const int iters = imin(overlap - istart, imin(blen - istart, alen - jstart));                                  // :582
            const int imx = istart + iters;                                                                                // :583
            const int badlim = bestBad + margin;                                                                           // :584
            for (int i = istart, j = jstart; i < imx && bad <= badlim; i++, j++) {                                         // :586
                const int8_t ca1 = abases[j], cb1 = bbases[i];                                                             // :590
                const float pc = aprob[j] * bprob[i];                                                                      // :591
                columns++;
                if (pc <= minprob) {                                                                                       // :593
                } else if (ca1 == cb1) { good++; }                                                                         // :594
                else { bad++; }                                                                                            // :595
            }
        }
        if (bad * 2 < good) {                                                                                              // :610
            if (good > minOverlap) {                                                                                       // :612
                if (bad <= bestBad) {                                                                                      // :614
                    if (bad < bestBad || (bad == bestBad && good > bestGood)) {                                            // :617
                        if (bestBad - bad < margin) { ambig = true; }                                                      // :619
                        bestOverlap = overlap;                                                                             // :620
                        bestBad = bad;                                                                                     // :621
                        bestGood = good;                                                                                   // :622
                    } else if (bad == bestBad) {                                                                           // :623
                        ambig = true;                                                                                      // :625
                    }
                    if (ambig && bestBad < margin) {                                                                       // :628
                        rvector[2] = bestBad;                                                                              // :630
                        rvector[4] = (ambig ? 1 : 0);                                                                      // :631
                        if (columns_out) *columns_out = columns;
                        return -1;                                                                                         // :632
                    }
                }
            } else if (bad < margin) {                                                                                     // :635
                ambig = true;                                                                                              // :637
                rvector[2] = bestBad;                                                                                      // :638
                rvector[4] = (ambig ? 1 : 0);                                                                              // :639
                if (columns_out) *columns_out = columns;
                return -1;                                                                                                 // :640
            }
        }
    }
    if (!ambig && bestBad > maxMismatches - margin) { bestOverlap = -1; }                                                  // :647
    rvector[2] = bestBad;                                                                                                  // :649
    rvector[4] = (ambig ? 1 : 0);                                                                                          // :650
    if (columns_out) *columns_out = columns;
    return (bestOverlap < 0 ? -1 : alen + blen - bestOverlap);                                                             // :656
}
