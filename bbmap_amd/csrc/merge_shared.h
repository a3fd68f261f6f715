// The merge stage's arithmetic, shared by its host form and its kernels (merge.hip): BBMerge's ratio-mode overlap natives
// (jni/BBMergeOverlapper.c: findBestRatio :127-179, findBestRatio_WithQualities :182-228, mateByOverlapRatio_WithQualities :230-319,
// mateByOverlapRatio :321-402) and one column of Read.joinRead's overlapped branch (current/stream/Read.java:2804-2840).
//
// The natives are cut at one seam.  For an insert, findBestRatio and the main loop sum the same columns; only their `badlimit`
// differs, and it only decides where the column loop stops.  The addends are not negative, so `bad` never falls: the loop stops
// early exactly when the full sum fails `bad <= badlimit`, and then the insert is skipped whatever `good` was.  So (good, bad) are
// summed once per insert over every column (column_sums, in the reference's order: float32, no reassociation, no contraction), the
// quotient (bad + offset) / overlapLength is taken beside them, and the two decision walks run over the stored triples, from the
// largest insert to the smallest, with the reference's running state and its early returns.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bbmap_amd.h"

namespace bbmerge {

#define BBM_HD __host__ __device__ inline

// QualityTools.PROB_CORRECT as the natives embed it (jni/BBMergeOverlapper.c:45-49); qualities above 70 are outside it
#define BBMERGE_PROB_CORRECT                                                                                                              \
    0.000f, 0.251f, 0.369f, 0.499f, 0.602f, 0.684f, 0.749f, 0.800f, 0.842f, 0.874f, 0.900f, 0.921f, 0.937f, 0.950f, 0.960f, 0.968f,       \
    0.975f, 0.980f, 0.984f, 0.987f, 0.990f, 0.992f, 0.994f, 0.995f, 0.996f, 0.997f, 0.997f, 0.998f, 0.998f, 0.999f, 0.999f, 0.999f,       \
    0.999f, 0.999f, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1
constexpr int MAX_QUALITY = 70;

BBM_HD int imin(int a, int b) { return a < b ? a : b; }
BBM_HD int imax(int a, int b) { return a > b ? a : b; }
BBM_HD float fmin2(float a, float b) { return a < b ? a : b; }
BBM_HD float fmax2(float a, float b) { return a > b ? a : b; }
BBM_HD int mid(int x, int y, int z) { return x < y ? (x < z ? imin(y, z) : x) : (y < z ? imin(x, z) : y); }

// the natives' arguments after their own clamping (:236-237, :327-328)
struct Params {
    int minOverlap0, minOverlap, minInsert0, minInsert;
    float maxRatio, margin, offset, gIncr, bIncr;
};
BBM_HD Params params_of(const bbmerge_config &c) {
    Params p;
    p.minOverlap = imax(4, imax(c.minOverlap0, c.minOverlap));
    p.minOverlap0 = mid(4, c.minOverlap0, p.minOverlap);
    p.minInsert0 = c.minInsert0; p.minInsert = c.minInsert;
    p.maxRatio = c.maxRatio; p.margin = c.ratioMargin; p.offset = c.ratioOffset; p.gIncr = c.gIncr; p.bIncr = c.bIncr;
    return p;
}

inline bool good_config(const bbmerge_config &c) {
    const float f[5] = {c.maxRatio, c.ratioMargin, c.ratioOffset, c.gIncr, c.bIncr};
    for (float x : f) if (x != x) return false;
    return c.ratioMargin >= 1 && c.gIncr >= 0 && c.bIncr >= 0 && c.minInsert0 >= 0 && c.minInsert >= 0 && c.maxMergeQuality >= 0 &&
           c.maxMergeQuality <= 127;
}

// The inserts either walk visits are hi, hi - 1, ..., lo (none when hi < lo); triple k belongs to insert hi - k.
struct Range { int hi, lo; };
BBM_HD Range insert_range(const Params &p, int alen, int blen) {
    Range r;
    r.hi = alen + blen - p.minOverlap0;                  // (minOverlap0 <= minOverlap: the main loop's start is the larger one)
    r.lo = imin(p.minInsert, p.minInsert0);
    return r;
}

// the overlap of the two reads for an insert (:139-141, :196-198, :274-277, :349-351); len is never negative for insert >= 0
struct Span { int istart, jstart, len; };
BBM_HD Span span_of(int insert, int alen, int blen) {
    Span s;
    s.istart = insert <= blen ? 0 : insert - blen;
    s.jstart = insert >= blen ? 0 : blen - insert;
    s.len = imin(alen - s.istart, imin(blen - s.jstart, insert));
    return s;
}

// good and bad of one insert over all its columns.  S gives base(i) and, for the quality form, prob(i).
template <bool Q, class SA, class SB>
BBM_HD void column_sums(const SA &A, const SB &B, const Span &s, float gIncr, float bIncr, float &good, float &bad) {
    good = 0; bad = 0;
    for (int c = 0; c < s.len; c++) {
        const int ca = A.base(s.istart + c), cb = B.base(s.jstart + c);
        // (selects, not branches: the sums stay in registers and the lanes of a wavefront in step; the additions are the same)
        const bool same = ca == cb;
        if (Q) {
            const float x = A.prob(s.istart + c) * B.prob(s.jstart + c);
            good = same ? good + x : good;
            bad = same ? bad : bad + x;
        } else {
            good = same && ca != 'N' ? good + gIncr : good;
            bad = same ? bad : bad + bIncr;
        }
    }
}

BBM_HD float ratio_of(float bad, float offset, int len) { return (bad + offset) / len; }

// findBestRatio's loop body (:142-176 / :199-226) over a stored triple; true: the function returned `ret`
struct BestRatioWalk {
    float bestRatio, halfmax, ret;
    BBM_HD void start(float maxRatio) { bestRatio = maxRatio + 0.0001f; halfmax = maxRatio * 0.5f; }
    BBM_HD bool step(float good, float bad, float ratio, int len, int minOverlap0, int minOverlap) {
        const float badlimit = bestRatio * len;
        if (bad <= badlimit) {
            if (bad == 0 && good > minOverlap0 && good < minOverlap) { ret = 100.0f; return true; }
            if (ratio < bestRatio) {
                bestRatio = ratio;
                if (good >= minOverlap && ratio < halfmax) { ret = bestRatio; return true; }
            }
        }
        return false;
    }
    BBM_HD float finish() { ret = bestRatio; return ret; }
};

// the main loop's body (:278-316 / :352-399); true: the native returned (insert -1, bad = bestBad, ambiguous)
struct MainWalk {
    float maxRatio, altBadlimit, margin2, bestBad, bestRatio;
    int bestInsert, ambig;
    BBM_HD void start(float maxRatio_, int alen, int minLength, float margin, float offset) {
        maxRatio = maxRatio_;
        altBadlimit = fmax2(maxRatio, 0.07f) * 2.0f * alen + 1;
        margin2 = (margin + offset) / minLength;
        bestInsert = -1; ambig = 0;
        bestBad = minLength; bestRatio = 1;
    }
    BBM_HD float bound(float margin, int len) const { return fmin2(bestRatio, maxRatio) * margin * len; }
    BBM_HD bool step(int insert, float good, float bad, float ratio, int len, float margin, int minOverlap0, int minOverlap) {
        const float badlimit = fmin2(altBadlimit, bound(margin, len));
        if (bad <= badlimit) {
            if (bad == 0 && good > minOverlap0 && good < minOverlap) return true;
            if (ratio < bestRatio * margin) {
                ambig = (ratio * margin >= bestRatio || good < minOverlap);
                if (ratio < bestRatio) { bestInsert = insert; bestBad = bad; bestRatio = ratio; }
                if (ambig && bestRatio < margin2) return true;
            }
        }
        return false;
    }
    BBM_HD void returned_early(bbmerge_rec &r) const { r.insert = -1; r.bad = (int32_t)bestBad; r.ambig = 1; }
    BBM_HD void finish(bbmerge_rec &r) {
        if (!ambig && bestRatio > maxRatio) bestInsert = -1;
        r.insert = bestInsert < 0 ? -1 : bestInsert; r.bad = (int32_t)bestBad; r.ambig = ambig ? 1 : 0;
    }
};

// findBestRatio's verdict in the caller (:243-249 uses x > maxRatio, :334-340 x >= maxRatio); true: the native returns here
template <bool Q> BBM_HD bool no_ratio(float x, float maxRatio, int minLength, bbmerge_rec &r) {
    if (Q ? x > maxRatio : x >= maxRatio) { r.insert = -1; r.bad = minLength; r.ambig = 0; return true; }
    return false;
}

// One native over stored triples.  T gives good(k), bad(k), ratio(k) for insert range.hi - k.  Most inserts fail `bad <= badlimit`
// under any state a walk can be in, so a walk does not visit them one by one: it takes 64 inserts at a time, every lane tests one
// against the limit as it stands at the head of the 64 (bestRatio only falls, the products are monotone in it and lengths are not
// negative, so what fails there fails at its own turn too; a NaN limit fails both), and the walk steps through the survivors in
// order, with the exact test.  W::ballot(f) is the mask of lanes for which f(lane) holds: the wavefront on the device, a loop over
// 64 lanes on the host, so both forms run this very code.
typedef unsigned long long LaneMask;
template <bool Q, class W, class T> BBM_HD void decide(const W &wave, const T &t, const Params &p, const Range &range, int alen, int blen, bbmerge_rec &r) {
    const int minLength = imin(alen, blen);
    BestRatioWalk w1;
    w1.start(p.maxRatio);
    bool returned = false;
    // findBestRatio: inserts alen + blen - minOverlap .. minInsert, that is triples first .. last
    for (int k0 = range.hi - (alen + blen - p.minOverlap), last = range.hi - p.minInsert; k0 <= last && !returned; k0 += 64) {
        const float head = w1.bestRatio;
        LaneMask m = wave.ballot([&](int lane) {
            const int k = k0 + lane;
#ifdef BBMERGE_WALK_EVERY_INSERT          // (an experiment's build, DESIGN 8l: no wave-wide test, the walk visits every insert)
            return k <= last;
#endif
            return k <= last && t.bad(k) <= head * span_of(range.hi - k, alen, blen).len;
        });
        for (; m && !returned; m &= m - 1) {
            const int k = k0 + __builtin_ctzll(m);
            returned = w1.step(t.good(k), t.bad(k), t.ratio(k), span_of(range.hi - k, alen, blen).len, p.minOverlap0, p.minOverlap);
        }
    }
    const float x = returned ? w1.ret : w1.finish();
    if (no_ratio<Q>(x, p.maxRatio, minLength, r)) return;
    MainWalk w2;
    w2.start(fmin2(p.maxRatio, x), alen, minLength, p.margin, p.offset);
    // the main loop: inserts range.hi .. minInsert0
    for (int k0 = 0, last = range.hi - p.minInsert0; k0 <= last; k0 += 64) {
        const MainWalk head = w2;
        LaneMask m = wave.ballot([&](int lane) {
            const int k = k0 + lane;
#ifdef BBMERGE_WALK_EVERY_INSERT
            return k <= last;
#endif
            return k <= last && t.bad(k) <= head.bound(p.margin, span_of(range.hi - k, alen, blen).len);
        });
        for (; m; m &= m - 1) {
            const int k = k0 + __builtin_ctzll(m);
            if (w2.step(range.hi - k, t.good(k), t.bad(k), t.ratio(k), span_of(range.hi - k, alen, blen).len, p.margin, p.minOverlap0, p.minOverlap)) {
                w2.returned_early(r);
                return;
            }
        }
    }
    w2.finish(r);
}

// BBMerge.mateByOverlap_ratioMode's choice of forms (BBMerge.java:1627-1637)
BBM_HD bool runs_quality_form(const bbmerge_config &c, bool have_quality) { return c.useQuality != 0 && have_quality; }
BBM_HD bool runs_flat_form(const bbmerge_config &c, bool ran_quality, const bbmerge_rec &r) {
    return !ran_quality || (c.withoutQuality != 0 && (r.insert < 0 || r.ambig == 1));
}

// Position i of joinRead's result for an overlapped pair (Read.java:2806-2818 without qualities, :2820-2839 with): a's base or 0
// (`new byte[insert]`), then b's base at j = blen - insert + i where that is >= 0.  b is mate 2 reverse-complemented.  Bytes compare
// as Java's signed bytes.
BBM_HD void join_column(bool with_quality, int8_t ca, int8_t qa, bool have_b, int8_t cb, int8_t qb, int maxMergeQuality, uint8_t &base,
                        uint8_t &qual) {
    if (have_b) {
        if (!with_quality) {
            if (ca == 0 || ca == 'N') ca = cb;
            else if (ca != cb) ca = ca >= cb ? ca : cb;
        } else if (ca == 0 || ca == 'N') {
            ca = cb; qa = qb;
        } else if (cb == 0 || cb == 'N') {
        } else if (ca == cb) {
            qa = (int8_t)imin(imax(qa, qb) + imin(qa, qb) / 4, maxMergeQuality);
        } else {
            ca = qa > qb ? ca : qa < qb ? cb : (int8_t)'N';
            qa = (int8_t)(imax(qa, qb) - imin(qa, qb));
        }
    }
    base = (uint8_t)ca; qual = (uint8_t)qa;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// BBMerge's verdict (bbmerge_verdict_batch): what BBMerge.mateByOverlap (current/jgi/BBMerge.java:1741-1837) and
// processReadPair_inner (:2044-2068) put around the ratio search.  A mate S gives base(i), prob(i) = probCorrect[q] and qual(i).

// BBMergeOverlapper.probCorrect2 (BBMergeOverlapper.java:951-956): 60 entries, the filters' table
#define BBMERGE_PROB_CORRECT2                                                                                                             \
    0.0000f, 0.2501f, 0.3690f, 0.4988f, 0.6019f, 0.6838f, 0.7488f, 0.8005f, 0.8415f, 0.8741f, 0.9000f, 0.9206f, 0.9369f, 0.9499f,         \
    0.9602f, 0.9684f, 0.9749f, 0.9800f, 0.9842f, 0.9874f, 0.9900f, 0.9921f, 0.9937f, 0.9950f, 0.9960f, 0.9968f, 0.9975f, 0.9980f,         \
    0.9984f, 0.9987f, 0.9990f, 0.9992f, 0.9994f, 0.9995f, 0.9996f, 0.9997f, 0.9997f, 0.9998f, 0.9998f, 0.9999f, 0.9999f, 0.9999f,         \
    0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f, 0.9999f,         \
    0.9999f, 0.9999f, 0.9999f, 0.9999f
constexpr int MAX_FILTER_QUALITY = 59;
constexpr int MAX_ENTROPY_K = 5;

inline bool good_verdict_config(const bbmerge_verdict_config &c) {
    const float f[3] = {c.efilterRatio, c.efilterOffset, c.pfilterRatio};
    for (float x : f) if (x != x) return false;
    return good_config(c.ratio) && c.entropyK >= 1 && c.entropyK <= MAX_ENTROPY_K && c.qualIters >= 1 && c.maxMismatches0 >= 0 &&
           c.maxMismatches0 >= c.maxMismatches && c.margin <= c.maxMismatches && (c.useRatioMode != 0 || c.useNormalMode != 0);
}

// which tables a pair's qualities index; have_quality: useQuality is set and the batch has qualities (BBMerge.java:1913-1916)
BBM_HD bool reads_prob_correct(const bbmerge_verdict_config &c, bool have_quality) {
    return have_quality && ((c.useRatioMode != 0 && c.ratio.useQuality != 0) || c.useNormalMode != 0);
}
BBM_HD bool filters_on(const bbmerge_verdict_config &c, bool have_quality) { return have_quality && (c.useEfilter != 0 || c.pfilterRatio > 0); }

// AminoAcid.isFullyDefined with Dedupe.baseToNumber: the base's number, -1 where it is not fully defined
BBM_HD int base_number(int b) {
    switch (b) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': case 'U': case 'u': return 3;
    }
    return -1;
}

// calcMinOverlapByEntropyHead (BBMergeOverlapper.java:898-934) over s.base(0 .. n - 1); the Tail form (:860-896) is the same scan
// over the mate read from its end, which is what the caller's view does.  counts: 4^k entries, zeroed by the caller (Arrays.fill).
template <class S> BBM_HD int entropy_scan(const S &s, int n, int k, int minscore, uint16_t *counts) {
    const int mask = ~((-1) << (2 * k));
    int kmer = 0, len = 0, ones = 0, twos = 0;
    for (int i = 0; i < n; i++) {
        const int x = base_number(s.base(i));
        if (x < 0) {
            len = 0; kmer = 0;
        } else {
            len++;
            kmer = ((kmer << 2) | x) & mask;
            if (len >= k) {
                const int c = ++counts[kmer];
                if (c == 1) ones++;
                else if (c == 2) twos++;
                if (ones * 4 + twos >= minscore) return i;
            }
        }
    }
    return n + 1;
}
template <class S> struct FromEnd {
    S s; int n;
    BBM_HD int base(int i) const { return s.base(n - 1 - i); }
};

// mateByOverlapJava_unrolled's arguments for pass i of mateByOverlap_normalMode's loop (BBMerge.java:1651-1654) after its own clamping
// (BBMergeOverlapper.java:546-548, :560, :571-573).  The overlaps a pass visits are first, first + 1, ..., maxOverlap - 1.
struct NormalParams { int minOverlap, margin, maxMismatches0, maxMismatches, first, maxOverlap, minq; };
BBM_HD NormalParams normal_params(const bbmerge_verdict_config &c, int pairMinOverlap, int pass, int alen, int blen) {
    NormalParams p;
    p.minOverlap = pairMinOverlap + pass;
    p.first = imax(imin(imax(1, c.minOverlapBases0 - pass), p.minOverlap), 0);
    p.margin = imax(c.margin, 0);
    p.maxMismatches0 = c.maxMismatches0; p.maxMismatches = c.maxMismatches;
    p.maxOverlap = alen + blen - imax(p.minOverlap, c.ratio.minInsert0);
    p.minq = mid(1, (int)(int8_t)(c.minQuality - 2 * pass), 41);             // (the index of minprob in probCorrect)
    return p;
}

// good and bad of one overlap over all its columns (:576-596 without `bad <= badlim`): i walks b, j walks a
template <bool Q, class SA, class SB> BBM_HD void normal_counts(const SA &A, const SB &B, int overlap, int alen, int blen, float minprob, int &good, int &bad) {
    const int istart = overlap <= alen ? 0 : overlap - alen;
    const int jstart = overlap <= alen ? alen - overlap : 0;
    const int iters = imin(overlap - istart, imin(blen - istart, alen - jstart));
    good = 0; bad = 0;
    for (int c = 0; c < iters; c++) {
        const float pc = Q ? A.prob(jstart + c) * B.prob(istart + c) : 0.98f * 0.98f;
        const bool counts = !(pc <= minprob), same = A.base(jstart + c) == B.base(istart + c);
        good += counts && same; bad += counts && !same;
    }
}

// the decision walk of mateByOverlapJava_unrolled (:610-644) for an overlap that passed `bad * 2 < good`; true: it returned -1
struct NormalWalk {
    int bestOverlap, bestGood, bestBad, ambig;
    BBM_HD void start(const NormalParams &p) { bestOverlap = -1; bestGood = -1; bestBad = p.maxMismatches0; ambig = 0; }
    BBM_HD bool step(const NormalParams &p, int overlap, int good, int bad) {
        if (good > p.minOverlap) {
            if (bad <= bestBad) {
                if (bad < bestBad || (bad == bestBad && good > bestGood)) {
                    if (bestBad - bad < p.margin) ambig = 1;
                    bestOverlap = overlap; bestBad = bad; bestGood = good;
                } else if (bad == bestBad) {
                    ambig = 1;
                }
                if (ambig && bestBad < p.margin) return true;
            }
        } else if (bad < p.margin) {
            ambig = 1;
            return true;
        }
        return false;
    }
};
// One pass over stored counts: T gives good(k), bad(k) of overlap p.first + k.  `bad * 2 < good` does not depend on the walk's state,
// so the wave tests it for 64 overlaps at a time and the walk visits the rest in order.  Returns the insert or -1; bad and ambig are
// rvector[2] and rvector[4].
template <class W, class T> BBM_HD int normal_decide(const W &wave, const T &t, const NormalParams &p, int alen, int blen, int &bad, int &ambig) {
    NormalWalk w;
    w.start(p);
    for (int k0 = 0, n = p.maxOverlap - p.first; k0 < n; k0 += 64) {
        LaneMask m = wave.ballot([&](int lane) { const int k = k0 + lane; return k < n && t.bad(k) * 2 < t.good(k); });
        for (; m; m &= m - 1) {
            const int k = k0 + __builtin_ctzll(m);
            if (w.step(p, p.first + k, (int)t.good(k), (int)t.bad(k))) { bad = w.bestBad; ambig = 1; return -1; }
        }
    }
    if (!w.ambig && w.bestBad > p.maxMismatches - p.margin) w.bestOverlap = -1;
    bad = w.bestBad; ambig = w.ambig;
    return w.bestOverlap < 0 ? -1 : alen + blen - w.bestOverlap;
}

// The two filters, each cut at one seam like the ratio sums: a column's term depends on that column alone (term functions below), and
// only the running sum or product has an order.  The host form takes the columns one after the other; the kernel lets 64 lanes work
// out 64 terms and then adds or multiplies them in the reference's order.  An N column does nothing in the reference; here it has the
// neutral term (+0 to a sum that is never negative, 1 to a product), which leaves every bit as it was.
struct FilterSpan { int istart, jstart, n; };          // columns (istart + c, jstart + c), c < n: the loops' `i < x && i < alen && j < blen`
BBM_HD FilterSpan filter_span(int istart, int jstart, int upto, int alen, int blen) {
    FilterSpan s = {istart, jstart, imax(0, imin(upto - istart, imin(alen - istart, blen - jstart)))};
    return s;
}
// BBMergeOverlapper.expectedMismatches (:667-724) with qualities; note jstart from alen (the reference's own convention)
BBM_HD FilterSpan expected_span(int alen, int blen, int overlap) {
    return filter_span(overlap <= blen ? 0 : overlap - blen, overlap <= alen ? alen - overlap : 0, overlap, alen, blen);
}
template <class SA, class SB> BBM_HD float expected_term(const SA &A, const SB &B, int i, int j, const float *probCorrect2) {
    if (A.base(i) == 'N' || B.base(j) == 'N') return 0;
    const float probC = probCorrect2[A.qual(i)] * probCorrect2[B.qual(j)];
    return 1 - probC;                                   // probE; `expected += probE`
}
// BBMergeOverlapper.probability (:728-785) with qualities
BBM_HD FilterSpan probability_span(int alen, int blen, int insert) {
    return filter_span(insert <= blen ? 0 : insert - blen, insert >= blen ? 0 : blen - insert, insert, alen, blen);
}
template <class SA, class SB> BBM_HD void probability_terms(const SA &A, const SB &B, int i, int j, const float *probCorrect2, float &common, float &actual) {
    const int ca = A.base(i), cb = B.base(j);
    common = 1; actual = 1;
    if (ca == 'N' || cb == 'N') return;
    const float probC = probCorrect2[A.qual(i)] * probCorrect2[B.qual(j)];
    const float probM = probC + (1 - probC) * 0.25f;
    const float probE = 1 - probM;
    common = fmax2(probM, probE);                       // `probCommon *= ...`
    actual = ca == cb ? probM : probE;                  // `probActual *= ...`
}
// :784: the quotient in float, the square root in double; a NaN (0 / 0 after both products underflow) comes back as Java's one NaN
BBM_HD float probability_of(float probActual, float probCommon) {
    const float q = probActual / probCommon;
    const float r = (float)sqrt((double)q);
    return r != r ? __builtin_nanf("") : r;
}
template <class SA, class SB> BBM_HD float expected_mismatches(const SA &A, const SB &B, int alen, int blen, int overlap, const float *probCorrect2) {
    const FilterSpan s = expected_span(alen, blen, overlap);
    float expected = 0;
    for (int c = 0; c < s.n; c++) expected += expected_term(A, B, s.istart + c, s.jstart + c, probCorrect2);
    return expected;
}
template <class SA, class SB> BBM_HD float merge_probability(const SA &A, const SB &B, int alen, int blen, int insert, const float *probCorrect2) {
    const FilterSpan s = probability_span(alen, blen, insert);
    float probActual = 1, probCommon = 1;
    for (int c = 0; c < s.n; c++) {
        float common, actual;
        probability_terms(A, B, s.istart + c, s.jstart + c, probCorrect2, common, actual);
        probCommon *= common; probActual *= actual;
    }
    return probability_of(probActual, probCommon);
}

BBM_HD void skipped_verdict(bbmerge_verdict_rec &v) {
    v.code = BBMERGE_RET_NO_SOLUTION; v.minOverlap = 0;
    v.insertRM = -1; v.badRM = 0; v.ambigRM = 0;
    v.insertNM = -1; v.badNM = 99999; v.ambigNM = 0;
    v.bad = 0; v.expected = 0; v.probability = 0; v.info = BBMERGE_INFO_SKIPPED;
}

// One pair.  E is where the pair lives (host arrays, or LDS and a wavefront): entropy_a() / entropy_b() the two scans, ratio<Q>(p, r)
// one ratio native, normal<Q>(p, bad, ambig) one normal-mode pass, expected(insert) and probability(insert) the filters.
template <class E> BBM_HD void verdict_of(E &e, const bbmerge_verdict_config &c, int alen, int blen, bool have_quality, bbmerge_verdict_rec &v) {
    int info = 0;
    v.expected = 0; v.probability = 0;
    // calcMinOverlapFromEntropy (:1696-1711)
    int minOverlap = c.minOverlapBases;
    if (c.useEntropy) {
        const int a = e.entropy_a(), b = e.entropy_b();
        minOverlap = imax(c.minOverlapBases, imax(a, b));
    }
    v.minOverlap = minOverlap;
    // :1765-1775, mateByOverlap_ratioMode (:1615-1639)
    int insertRM = -1, badRM = 0, ambigRM = 0;
    if (c.useRatioMode) {
        bbmerge_config rc = c.ratio;
        rc.minOverlap0 = c.minOverlapBases0 - c.ratioReduction; rc.minOverlap = minOverlap - c.ratioReduction;
        const Params p = params_of(rc);
        bbmerge_rec r = {-1, 0, 0, 0};
        const bool quality_form = runs_quality_form(c.ratio, have_quality);
        if (quality_form) {
            e.template ratio<true>(p, r);
            r.info |= BBMERGE_INFO_QUALITY;
        }
        if (runs_flat_form(c.ratio, quality_form, r)) {
            e.template ratio<false>(p, r);
            r.info |= BBMERGE_INFO_FLAT;
        }
        insertRM = r.insert; badRM = r.bad; ambigRM = insertRM > -1 ? r.ambig == 1 : 0;
        info |= r.info | BBMERGE_INFO_RATIO;
    }
    // :1777-1787, mateByOverlap_normalMode (:1641-1661, :1690-1693)
    int insertNM = -1, badNM = 99999, ambigNM = 0;
    if (c.useNormalMode && ((!c.requireRatioMatch && (insertRM < 0 || ambigRM)) || (c.requireRatioMatch && (insertRM > 0 && !ambigRM)))) {
        int best = -1, bestBad = 999999, ambig = 0;
        const int maxQualIters = have_quality ? c.qualIters : 1;
        for (int i = 0; i < maxQualIters && best < 0; i++) {
            const NormalParams p = normal_params(c, minOverlap, i, alen, blen);
            int bad = 0, amb = 0;
            const int x = have_quality ? e.template normal<true>(p, bad, amb) : e.template normal<false>(p, bad, amb);
            if (x > -1) { best = x; bestBad = bad; ambig = amb == 1; break; }
        }
        insertNM = best; badNM = bestBad; ambigNM = best > -1 ? ambig : 0;
        info |= BBMERGE_INFO_NORMAL;
    }
    v.insertRM = insertRM; v.badRM = badRM; v.ambigRM = ambigRM;
    v.insertNM = insertNM; v.badNM = badNM; v.ambigNM = ambigNM;
    // :1789-1809
    int ambig, bestBad, bestInsert;
    if (c.requireRatioMatch && c.useNormalMode && c.useRatioMode) {
        ambig = ambigRM || ambigNM; bestBad = badRM; bestInsert = insertNM == insertRM ? insertNM : -1;
    } else if (c.useRatioMode && insertRM > -1 && !ambigRM) {
        ambig = ambigRM; bestBad = badRM; bestInsert = insertRM;
    } else {
        ambig = ambigNM; bestBad = badNM; bestInsert = insertNM;
    }
    if (bestBad > c.maxMismatchesR) ambig = 1;
    v.bad = bestBad;
    // :1811-1836 (TAG_CUSTOM is false)
    int ret;
    if (ambig) {
        ret = BBMERGE_RET_AMBIG;
    } else if (bestInsert < 0) {
        ret = BBMERGE_RET_NO_SOLUTION;
    } else {
        if (have_quality) {
            if (c.useEfilter && bestInsert > 0 && !ambig) {
                const float bestExpected = e.expected(bestInsert);
                if ((bestExpected + c.efilterOffset) * c.efilterRatio < bestBad) ambig = 1;
                v.expected = bestExpected; info |= BBMERGE_INFO_EFILTER;
            }
            if (c.pfilterRatio > 0 && bestInsert > 0 && !ambig) {
                const float probability = e.probability(bestInsert);
                if (probability < c.pfilterRatio) bestInsert = -1;
                v.probability = probability; info |= BBMERGE_INFO_PFILTER;
            }
        }
        ret = ambig ? BBMERGE_RET_AMBIG : bestInsert > 0 ? bestInsert : BBMERGE_RET_NO_SOLUTION;
    }
    // processReadPair_inner (:2061-2067)
    if (ret > 0) {
        if (ret < c.ratio.minInsert) ret = BBMERGE_RET_SHORT;
        else if (c.maxLength > 0 && ret > c.maxLength) ret = BBMERGE_RET_LONG;
    }
    v.code = ret; v.info = info;
}

// what one verdict adds to bbmerge_stats (BBMerge.java:1402-1422); S::add / S::min / S::max say how
struct StatsDelta {
    int pairs, merged, ambiguous, tooShort, tooLong, noSolution, skipped;
    long long insertSum;
    int insertMin, insertMax;
    BBM_HD void clear() { pairs = merged = ambiguous = tooShort = tooLong = noSolution = skipped = 0; insertSum = 0; insertMin = 999999999; insertMax = 0; }
    BBM_HD void count(const bbmerge_verdict_rec &v) {
        pairs++;
        if (v.info & BBMERGE_INFO_SKIPPED) skipped++;
        else if (v.code > 0) { merged++; insertSum += v.code; insertMin = imin(insertMin, v.code); insertMax = imax(insertMax, v.code); }
        else if (v.code == BBMERGE_RET_AMBIG) ambiguous++;
        else if (v.code == BBMERGE_RET_SHORT) tooShort++;
        else if (v.code == BBMERGE_RET_LONG) tooLong++;
        else noSolution++;
    }
};

}  // namespace bbmerge
