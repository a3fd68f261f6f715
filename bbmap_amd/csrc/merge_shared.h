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

}  // namespace bbmerge
