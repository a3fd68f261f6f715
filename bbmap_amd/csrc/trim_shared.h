// What the host and the device form of the trim stage share (trim.hip): align2.TrimRead.trim for one read, over any reader of the
// read's bytes.  One copy, so that the two forms cannot drift apart.  Every float step is one IEEE single-precision operation in
// Java's order (the library is built with -ffp-contract=off -fno-fast-math); the error probability table is the caller's
// (bbkeys::tables().probError on the host, a copy of it on the device), so nothing here calls libm.
#pragma once
#include <cstdint>

#include "bbmap_amd.h"

#if defined(__HIPCC__)
#define BBTRIM_HD __host__ __device__
#else
#define BBTRIM_HD
#endif

namespace bbtrim {

// A reader R gives R::get(i) = byte i of the read (bases or qualities), 0 <= i < len, in any order.

// TrimRead.testLeftN / testRightN :388-413
template <class R> BBTRIM_HD inline int test_left_n(R &B, int len, int minGoodInterval) {
    int good = 0, lastBad = -1;
    for (int i = 0; i < len && good < minGoodInterval; i++) {
        if (B.get(i) != 'N') good++;
        else { good = 0; lastBad = i; }
    }
    return lastBad + 1;
}
template <class R> BBTRIM_HD inline int test_right_n(R &B, int len, int minGoodInterval) {
    int good = 0, lastBad = len;
    for (int i = len - 1; i >= 0 && good < minGoodInterval; i--) {
        if (B.get(i) != 'N') good++;
        else { good = 0; lastBad = i; }
    }
    return len - lastBad;
}

// TrimRead.testOptimal :264-324
template <class R> BBTRIM_HD inline void test_optimal(const bbtrim_config &c, const float *probError, R &B, R &Q, bool hasQual, int len,
                                                      int &left, int &right) {
    float avgErrorRate = probError[c.trimq & 127];
    if (c.optimalBias >= 0) avgErrorRate = c.optimalBias;
    left = right = 0;
    if (len == 0) return;
    if (!hasQual) {
        if (!(avgErrorRate >= 1)) { left = test_left_n(B, len, c.minGoodInterval); right = test_right_n(B, len, c.minGoodInterval); }
        return;
    }
    float maxScore = 0, score = 0;
    int maxLoc = -1, maxCount = -1, count = 0;
    float nprob = avgErrorRate * 1.1f;
    nprob = nprob < 1.0f ? nprob : 1.0f;
    nprob = nprob > 0.75f ? nprob : 0.75f;
    for (int i = 0; i < len; i++) {
        const int b = B.get(i), q = Q.get(i);
        const float pe = b == 'N' ? nprob : probError[q & 127];
        const float delta = avgErrorRate - pe;
        score = score + delta;
        if (score > 0) {
            count++;
            if (score > maxScore || (score == maxScore && count > maxCount)) { maxScore = score; maxCount = count; maxLoc = i; }
        } else { score = 0; count = 0; }
    }
    if (maxScore > 0) { left = maxLoc - maxCount + 1; right = len - maxLoc - 1; }
    else { left = 0; right = len; }
}

// TrimRead.testRightWindow :349-365.  Q2 is a second reader of the qualities: it trails Q by `window` bytes.
template <class R> BBTRIM_HD inline int test_right_window(const bbtrim_config &c, R &B, R &Q, R &Q2, bool hasQual, int len) {
    const int window = c.windowLength;
    if (len == 0) return 0;
    if (!hasQual || len < window) return c.trimq > 0 ? 0 : test_right_n(B, len, c.minGoodInterval);
    const int t = window * c.trimq, thresh = t > 1 ? t : 1;
    int sum = 0;
    for (int i = 0, j = -window; i < len; i++, j++) {
        sum += Q.get(i);
        if (j >= -1) {
            if (j >= 0) sum -= Q2.get(j);
            if (sum < thresh) return len - j - 1;
        }
    }
    return 0;
}

// TrimRead.testLeft / testRight :327-385 (trimq >= 0, so a read without qualities takes the N-only scan)
template <class R> BBTRIM_HD inline int test_left(const bbtrim_config &c, R &B, R &Q, bool hasQual, int len) {
    if (len == 0) return 0;
    if (!hasQual) return test_left_n(B, len, c.minGoodInterval);
    int good = 0, lastBad = -1;
    for (int i = 0; i < len && good < c.minGoodInterval; i++) {
        if (Q.get(i) > c.trimq) good++;
        else { good = 0; lastBad = i; }
    }
    return lastBad + 1;
}
template <class R> BBTRIM_HD inline int test_right(const bbtrim_config &c, R &B, R &Q, bool hasQual, int len) {
    if (len == 0) return 0;
    if (!hasQual) return test_right_n(B, len, c.minGoodInterval);
    int good = 0, lastBad = len;
    for (int i = len - 1; i >= 0 && good < c.minGoodInterval; i--) {
        if (Q.get(i) > c.trimq) good++;
        else { good = 0; lastBad = i; }
    }
    return len - lastBad;
}

// TrimRead.trim(Read, trimLeft, trimRight, trimq, minlen) :47-63 and the constructor's clamp, trim(int, int, int) :164-197.
// left / right = leftTrimmed / rightTrimmed; both 0 when Java returns null or the clamp leaves nothing.
template <class R> BBTRIM_HD inline void trim_read(const bbtrim_config &c, const float *probError, R &B, R &Q, R &Q2, bool hasQual, int len,
                                                   int &left, int &right) {
    int a = 0, b = 0;
    if (len > 0) {
        if (c.mode == BBTRIM_MODE_OPTIMAL) {
            test_optimal(c, probError, B, Q, hasQual, len, a, b);
            if (!c.trimLeft) a = 0;
            if (!c.trimRight) b = 0;
        } else if (c.mode == BBTRIM_MODE_WINDOW) {
            b = c.trimRight ? test_right_window(c, B, Q, Q2, hasQual, len) : 0;
        } else {
            a = c.trimLeft ? test_left(c, B, Q, hasQual, len) : 0;
            b = c.trimRight ? test_right(c, B, Q, hasQual, len) : 0;
        }
    }
    if (a + b > 0) {
        const int minlen = c.minLength > 0 ? c.minLength : 0;
        const int maxTrim = len < len - minlen ? len : len - minlen;
        if (a + b > maxTrim) {
            int excess = a + b - maxTrim;
            if (a > 0 && excess > 0) { a = a - excess > 0 ? a - excess : 0; excess = a + b - maxTrim; }
            if (b > 0 && excess > 0) { b = b - excess > 0 ? b - excess : 0; }
        }
    }
    left = a; right = b;
}

BBTRIM_HD inline bool good_config(const bbtrim_config &c) {
    return c.mode >= BBTRIM_MODE_OPTIMAL && c.mode <= BBTRIM_MODE_INTERVAL && c.trimq >= 0 && c.trimq <= 126 && c.windowLength >= 1 &&
           c.minGoodInterval >= 1 && c.optimalBias <= 1.0f;          // (also refuses a NaN bias)
}

}  // namespace bbtrim
