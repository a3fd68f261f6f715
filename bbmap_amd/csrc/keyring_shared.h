// What the host and the device form of quickMap's key stage share (keyring_host.hip, keyring_device.hip): the quality tables, the
// Java rounding helpers and the pieces of KeyRing / Read that both restate.  One copy, so that the two forms cannot drift apart.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BBKEYS_HD __host__ __device__
#else
#define BBKEYS_HD
#endif

namespace bbkeys {

struct QualTables {
    float probError[128], probCorrect[128], probCorrectInverse[128];
    QualTables() {                                      // QualityTools.java:475-480, :519-539
        for (int i = 0; i < 128; i++) probError[i] = (float)pow(10.0, 0 - .1 * i);
        probError[0] = .8f;
        for (int i = 0; i < 128; i++) { probCorrect[i] = 1 - probError[i]; probCorrectInverse[i] = 1 / probCorrect[i]; }
    }
};
inline const QualTables &tables() { static const QualTables t; return t; }

BBKEYS_HD inline int java_round(float f) { return (int)floor((double)f + 0.5); }          // Math.round(float)
BBKEYS_HD inline int imin(int a, int b) { return a < b ? a : b; }
BBKEYS_HD inline int imax(int a, int b) { return a > b ? a : b; }
BBKEYS_HD inline bool fully_defined(int b) { const int u = b & ~32; return b < 128 && (u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U'); }

// KeyRing.desiredKeysFromDensity :269-282
BBKEYS_HD inline int desired_keys_from_density(int readlen, int blocksize, float density, int minKeysDesired) {
    const int slots = readlen - blocksize + 1;
    int desired = (int)ceil((double)((readlen * density) / blocksize));
    desired = imax(minKeysDesired, desired);
    return imin(slots, desired);
}

// The tail of Read.avgQualityByProbability(false, 0) from p = expectedErrors / length on (current/stream/Read.java:1738-1745,
// QualityTools.java:497-517).  Host only: log10 on a double.
inline int avg_quality_from_p(float p) {
    const double prob = 1 - (double)(1 - p);
    double phred;
    if (prob >= 1) phred = 0; else if (prob <= 0.000001) phred = 60; else phred = -10 * log10(prob);
    const long q = (long)floor(phred + 0.5);
    return (int)(q < 0 ? 0 : (q > 41 ? 41 : q));          // Read.MAX_CALLED_QUALITY = 41; only `< 2` is ever asked of this value here
}

}  // namespace bbkeys
