// Device form of bbkeys_make_batch (keyring_host.hip): AbstractMapThread.quickMap up to the findAdvanced call, one read per lane.
//
// The host form is the reference and this file follows it operation by operation: every float step is the same single IEEE
// operation in the same order (the library is built with -ffp-contract=off -fno-fast-math and hipcc's correctly rounded fp32
// division), Math.round / Math.ceil work on doubles, and nothing here calls libm: the quality tables and the 128 base scores are
// built on the host by the shared code (keyring_shared.h) and uploaded once, and the one question asked of
// Read.avgQualityByProbability, `< 2`, becomes a comparison of p = sum / len with the float at which the host function flips.
//
// makeKeyProbs is a running float product, so a read's chain is serial: one read per lane, the batch hides the latency.
//   pass 1   walks the read once: base scores, the undefined count, the probability sum, and the key error probabilities.
//            KeyRing.makeOffsets3 asks two things of keyErrorProb[i]: `>= errorLimit1` (only to find left / right: kept as running
//            values) and `< errorLimit2` (one bit per position, in the workspace).
//   walk     makeOffsets3's placement loop over those bits; misses are dropped as they happen, offsets go to the read's slot in
//            a temporary buffer (its size bounded before the walk by desiredKeysFromDensity(len, k, keyDen2, 2)).
//   pass 2   the chosen offsets ascend, so a second run of the same chain picks up the float at each of them for the key score
//            and probAllErrors.
// Bases, qualities and base scores are one byte per base: they are read and written as aligned 8-byte words, never byte by byte.
// Placement: exclusive sums (hipcub) of the slot bounds, of the lengths (they place the bit words) and finally of 2 * nkeys; the
// pack kernel then lays keyinfo out in read order exactly as the host form does.  No atomics.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <mutex>

#include "bbmap_amd.h"
#include "host_common.h"
#include "keyring_shared.h"

namespace bbkeys {

struct DevTables {                       // what the kernel copies to LDS
    float probError[128], probCorrect[128], probCorrectInverse[128];
    int baseScore[128];                  // makeByteScoreArray(quality, 100, out, negative=true): round(100 * probCorrect[q]) - 100
};
__device__ DevTables g_tables;

struct ToLL { __host__ __device__ long long operator()(int v) const { return (long long)v; } };

// p[0], p[1], ... in ascending order, fetched as the aligned 8-byte words that hold them.  A word is loaded only when one of its
// bytes is asked for, so nothing beyond the aligned words that overlap the read is touched.
struct ByteReader {
    const unsigned long long *wp;
    unsigned long long w;
    int sh;
    __device__ void seek(const uint8_t *p) {
        const uintptr_t a = (uintptr_t)p;
        wp = (const unsigned long long *)(a & ~(uintptr_t)7) - 1;
        sh = 64 + (int)(a & 7) * 8;
        w = 0;
    }
    __device__ int next() {
        if (sh >= 64) { sh -= 64; w = *++wp; }
        const int b = (int)((w >> sh) & 255);
        sh += 8;
        return b;
    }
};

// out[0], out[1], ... in ascending order: whole aligned words where all eight bytes are this read's, single bytes at its edges
// (the neighbouring bytes belong to other reads, or to nobody)
struct ByteWriter {
    uint8_t *p;
    unsigned long long w;
    int n;                               // bytes gathered in w
    __device__ void seek(uint8_t *out) { p = out; w = 0; n = 0; }
    __device__ void flush() {
        if (n == 8) *(unsigned long long *)(p - 8) = w;
        else for (int i = 0; i < n; i++) p[i - n] = (uint8_t)(w >> (8 * i));
        w = 0; n = 0;
    }
    __device__ void put(int v) {
        w |= (unsigned long long)(v & 255) << (8 * n);
        n++; p++;
        if (((uintptr_t)p & 7) == 0) flush();
    }
};

// QualityTools.makeKeyProbs(quality, bases, keylen, out, useModulo=false) :188-247 / :250-279, one base at a time: feed(i, q)
// for i = 0 .. len - 1 returns keyErrorProb[i - keylen + 1] once i >= keylen - 1
struct KeyChain {
    float key1;
    int timeSinceZero;
    ByteReader qa;                       // quality[a], keylen bases behind
    __device__ void start(const uint8_t *quality) { key1 = 1; timeSinceZero = 0; qa.seek(quality); }
    __device__ float feed(int i, int q, int keylen, const DevTables &T) {
        if (q > 0) timeSinceZero++; else timeSinceZero = 0;
        if (i < keylen) key1 *= T.probCorrect[q];
        else key1 = key1 * T.probCorrectInverse[qa.next() & 127] * T.probCorrect[q];
        float out = 1 - key1;
        if (timeSinceZero < keylen) out = 1;
        return out;
    }
};

// the density window of AbstractMapThread.java:663-676, as bbkeys_make states it
__device__ inline float key_density2(const bbkeys_config &c, int len) {
    const int K = c.k;
    float keyDen2 = ((c.maxDesiredKeys * K) / (float)len);
    keyDen2 = keyDen2 > c.minKeyDensity ? keyDen2 : c.minKeyDensity;
    const float m = c.keyDensity < keyDen2 ? c.keyDensity : keyDen2;
    return m < (float)K ? m : (float)K;
}
__device__ inline float key_density3(const bbkeys_config &c, int len) {
    const int K = c.k;
    float keyDen3;
    if (len <= 50) keyDen3 = c.maxKeyDensity;
    else if (len >= 200) keyDen3 = c.maxKeyDensity - 0.5f;
    else keyDen3 = c.maxKeyDensity - 0.003333333333f * (len - 50);
    keyDen3 = keyDen3 > c.keyDensity ? keyDen3 : c.keyDensity;
    return keyDen3 < (float)K ? keyDen3 : (float)K;
}

// per read: the slots it can need in the temporary key buffer (what makeOffsets3 starts from; misses and the later tests only
// shrink it) and its length, both to be summed
__global__ void bbkeys_bound_kernel(bbkeys_config cfg, long long n, const bbidx_read *reads, int *bound, int *lens) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    int b = 0, len = 0;
    if (r < n) {
        len = imax(reads[r].len, 0);
        if (len >= cfg.k) b = desired_keys_from_density(len, cfg.k, key_density2(cfg, len), 2);
    }
    bound[r] = b; lens[r] = len;         // entry n is the zero that makes the scan's last output the total
}

struct KeyArgs {
    bbkeys_config cfg;
    long long n;
    const bbidx_read *reads;
    const uint8_t *bases, *quality;
    int8_t *baseScores;
    const long long *slotOff, *lenOff;   // exclusive sums of the slot bounds / the lengths, n + 1 entries
    long long slotCap, wordCap;
    int *tmpOffsets, *tmpScores;
    unsigned *bits;
    int *nkeys2;                         // 2 * nkeys per read, entry n = 0
    int *tooSmall;                       // set when a read's slots or words do not fit the workspace
    float avgQualityFlip;                // avgQualityByProbability < 2  <=>  sum / len >= this
};

__global__ void __launch_bounds__(256) bbkeys_make_kernel(KeyArgs A) {
    __shared__ DevTables T;
    for (int i = threadIdx.x; i < (int)(sizeof(DevTables) / 4); i += blockDim.x) ((int *)&T)[i] = ((const int *)&g_tables)[i];
    __syncthreads();
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > A.n) return;
    if (r == A.n) { A.nkeys2[r] = 0; return; }
    const int K = A.cfg.k;
    const int len = A.reads[r].len;
    const long long off = A.reads[r].bases_off;
    const uint8_t *quality = A.quality ? A.quality + off : nullptr;
    const int nprob = len - K + 1;
    // a read's `< errorLimit2` bits take (nprob + 31) / 32 <= len / 32 + 1 words: lenOff / 32 + r leaves every read that room
    const long long slot0 = A.slotOff[r], word0 = A.lenOff[r] / 32 + r;
    const bool fits = A.slotOff[r + 1] <= A.slotCap && A.lenOff[r + 1] / 32 + r + 1 <= A.wordCap;
    if (!fits) *A.tooSmall = 1;
    unsigned *bits = A.bits + word0;
    const float errorLimit2 = 0.9999f, errorLimit1 = A.cfg.semiperfectMode ? 0.99f : 0.94f;

    // ---- pass 1: base scores, undefined bases, sum of error probabilities, key error probabilities as left / right / bits
    int undefined = 0, left = -1, right = -1, potentialKeys = 0, seen = 0;
    float sum = 0;
    if (len > 0) {
        ByteReader B, Q;
        ByteWriter W;
        KeyChain C;
        B.seek(A.bases + off);
        W.seek((uint8_t *)A.baseScores + off);
        if (quality) { Q.seek(quality); C.start(quality); }
        unsigned acc = 0;
        for (int i = 0; i < len; i++) {
            const int b = B.next();
            const bool def = fully_defined(b);
            if (!def) undefined++;
            if (!quality) { W.put(0); continue; }
            const int q = Q.next() & 127;
            W.put(T.baseScore[q]);
            if (def) sum += T.probError[q];
            const float prob = C.feed(i, q, K, T);
            const int p = i - K + 1;
            if (p < 0) continue;
            const bool usable = prob < errorLimit2;
            if (!(prob >= errorLimit1)) {        // the two `while` loops of makeOffsets3: first and last position below errorLimit1
                if (left < 0) left = p;
                right = p;
            }
            if (left >= 0 && usable) seen++;
            if (right == p) potentialKeys = seen;
            if (usable) acc |= 1u << (p & 31);
            if ((p & 31) == 31 || p == nprob - 1) { if (fits) bits[p >> 5] = acc; acc = 0; }
        }
        W.flush();
    }
    if (!quality && nprob > 0) { left = 0; right = nprob - 1; potentialKeys = nprob; }     // every probability is 0

    // ---- the tests of bbkeys_make that need no keys
    bool live = fits && len >= K;
    if (A.cfg.semiperfectMode ? undefined > 0 : (undefined > 25 && len - undefined < undefined)) live = false;
    if (left < 0 || potentialKeys == 0 || right < left) live = false;
    if (quality && len > 0 && sum / len >= A.avgQualityFlip) live = false;
    int n = 0;
    int *offsets = A.tmpOffsets + slot0, *scores = A.tmpScores + slot0;

    // ---- KeyRing.makeOffsets3 :396-506 from `readlen = right - left + blocksize` on
    if (live) {
        const int maxProbIndex = len - K;
        const int readlen = right - left + K;
        const float density = key_density2(A.cfg, len), maxDensity = key_density3(A.cfg, len);
        int desiredKeys = desired_keys_from_density(len, K, density, 2);
        if (readlen < len) desiredKeys = imin(desiredKeys, desired_keys_from_density(readlen, K, maxDensity, 2));
        desiredKeys = imin(desiredKeys, potentialKeys);
        const float interval = (right - left) / (float)imax(desiredKeys - 1, 1);
        const int intervalInt = ((int)interval) + 1;
        float f = (float)left;
        int prev = -1;
        int wordAt = -1;
        unsigned word = 0;
        auto usable = [&](int i) -> bool {
            if (!quality) return true;
            if ((i >> 5) != wordAt) { wordAt = i >> 5; word = bits[wordAt]; }
            return (word >> (i & 31)) & 1;
        };
        for (int i = 0, j = left; i < desiredKeys; i++) {
            int x = -1;
            if (prev < j) {
                if (usable(j) && (prev < 0 || j - prev > 0)) x = j;
                else {
                    for (int k = j - 1, lim = prev + 2; k > lim; k--) if (usable(k)) { x = k; break; }
                    if (x < 0) for (int k = j + 1, lim = imin(j + intervalInt, right); k < lim; k++) if (usable(k)) { x = k; break; }
                }
            }
            if (x > -1) { offsets[n++] = x; prev = x; }
            else prev = imax(prev, j - 2);
            f += interval;
            j = imin(maxProbIndex, imax(j + 1, java_round(f)));
        }
        if (n == 0 || n < A.cfg.minApproxHitsToKeep) n = 0;
    }

    // ---- pass 2: makeKeyScores :712-724 -- the chain again, as far as the last offset, taking the probability at each offset
    if (n > 0) {
        const int a = 100 * K, baseKeyScore = a / 8, range = a - baseKeyScore;
        float probAllErrors = 1.0f;
        if (!quality) {
            for (int m = 0; m < n; m++) { scores[m] = baseKeyScore + java_round(range * (1 - 0.0f)); probAllErrors *= 0.0f; }
        } else {
            ByteReader Q;
            KeyChain C;
            Q.seek(quality); C.start(quality);
            int m = 0, want = offsets[0];
            for (int i = 0; m < n; i++) {
                const float p = C.feed(i, Q.next() & 127, K, T);
                if (i - K + 1 != want) continue;
                scores[m] = baseKeyScore + java_round(range * (1 - p));
                probAllErrors *= p;
                if (++m < n) want = offsets[m];
            }
        }
        if (probAllErrors > 0.50f) n = 0;
    }
    A.nkeys2[r] = 2 * n;
}

// keyinfo in the host form's layout: offsets[nkeys] then keyScores[nkeys] per read at keys_off = the exclusive sum of 2 * nkeys
__global__ void bbkeys_pack_kernel(long long n, bbidx_read *reads, const long long *slotOff, const long long *keyOff, const int *nkeys2,
                                   const int *tmpOffsets, const int *tmpScores, int *keyinfo) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int nk = nkeys2[r] >> 1;
    const long long ko = keyOff[r], so = slotOff[r];
    reads[r].keys_off = ko; reads[r].nkeys = nk;
    for (int i = 0; i < nk; i++) { keyinfo[ko + i] = tmpOffsets[so + i]; keyinfo[ko + nk + i] = tmpScores[so + i]; }
}

// ---------------------------------------------------------------------------------------------------------------- host side
static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {                          // byte offsets into the caller's workspace; everything up to `bits` follows from n alone
    size_t bound, lens, nkeys2, slotOff, lenOff, keyOff, flag, scanTmp, scanTmpBytes, bits, tmpOffsets, tmpScores, total;
    long long slotCap, wordCap;
};

// sizes that hold for any batch of n reads with total_bases bases in all: a read's slots are at most
// max(2, ceil(len * keyDen2 / k)) with keyDen2 <= keyDensity, and at most len; its bit words at most len / 32 + 1
static int make_layout(const bbkeys_config *cfg, long long n, long long total_bases, Layout &L) {
    // room for hipcub's scan of n + 1 long long sums (it is asked for its real need when the pointers exist, at the call): its state is a
    // few words per block of at least 256 items
    const size_t scan = 64 * ((size_t)(n + 1) / 256 + 64) + 4096;
    const double perBase = (double)cfg->keyDensity / (double)cfg->k;
    long long slots = 3 * n + (long long)ceil((double)total_bases * perBase * 1.001) + 64;
    if (slots > total_bases) slots = total_bases;
    L.slotCap = slots;
    L.wordCap = total_bases / 32 + n;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
    L.bound = take(4 * (size_t)(n + 1)); L.lens = take(4 * (size_t)(n + 1)); L.nkeys2 = take(4 * (size_t)(n + 1));
    L.slotOff = take(8 * (size_t)(n + 1)); L.lenOff = take(8 * (size_t)(n + 1)); L.keyOff = take(8 * (size_t)(n + 1));
    L.flag = take(4);
    L.scanTmpBytes = scan; L.scanTmp = take(scan);
    L.bits = take(4 * (size_t)L.wordCap);
    L.tmpOffsets = take(4 * (size_t)L.slotCap); L.tmpScores = take(4 * (size_t)L.slotCap);
    L.total = o;
    return BBMAP_OK;
}

static bool good_config(const bbkeys_config *cfg) {
    return cfg && cfg->k >= 1 && cfg->keyDensity >= 0 && cfg->keyDensity < 1e6f;      // (also refuses a NaN density)
}

// the float at which avg_quality_from_p(p) < 2 starts to hold: the function does not increase with p, and non-negative floats
// order as their bit patterns do
static float avg_quality_flip() {
    uint32_t lo = 0, hi = 0x40000000u;   // 0.0f (quality 60) .. 2.0f (quality 0)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float p;
        memcpy(&p, &mid, 4);
        if (avg_quality_from_p(p) < 2) hi = mid; else lo = mid + 1;
    }
    float p;
    memcpy(&p, &lo, 4);
    return p;
}

// once per process and device: the gfx950 check and the upload of the tables
static int prepare_device(float &flip) {
    static std::mutex mu;
    static bool ready[64];
    static float flipValue;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;       // (a machine without a device: the check below says so)
    if (dev < 0 || dev >= 64) return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: device ordinal beyond 63");
    std::lock_guard<std::mutex> lock(mu);
    if (!ready[dev]) {
        BBTRY(bb_use_gfx950("bbkeys_make_batch_device", dev));
        static DevTables h;
        const QualTables &T = tables();
        for (int i = 0; i < 128; i++) {
            h.probError[i] = T.probError[i]; h.probCorrect[i] = T.probCorrect[i]; h.probCorrectInverse[i] = T.probCorrectInverse[i];
            h.baseScore[i] = (int8_t)(java_round(100 * T.probCorrect[i]) - 100);
        }
        BBHIP(hipMemcpyToSymbol(HIP_SYMBOL(g_tables), &h, sizeof h));
        flipValue = avg_quality_flip();
        ready[dev] = true;
    }
    flip = flipValue;
    return BBMAP_OK;
}

}  // namespace bbkeys

extern "C" int64_t bbkeys_device_workspace_bytes(const bbkeys_config *cfg, int64_t n_reads, int64_t total_bases) {
    if (!bbkeys::good_config(cfg) || n_reads < 0 || n_reads >= 0x7fffffff || total_bases < 0) return bbfail(BBMAP_E_ARG, "bbkeys_device_workspace_bytes: bad argument");
    bbkeys::Layout L;
    const int rc = bbkeys::make_layout(cfg, n_reads, total_bases, L);
    return rc != BBMAP_OK ? rc : (int64_t)L.total;
}

extern "C" int bbkeys_make_batch_device(const bbkeys_config *cfg, void *stream_, int64_t n_reads, bbidx_read *reads,
                                        const uint8_t *bases, const uint8_t *quality, int32_t *keyinfo, int64_t keyinfo_cap,
                                        int8_t *baseScores, void *workspace, int64_t workspace_bytes, int64_t *keyinfo_used) {
    using namespace bbkeys;
    if (!good_config(cfg) || n_reads < 0 || n_reads >= 0x7fffffff || keyinfo_cap < 0 || workspace_bytes < 0 || !keyinfo_used ||
        (n_reads > 0 && (!reads || !bases || !keyinfo || !baseScores || !workspace)))
        return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: bad argument");
    if (((uintptr_t)workspace & 255) != 0) return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: the workspace must be 256-byte aligned");
    float flip = 0;
    const int prc = prepare_device(flip);
    if (prc != BBMAP_OK) return prc;
    *keyinfo_used = 0;
    if (n_reads == 0) return BBMAP_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const long long n = n_reads;
    // The lengths live on the device, so the check comes in two parts: what follows from n_reads alone here, before anything is
    // launched, and the rest once the lengths have been summed (into that first part), before the key kernel runs.
    Layout L;
    int rc = make_layout(cfg, n, 0, L);
    if (rc != BBMAP_OK) return rc;
    if ((size_t)workspace_bytes < L.total) return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: workspace too small (bbkeys_device_workspace_bytes)");
    char *ws = (char *)workspace;
    auto I = [&](size_t at) { return (int *)(ws + at); };
    auto LL = [&](size_t at) { return (long long *)(ws + at); };
    const dim3 grid((unsigned)((n + 1 + 255) / 256)), block(256);
    auto wideBound = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)I(L.bound), ToLL());
    auto wideLens = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)I(L.lens), ToLL());
    auto wideKeys = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)I(L.nkeys2), ToLL());
    size_t scanBytes = 0;
    BBHIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, wideBound, LL(L.slotOff), (int)(n + 1), stream));
    if (scanBytes > L.scanTmpBytes) return bbfail(BBMAP_E_HIP, "bbkeys_make_batch_device: hipcub's scan asks for more temporary storage than the workspace reserves");
    hipLaunchKernelGGL(bbkeys_bound_kernel, grid, block, 0, stream, *cfg, n, (const bbidx_read *)reads, I(L.bound), I(L.lens));
    BBHIP(hipGetLastError());
    BBHIP(hipcub::DeviceScan::ExclusiveSum(ws + L.scanTmp, scanBytes, wideBound, LL(L.slotOff), (int)(n + 1), stream));
    BBHIP(hipcub::DeviceScan::ExclusiveSum(ws + L.scanTmp, scanBytes, wideLens, LL(L.lenOff), (int)(n + 1), stream));
    long long totals[2] = {0, 0};        // {slots, bases}
    BBHIP(hipMemcpyAsync(&totals[0], LL(L.slotOff) + n, 8, hipMemcpyDeviceToHost, stream));
    BBHIP(hipMemcpyAsync(&totals[1], LL(L.lenOff) + n, 8, hipMemcpyDeviceToHost, stream));
    BBHIP(hipStreamSynchronize(stream));
    rc = make_layout(cfg, n, totals[1], L);
    if (rc != BBMAP_OK) return rc;
    if ((size_t)workspace_bytes < L.total || totals[0] > L.slotCap)
        return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: workspace too small for the bases of these reads (bbkeys_device_workspace_bytes)");

    KeyArgs A;
    A.cfg = *cfg; A.n = n; A.reads = reads; A.bases = bases; A.quality = quality; A.baseScores = baseScores;
    A.slotOff = LL(L.slotOff); A.lenOff = LL(L.lenOff); A.slotCap = L.slotCap; A.wordCap = L.wordCap;
    A.tmpOffsets = I(L.tmpOffsets); A.tmpScores = I(L.tmpScores); A.bits = (unsigned *)(ws + L.bits);
    A.nkeys2 = I(L.nkeys2); A.tooSmall = I(L.flag); A.avgQualityFlip = flip;
    BBHIP(hipMemsetAsync(ws + L.flag, 0, 4, stream));
    hipLaunchKernelGGL(bbkeys_make_kernel, grid, block, 0, stream, A);
    BBHIP(hipGetLastError());
    BBHIP(hipcub::DeviceScan::ExclusiveSum(ws + L.scanTmp, scanBytes, wideKeys, LL(L.keyOff), (int)(n + 1), stream));
    long long used = 0;
    int tooSmall = 0;
    BBHIP(hipMemcpyAsync(&used, LL(L.keyOff) + n, 8, hipMemcpyDeviceToHost, stream));
    BBHIP(hipMemcpyAsync(&tooSmall, ws + L.flag, 4, hipMemcpyDeviceToHost, stream));
    BBHIP(hipStreamSynchronize(stream));
    if (tooSmall) return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: a read's keys did not fit the workspace");
    *keyinfo_used = used;
    if (used > keyinfo_cap) return bbfail(BBMAP_E_ARG, "bbkeys_make_batch_device: keyinfo buffer too small (*keyinfo_used = the size needed)");
    hipLaunchKernelGGL(bbkeys_pack_kernel, grid, block, 0, stream, n, reads, (const long long *)LL(L.slotOff), (const long long *)LL(L.keyOff),
                       (const int *)I(L.nkeys2), (const int *)I(L.tmpOffsets), (const int *)I(L.tmpScores), keyinfo);
    BBHIP(hipGetLastError());
    BBHIP(hipStreamSynchronize(stream));
    return BBMAP_OK;
}
