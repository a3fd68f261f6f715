// The trim stage: align2.TrimRead.trim as AbstractMapThread.run applies it before processRead (current/align2/AbstractMapThread.java:
// 484-487), over a batch.  A read is (bases_off, len) into a blob, so trimming moves no base: the stage writes a second read array
// whose records start `left` bytes later and are left + right shorter, and the (left, right) pairs that bbmap_untrim_batch_device
// takes back (untrim.hip).
//
// Two forms of one per-read function (trim_shared.h): bbtrim_batch, plain C++ over host arrays, and bbtrim_batch_device, one read per
// lane.  testOptimal's score is a chain of float adds in read order with a reset in the middle: it is sequential by definition and
// stays so (a parallel scan would add in another order and round differently); the batch hides the latency, as in the key stage.
// A read's bytes come in as the aligned 8-byte words that hold them, one load per word and reader.  The 128 error probabilities are
// built on the host by the key stage's shared code (keyring_shared.h) and travel as a kernel argument: the call allocates nothing,
// copies nothing and does not wait.
#include <hip/hip_runtime.h>

#include <mutex>

#include "bbmap_amd.h"
#include "host_common.h"
#include "keyring_shared.h"
#include "trim_shared.h"

namespace bbtrim {

struct ProbTable { float v[128]; };

// byte i of a read on the host
struct HostBytes {
    const uint8_t *p;
    int get(int i) const { return p[i]; }
};

// byte i of a read on the device, fetched as the aligned 8-byte word that holds it; the word is kept, so a scan in either
// direction loads each word once.  Nothing beyond the aligned words that overlap the read is touched.
struct WordBytes {
    const uint8_t *p;
    uintptr_t at;                        // address of the word held (0 = none)
    unsigned long long w;
    __device__ void seek(const uint8_t *q) { p = q; at = 0; w = 0; }
    __device__ int get(int i) {
        const uintptr_t a = (uintptr_t)(p + i), wa = a & ~(uintptr_t)7;
        if (wa != at) { at = wa; w = *(const unsigned long long *)wa; }
        return (int)((w >> ((a & 7) * 8)) & 255);
    }
};

__global__ void __launch_bounds__(256) bbtrim_kernel(bbtrim_config cfg, ProbTable table, long long n, const bbidx_read *reads_in,
                                                     const uint8_t *bases, const uint8_t *quality, bbidx_read *reads_out, bbtrim_rec *trims) {
    __shared__ float probError[128];
    if (threadIdx.x < 128) probError[threadIdx.x] = table.v[threadIdx.x];
    __syncthreads();
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const bbidx_read in = reads_in[r];
    const int len = in.len > 0 ? in.len : 0;
    WordBytes B, Q, Q2;
    B.seek(bases + in.bases_off);
    Q.seek(quality ? quality + in.bases_off : bases);
    Q2.seek(quality ? quality + in.bases_off : bases);
    int left = 0, right = 0;
    trim_read(cfg, probError, B, Q, Q2, quality != nullptr, len, left, right);
    bbidx_read out;
    out.bases_off = in.bases_off + left; out.keys_off = 0; out.len = in.len - left - right; out.nkeys = 0;
    reads_out[r] = out;
    bbtrim_rec t; t.left = left; t.right = right;
    trims[r] = t;
}

static int check_args(const char *who, const bbtrim_config *cfg, int64_t n_reads, const bbidx_read *reads_in, const uint8_t *bases,
                      const bbidx_read *reads_out, const bbtrim_rec *trims) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "%s: null config", who);
    if (n_reads < 0 || n_reads >= 0x7fffffff) return bbfail(BBMAP_E_ARG, "%s: bad read count", who);
    if (!good_config(*cfg))
        return bbfail(BBMAP_E_ARG, "%s: bad config (mode 0..2, trimq 0..126, windowLength >= 1, minGoodInterval >= 1, optimalBias <= 1)", who);
    if (n_reads > 0 && (!reads_in || !bases || !reads_out || !trims)) return bbfail(BBMAP_E_ARG, "%s: null buffer", who);
    if (n_reads > 0) {
        const char *a = (const char *)reads_in, *b = (const char *)reads_out;
        const size_t bytes = (size_t)n_reads * sizeof(bbidx_read);
        if (a < b + bytes && b < a + bytes) return bbfail(BBMAP_E_ARG, "%s: reads_out must not alias reads_in", who);
    }
    return BBMAP_OK;
}

// once per process and device: the gfx950 check
static int prepare_device() {
    static std::mutex mu;
    static bool ready[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;       // (a machine without a device: the check below says so)
    if (dev < 0 || dev >= 64) return bbfail(BBMAP_E_ARG, "bbtrim_batch_device: device ordinal beyond 63");
    std::lock_guard<std::mutex> lock(mu);
    if (!ready[dev]) {
        BBTRY(bb_use_gfx950("bbtrim_batch_device", dev));
        ready[dev] = true;
    }
    return BBMAP_OK;
}

}  // namespace bbtrim

extern "C" int bbtrim_default_config(bbtrim_config *cfg) {
    if (!cfg) return bbfail(BBMAP_E_ARG, "bbtrim_default_config: null argument");
    cfg->mode = BBTRIM_MODE_OPTIMAL;                // TrimRead.optimalMode = true
    cfg->trimLeft = cfg->trimRight = 0;
    cfg->trimq = 6;                                 // Parser.java:930
    cfg->minLength = 60;                            // AbstractMapper.java:2720
    cfg->windowLength = 4; cfg->minGoodInterval = 2; cfg->optimalBias = -1.0f;
    return BBMAP_OK;
}

extern "C" int bbtrim_batch(const bbtrim_config *cfg, int64_t n_reads, const bbidx_read *reads_in, const uint8_t *bases,
                            const uint8_t *quality, bbidx_read *reads_out, bbtrim_rec *trims) {
    using namespace bbtrim;
    BBTRY(check_args("bbtrim_batch", cfg, n_reads, reads_in, bases, reads_out, trims));
    const float *probError = bbkeys::tables().probError;
    for (int64_t r = 0; r < n_reads; r++) {
        const bbidx_read in = reads_in[r];
        const int len = in.len > 0 ? in.len : 0;
        HostBytes B{bases + in.bases_off}, Q{quality ? quality + in.bases_off : bases}, Q2 = Q;
        int left = 0, right = 0;
        trim_read(*cfg, probError, B, Q, Q2, quality != nullptr, len, left, right);
        reads_out[r].bases_off = in.bases_off + left; reads_out[r].keys_off = 0; reads_out[r].len = in.len - left - right; reads_out[r].nkeys = 0;
        trims[r].left = left; trims[r].right = right;
    }
    return BBMAP_OK;
}

extern "C" int bbtrim_batch_device(const bbtrim_config *cfg, void *stream, int64_t n_reads, const bbidx_read *reads_in,
                                   const uint8_t *bases, const uint8_t *quality, bbidx_read *reads_out, bbtrim_rec *trims) {
    using namespace bbtrim;
    BBTRY(check_args("bbtrim_batch_device", cfg, n_reads, reads_in, bases, reads_out, trims));
    if (n_reads == 0) return BBMAP_OK;
    BBTRY(prepare_device());
    ProbTable table;
    const float *probError = bbkeys::tables().probError;
    for (int i = 0; i < 128; i++) table.v[i] = probError[i];
    return launch<256>(bbtrim_kernel, n_reads, (hipStream_t)stream, *cfg, table, (long long)n_reads, reads_in, bases, quality, reads_out, trims);
}
