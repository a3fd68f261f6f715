// Size, scan, emit: the middle step.  Only the files that call it include this (hipcub is heavy to compile).
#pragma once
#include <hipcub/hipcub.hpp>

#include "host_common.h"

// (a scan's accumulator type follows its INPUT type: int counts go in as long long so that offsets beyond 2^31 stay exact)
struct ToLL { __host__ __device__ long long operator()(int x) const { return (long long)x; } };

// The same scan over scratch the caller owns (the raw forms, which neither allocate nor wait): scan_scratch_bytes(n) bytes at tmp.
static hipError_t scan_scratch_bytes(long long n, size_t *need) {
    auto wide = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)nullptr, ToLL());
    *need = 0;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *need, wide, (long long *)nullptr, (int)(n + 1));
}
static hipError_t scan_offsets_scratch(int *counts, long long n, long long *offsets, void *tmp, size_t tmpBytes, hipStream_t stream) {
    auto wide = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)counts, ToLL());
    const hipError_t e = hipMemsetAsync(counts + n, 0, 4, stream);
    return e != hipSuccess ? e : hipcub::DeviceScan::ExclusiveSum(tmp, tmpBytes, wide, offsets, (int)(n + 1), stream);
}

// offsets[i] = counts[0] + ... + counts[i - 1] for i in [0, n], all on `stream`.  counts has n + 1 entries: entry n is zeroed
// here, so that offsets[n] is the total.  tmp is the scan's scratch, grown to what hipcub asks for (the stream is waited for when
// an older one has to go).  total: null, or where the total is brought back to; the stream has then been waited for.
static int scan_offsets(int *counts, long long n, long long *offsets, DevBuf &tmp, hipStream_t stream, long long *total) {
    size_t need = 0;
    auto wide = hipcub::TransformInputIterator<long long, ToLL, const int *>((const int *)counts, ToLL());
    BBHIP(hipcub::DeviceScan::ExclusiveSum(nullptr, need, wide, offsets, (int)(n + 1), stream));
    BBHIP(tmp.grow(need, 0, &stream));
    BBHIP(hipMemsetAsync(counts + n, 0, 4, stream));
    BBHIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, need, wide, offsets, (int)(n + 1), stream));
    if (!total) return BBMAP_OK;
    BBHIP(hipMemcpyAsync(total, offsets + n, 8, hipMemcpyDeviceToHost, stream));
    BBHIP(hipStreamSynchronize(stream));
    return BBMAP_OK;
}
