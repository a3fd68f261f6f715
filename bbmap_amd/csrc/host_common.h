// What every host file of the library needs: the per-thread error store behind bbmap_last_error, one way to fail, one macro
// around a HIP call, the device check of the creators, and the two kinds of device buffer (kept and grown by a context; held for
// the length of one call).  Everything with inline members is hidden: none of it is a symbol of the library.
#pragma once
#include <hip/hip_runtime.h>

#include "bbmap_amd.h"

#define BB_HIDDEN __attribute__((visibility("hidden")))

// the message bbmap_last_error() returns on this thread
void bbmap_set_error(const char *msg);
// formats the message and returns `code`: `return bbfail(BBMAP_E_ARG, "f: bad argument");`
BB_HIDDEN int bbfail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// a HIP call: on failure "<expr> failed: <hipGetErrorString>" and BBMAP_E_HIP
#define BBHIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return bbfail(BBMAP_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)
// a call of the library's own: its code (and message) are handed on
#define BBTRY(expr) do { const int rc_ = (expr); if (rc_ != BBMAP_OK) return rc_; } while (0)

BB_HIDDEN int env_int(const char *name, int dflt);

// Makes `device` the current one and checks that it is a gfx950: BBMAP_E_NODEVICE without any HIP device or on another
// architecture, BBMAP_E_ARG for an ordinal the machine does not have.  `who` opens the message; `prop` may be null.
BB_HIDDEN int bb_use_gfx950(const char *who, int device, hipDeviceProp_t *prop = nullptr);

// kernel<<<ceil(threads / TB), TB, 0, stream>>>(args...)
template <unsigned TB, class K, class... A> static int launch(K kernel, long long threads, hipStream_t stream, const A &...args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + TB - 1) / TB)), dim3(TB), 0, stream, args...);
    BBHIP(hipGetLastError());
    return BBMAP_OK;
}

// A device buffer that is allocated on first use and replaced by a larger one when a call needs more (contents are not kept).
struct BB_HIDDEN DevBuf {
    void *p = nullptr; size_t cap = 0;
    // Room for `need` bytes.  slack: added when the buffer has to grow, so that sizes creeping up do not reallocate every batch.
    // busy: a stream whose queued work may still use the old buffer; it is waited for before the buffer is freed.
    hipError_t grow(size_t need, size_t slack = 0, const hipStream_t *busy = nullptr) {
        if (need <= cap) return hipSuccess;
        if (p) {
            if (busy) { const hipError_t e = hipStreamSynchronize(*busy); if (e != hipSuccess) return e; }
            release();
        }
        const hipError_t e = hipMalloc(&p, need + slack);
        if (e == hipSuccess) cap = need + slack;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

// A device array that lives as long as its scope: the copies a host-convenience entry point makes of its caller's buffers.
template <class T> struct BB_HIDDEN DevTmp {
    T *p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp &) = delete;
    DevTmp &operator=(const DevTmp &) = delete;
    ~DevTmp() { if (p) (void)hipFree(p); }
    operator T *() const { return p; }
    // room for `count` elements (one when count is 0: a null device pointer would read as "no buffer")
    int alloc(size_t count) {
        BBHIP(hipMalloc(&p, (count ? count : 1) * sizeof(T)));
        return BBMAP_OK;
    }
    int upload(const T *host, size_t count) {
        BBTRY(alloc(count));
        BBHIP(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
        return BBMAP_OK;
    }
};
