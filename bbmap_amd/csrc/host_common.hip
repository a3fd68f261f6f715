// The per-thread error store of the C ABI (include/bbmap_amd.h) and the few helpers every host file shares (host_common.h).
#include "host_common.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local char g_err[512] = "";

extern "C" const char *bbmap_last_error(void) { return g_err; }
extern "C" int bbmap_abi_version(void) { return BBMAP_AMD_ABI_VERSION; }
void bbmap_set_error(const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); }

int bbfail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

int bb_use_gfx950(const char *who, int device, hipDeviceProp_t *prop) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bbfail(BBMAP_E_NODEVICE, "%s: no HIP device (this library has no CPU path)", who);
    if (device < 0 || device >= ndev) return bbfail(BBMAP_E_ARG, "%s: bad device ordinal", who);
    BBHIP(hipSetDevice(device));
    hipDeviceProp_t mine;
    if (!prop) prop = &mine;
    BBHIP(hipGetDeviceProperties(prop, device));
    if (strncmp(prop->gcnArchName, "gfx950", 6) != 0) return bbfail(BBMAP_E_NODEVICE, "%s: device is %s, this build targets gfx950 only", who, prop->gcnArchName);
    return BBMAP_OK;
}
