// engine.hip -- the engine handle and the error report of the host runtime behind
// include/az_engine.h (libaz_hip.so).  The network is net_host.hip / net_load.hip, the search
// search_host.hip, the self-play driver selfplay.hip.
//
// The runtime owns device memory, streams and launches; no exceptions cross the C-ABI.
// The product path never falls back to the CPU: without a HIP device every entry
// point fails with AZ_ERR_HIP.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/az_engine.h"
#include "engine_internal.h"

namespace {
thread_local std::string g_err;
}  // namespace

int az_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// The profiling clock stamp of ProfClock (engine_internal.h).
__global__ void k_clock_stamp(unsigned long long* out) {
    if (threadIdx.x == 0) out[threadIdx.x] = __builtin_amdgcn_s_memrealtime();   // vector store (lane-indexed)
}

int g_step_trace = 0;   // STEP_TRACE (engine_internal.h)

extern "C" {

const char* az_last_error(void) { return g_err.c_str(); }

int az_engine_create(int device, az_engine** out) {
    if (!out) return az_fail(AZ_ERR_ARG, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return az_fail(AZ_ERR_HIP, "no HIP device available (hipGetDeviceCount: %s)", hipGetErrorString(e));
    if (device < 0 || device >= n) return az_fail(AZ_ERR_ARG, "device %d out of range (%d devices)", device, n);
    auto* en = new az_engine();
    en->device = device;
    hipError_t r = hipSetDevice(device);
    if (r == hipSuccess) r = hipGetDeviceProperties(&en->prop, device);
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&en->stream, hipStreamNonBlocking);
    if (r != hipSuccess) { delete en; return az_fail(AZ_ERR_HIP, "device init: %s", hipGetErrorString(r)); }
    *out = en;
    return 0;
}

void az_engine_destroy(az_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int az_engine_device_name(az_engine* e, char* buf, int len) {
    if (!e || !buf || len <= 0) return az_fail(AZ_ERR_ARG, "bad args");
    snprintf(buf, len, "%s (%s)", e->prop.name, e->prop.gcnArchName);
    return 0;
}

int az_diag_set_step_trace(int on) { g_step_trace = on; return 0; }

int az_diag_device_mem(int64_t* bytes, int64_t* buffers) {
    if (bytes) *bytes = DevPool::live_bytes.load();
    if (buffers) *buffers = DevPool::live_bufs.load();
    return 0;
}

int az_diag_fail_alloc(int nth) { return DevPool::fail_in.exchange(nth < 0 ? -1 : nth); }

}  // extern "C"
