// engine_internal.h -- pieces of the host runtime shared by the C-ABI translation units
// (engine.hip, net_host.hip, search_host.hip, selfplay.hip, dataset.hip, dist.hip): the engine
// handle, the thread-local error report, the allocation / HIP-status helpers, the sampled
// profiling clock and the step trace.  Not part of the public boundary (include/az_engine.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/az_engine.h"
#include "dev_pool.h"

struct az_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop{};
    std::mutex mu;
};

#define HIPCHK(x)                                                                            \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) return az_fail(AZ_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Net internals for the multi-GPU collectives (dist.hip, az_net_broadcast_weights):
// the device buffers of the net's loaded weights (every packed piece set), allocating them with a
// load of zero weights if the net was never loaded; the canonical blob on the host.
struct az_net;
int net_weight_buffers(az_net* n, std::vector<DevPool::Buf>& out);
const std::vector<float>& net_host_blob(az_net* n);
size_t net_param_count(az_net* n);
az_engine* net_engine(az_net* n);
std::mutex& net_mutex(az_net* n);
// after a broadcast filled the device buffers: the host copy of the canonical blob, loaded = true
void net_adopt_blob(az_net* n, const float* blob);

// Sampled kernel timing (az_net_profile / az_search_profile, bench.py's roofline and tree-kernel
// times): a one-wave kernel on the engine stream writes the 100 MHz device clock (s_memrealtime)
// into the next slot of a device buffer; a timed interval is the difference of two stamps around
// the kernels it brackets (same-stream order: each stamp runs after the previous kernel completes).
// HIP events, used before round 4, never completed under rocprofv3 --pmc counter collection once a
// selfplay step had recorded them (profiles/r03e_pmc_hang_probe.txt); stamps are ordinary dispatches.
__global__ void k_clock_stamp(unsigned long long* out);   // engine.hip
struct ProfClock {
    static constexpr size_t CAP = 1 << 16;      // stamps per profiling session (bench: a few thousand)
    unsigned long long* d = nullptr;
    size_t used = 0;
    bool room(size_t k) const { return d && used + k <= CAP; }
    void stamp(hipStream_t st) { hipLaunchKernelGGL(k_clock_stamp, dim3(1), dim3(64), 0, st, d + used); ++used; }
    // the stamps [0, used) on the host, in milliseconds (10 ns ticks)
    std::vector<double> read_ms() const {
        std::vector<unsigned long long> h(used);
        if (used && hipMemcpy(h.data(), d, used * 8, hipMemcpyDeviceToHost) != hipSuccess) h.assign(used, 0);
        std::vector<double> out(used);
        for (size_t i = 0; i < used; ++i) out[i] = (double)h[i] * 1e-5;
        return out;
    }
    // profiling switched on: the stamp buffer, once, from the owning handle's pool
    int enable(DevPool& pool) {
        if (!d && pool.alloc(&d, CAP)) return az_fail(AZ_ERR_OOM, "profile clock buffer");
        return 0;
    }
};

// Profiling stamps (ProfClock) are recorded on one simulation step / forward in AZ_PROF_EVERY
// (default 16): every marker on the queue leaves a gap of a few us (round 2 measured ~6 us per HIP
// event), which at C2 (a ~140 us simulation step) would otherwise inflate the timed loop.  Reads
// scale the sampled times to all steps.
inline int prof_every() {
    static const int p = getenv("AZ_PROF_EVERY") ? std::max(1, atoi(getenv("AZ_PROF_EVERY"))) : 16;
    return p;
}

// A page-locked host buffer: per-move copies to / from it run at DMA speed (a pageable host side
// goes through the runtime's staging buffer).  get(k) grows it to k elements (null on failure).
template <class T>
struct Pinned {
    T* p = nullptr;
    size_t n = 0;
    T* get(size_t k) {
        if (k > n) {
            if (p) (void)hipHostFree(p);
            p = nullptr; n = 0;
            if (hipHostMalloc((void**)&p, k * sizeof(T), hipHostMallocDefault) != hipSuccess) p = nullptr;
            else n = k;
        }
        return p;
    }
    T* data() { return p; }
    ~Pinned() { if (p) (void)hipHostFree(p); }
};

// diagnostic phase trace of az_selfplay_step on stderr (az_diag_set_step_trace; tools/pmc_progress.py):
// names the host call a step is blocked in when a profiler stalls it
extern int g_step_trace;   // engine.hip
// each line carries the host's wall clock (ms, steady_clock) so the phases of a move can be timed
#define STEP_TRACE(...)                                                                               \
    do {                                                                                              \
        if (g_step_trace) {                                                                           \
            fprintf(stderr, "[step %.3f] ", std::chrono::duration<double, std::milli>(                \
                                                std::chrono::steady_clock::now().time_since_epoch()).count()); \
            fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fflush(stderr);                        \
        }                                                                                             \
    } while (0)
