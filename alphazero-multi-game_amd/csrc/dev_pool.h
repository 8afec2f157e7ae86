// dev_pool.h -- device memory ownership of the host runtime: the only place that calls hipMalloc /
// hipFree.  Every handle (az_net, az_search, az_dataset, az_dist) allocates from DevPools it holds
// by value, so destroying the handle -- or leaving a function that built a local pool -- frees
// every buffer, on success and on every error path alike.  Host-only (no __global__ code).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/az_engine.h"

// Sets the az_last_error() message; returns code.
int az_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

struct DevPool {
    struct Buf { void* p; size_t bytes; };   // bytes: the payload asked for (before any tail)
    std::vector<Buf> bufs;                   // allocation order

    // Process-wide totals over every pool (az_diag_device_mem): payload bytes and buffers alive.
    static inline std::atomic<int64_t> live_bytes{0}, live_bufs{0};
    // Failure injection (az_diag_fail_alloc): allocations left before one fails; -1 = disarmed.
    static inline std::atomic<int> fail_in{-1};

    DevPool() = default;
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    DevPool(DevPool&& o) noexcept : bufs(std::move(o.bufs)) { o.bufs.clear(); }
    DevPool& operator=(DevPool&& o) noexcept {
        if (this != &o) { clear(); bufs = std::move(o.bufs); o.bufs.clear(); }
        return *this;
    }
    ~DevPool() { clear(); }

    // n elements of T plus `tail` more that the recorded size leaves out (n == 0 -> 1).
    // On failure *p is null and the pool is as it was.
    template <class T>
    int alloc(T** p, size_t n, size_t tail = 0) {
        if (n == 0) n = 1;
        const size_t bytes = (n + tail) * sizeof(T);
        *p = nullptr;
        const int c = fail_in.load();
        if (c >= 0) fail_in.store(c - 1);   // reaching zero fails this call and disarms
        hipError_t e = c == 0 ? hipErrorOutOfMemory : hipMalloc((void**)p, bytes);
        if (e != hipSuccess) {
            *p = nullptr;
            return az_fail(AZ_ERR_OOM, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
        }
        bufs.push_back({(void*)*p, n * sizeof(T)});
        live_bytes += (int64_t)(n * sizeof(T));
        ++live_bufs;
        return 0;
    }

    // Free one buffer and forget it; null or a pointer the pool does not hold is a no-op.
    void release(const void* p) {
        if (!p) return;
        for (size_t i = 0; i < bufs.size(); ++i)
            if (bufs[i].p == p) { drop(bufs[i]); bufs.erase(bufs.begin() + i); return; }
    }
    // Take over every buffer of `o`, after this pool's own.
    void adopt(DevPool& o) {
        bufs.insert(bufs.end(), o.bufs.begin(), o.bufs.end());
        o.bufs.clear();
    }
    void clear() {
        for (size_t i = bufs.size(); i-- > 0;) drop(bufs[i]);   // newest first
        bufs.clear();
    }

private:
    static void drop(const Buf& b) {
        (void)hipFree(b.p);
        live_bytes -= (int64_t)b.bytes;
        --live_bufs;
    }
};
