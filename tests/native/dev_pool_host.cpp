// dev_pool_host.cpp -- csrc/dev_pool.h on the CPU: a stand-alone program (tests/test_dev_pool_cpu.py)
// that defines the HIP allocation calls itself, malloc-backed, so it links without the HIP runtime
// and a sanitizer build sees every buffer the pool forgets to free or frees twice.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "../../alphazero-multi-game_amd/csrc/dev_pool.h"

static std::set<void*> g_live;      // what the fake device holds
static int g_mallocs = 0, g_bad_free = 0;
static char g_msg[256];

hipError_t hipMalloc(void** p, size_t bytes) {
    ++g_mallocs;
    *p = malloc(bytes);
    g_live.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!g_live.erase(p)) { ++g_bad_free; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
int az_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static int64_t bytes() { return DevPool::live_bytes.load(); }
static int64_t bufs() { return DevPool::live_bufs.load(); }

int main() {
    {   // allocation order, recorded bytes (n == 0 -> 1 element; the tail is allocated, not recorded)
        DevPool p;
        float* a = nullptr; uint16_t* h = nullptr; double* z = nullptr; int* i = nullptr;
        CHECK(p.alloc(&a, 10) == 0 && p.alloc(&h, 7, 64) == 0 && p.alloc(&z, 0) == 0 && p.alloc(&i, 3) == 0);
        CHECK(p.bufs.size() == 4 && g_live.size() == 4);
        CHECK(p.bufs[0].p == a && p.bufs[0].bytes == 40);
        CHECK(p.bufs[1].p == h && p.bufs[1].bytes == 14);
        CHECK(p.bufs[2].p == z && p.bufs[2].bytes == 8);
        CHECK(p.bufs[3].p == i && p.bufs[3].bytes == 12);
        CHECK(bytes() == 74 && bufs() == 4);
        h[7 + 63] = 1;                       // the tail is there (a sanitizer build checks the bound)
        // release: a middle buffer, null, an unknown pointer
        p.release(h);
        CHECK(p.bufs.size() == 3 && p.bufs[0].p == a && p.bufs[1].p == z && p.bufs[2].p == i);
        CHECK(bytes() == 60 && bufs() == 3 && g_live.size() == 3);
        int unknown = 0;
        p.release(nullptr);
        p.release(&unknown);
        p.release(h);                        // already forgotten
        CHECK(p.bufs.size() == 3 && bytes() == 60 && bufs() == 3 && g_bad_free == 0);
        // clear, then reuse
        p.clear();
        CHECK(p.bufs.empty() && bytes() == 0 && bufs() == 0 && g_live.empty());
        CHECK(p.alloc(&a, 5) == 0 && p.bufs.size() == 1 && p.bufs[0].bytes == 20 && bytes() == 20);
    }
    CHECK(bytes() == 0 && bufs() == 0 && g_live.empty());   // the destructor clears
    {   // move construction and assignment; adopt
        DevPool p;
        int *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(p.alloc(&a, 1) == 0 && p.alloc(&b, 2) == 0);
        DevPool q(std::move(p));
        CHECK(p.bufs.empty() && q.bufs.size() == 2 && q.bufs[0].p == a && q.bufs[1].p == b && bufs() == 2);
        DevPool r;
        CHECK(r.alloc(&c, 3) == 0 && bufs() == 3);
        r = std::move(q);                    // frees c, takes a and b
        CHECK(q.bufs.empty() && r.bufs.size() == 2 && r.bufs[0].p == a && bufs() == 2 && g_live.size() == 2);
        CHECK(g_live.count(c) == 0);
        DevPool s;
        CHECK(s.alloc(&c, 4) == 0);
        r.adopt(s);
        CHECK(s.bufs.empty() && r.bufs.size() == 3 && r.bufs[2].p == c && r.bufs[2].bytes == 16 && bufs() == 3);
    }
    CHECK(bytes() == 0 && bufs() == 0 && g_live.empty());
    // failure injection at every position of a 5-allocation sequence
    for (int k = 0; k < 5; ++k) {
        DevPool p;
        float* q[5] = {};
        DevPool::fail_in.store(k);
        const int m0 = g_mallocs;
        int rc = 0, done = 0;
        for (; done < 5 && !rc; ++done) rc = p.alloc(&q[done], 4 + done);
        CHECK(rc == AZ_ERR_OOM && done == k + 1);
        CHECK(g_mallocs - m0 == k);                          // the failing call never reaches hipMalloc
        CHECK(q[k] == nullptr);
        CHECK((int)p.bufs.size() == k && bufs() == k);       // exactly the earlier buffers
        for (int j = 0; j < k; ++j) CHECK(p.bufs[j].p == q[j] && p.bufs[j].bytes == (size_t)(4 + j) * 4);
        CHECK(DevPool::fail_in.load() == -1);                // disarmed
        CHECK(std::string(g_msg).find("hipMalloc(") == 0);
        CHECK(p.alloc(&q[k], 4 + k) == 0 && (int)p.bufs.size() == k + 1);   // and the next one succeeds
    }
    CHECK(bytes() == 0 && bufs() == 0 && g_live.empty() && g_bad_free == 0);
    {   // disarming: the countdown it replaces is visible, no allocation fails afterwards
        DevPool p;
        int* a = nullptr;
        DevPool::fail_in.store(3);
        CHECK(p.alloc(&a, 1) == 0 && DevPool::fail_in.load() == 2);
        CHECK(DevPool::fail_in.exchange(-1) == 2);
        for (int j = 0; j < 4; ++j) CHECK(p.alloc(&a, 1) == 0);
    }
    CHECK(bytes() == 0 && bufs() == 0 && g_live.empty() && g_bad_free == 0);
    printf(g_fail ? "dev_pool: %d FAILED\n" : "dev_pool ok\n", g_fail);
    return g_fail ? 1 : 0;
}
