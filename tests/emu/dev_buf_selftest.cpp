// dev_buf_selftest.cpp -- csrc/dev_buf.h on the host: a stand-alone program (its own main, no HIP library) that defines the few HIP
// entry points the header calls on top of malloc / free, with a count of live allocations, a count of stream syncs and a switch
// that makes the n-th allocation fail.  Built with -fsanitize=address,undefined by tests/test_dev_buf_cpu.py: a double free, a
// leak or a use after free in the type ends the run.  Prints "ok" and exits 0, or names the first miss and exits 1.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <unordered_map>
#include <utility>

#include "dev_buf.h"

namespace {
std::set<void*> g_dev, g_host;      // live allocations of either kind
int g_syncs = 0, g_allocs = 0, g_last_error_reads = 0, g_fails = 0;
int g_fail_at = 0;                  // > 0: the g_fail_at-th allocation from now fails (1 = the next one)
hipStream_t g_last_stream = nullptr;
char g_err[256] = "";

hipError_t stub_alloc(std::set<void*>& live, void** p, size_t n) {
    if (g_fail_at > 0 && --g_fail_at == 0) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    ++g_allocs;
    *p = malloc(n ? n : 1);
    live.insert(*p);
    return hipSuccess;
}

hipError_t stub_free(std::set<void*>& live, void* p) {
    if (!live.erase(p)) {
        printf("free of %p, which is not a live allocation of this kind\n", p);
        exit(1);
    }
    free(p);
    return hipSuccess;
}
}  // namespace

// (the signatures of <hip/hip_runtime_api.h>; hipMalloc / hipHostMalloc also have template overloads there, which forward to these)
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return stub_alloc(g_dev, p, n); }
hipError_t hipFree(void* p) { return stub_free(g_dev, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return stub_alloc(g_host, p, n); }
hipError_t hipHostFree(void* p) { return stub_free(g_host, p); }
hipError_t hipStreamSynchronize(hipStream_t s) { ++g_syncs; g_last_stream = s; return hipSuccess; }
hipError_t hipGetLastError(void) { ++g_last_error_reads; return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some error"; }
}

namespace r3g {
int fail(int code, const char* fmt, ...) {
    ++g_fails;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
int hip_fail(hipError_t e, const char* what) { return fail(-3, "%s: %s", what, hipGetErrorString(e)); }
}  // namespace r3g

using r3g::DevBuf;

#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                              \
        }                                                          \
    } while (0)

static int64_t live_bytes() { return r3g::g_device_bytes_live.load(); }

struct Pair { DevBuf a, b; };      // like Model::W8: two buffers as the value of a map

static int run() {
    hipStream_t s = reinterpret_cast<hipStream_t>(0x40);
    {   // growth
        DevBuf b;
        CHECK(!b && b.p == nullptr && b.bytes == 0 && live_bytes() == 0);
        CHECK(b.grow(0, s, "nothing") == 0 && !b && g_allocs == 0);
        CHECK(b.grow(100, s, "first") == 0 && b && b.bytes == 100 && g_dev.size() == 1 && g_syncs == 0 && live_bytes() == 100);
        memset(b.p, 0x5a, 100);
        CHECK(b.as<float>() == reinterpret_cast<float*>(b.p));
        char* p = b.p;
        const int allocs = g_allocs;
        CHECK(b.grow(100, s, "equal") == 0 && b.grow(7, s, "smaller") == 0 && b.p == p && b.bytes == 100);
        CHECK(g_syncs == 0 && g_allocs == allocs && live_bytes() == 100);
        CHECK(b.grow(101, s, "larger") == 0 && b.bytes == 101 && g_dev.size() == 1 && g_dev.count(b.p) == 1);
        CHECK(g_syncs == 1 && g_last_stream == s && g_allocs == allocs + 1 && live_bytes() == 101);
        memset(b.p, 0x5a, 101);
    }
    CHECK(g_dev.empty() && live_bytes() == 0);
    {   // failure handling
        DevBuf b;
        CHECK(b.grow(64, s, "before") == 0);
        g_fail_at = 1;
        g_err[0] = 0;
        const int syncs = g_syncs, reads = g_last_error_reads;
        CHECK(b.grow(128, s, "the named buffer") != 0);
        CHECK(!b && b.bytes == 0 && g_dev.empty() && live_bytes() == 0 && g_syncs == syncs + 1);
        CHECK(strstr(g_err, "the named buffer") && strstr(g_err, "128") && strstr(g_err, "out of memory"));
        CHECK(g_last_error_reads == reads + 1);      // the failed allocation's error does not stay behind
        CHECK(b.grow(128, s, "again") == 0 && b.bytes == 128 && g_syncs == syncs + 1 && live_bytes() == 128);
        // alloc: the error comes back as it is, fail / hip_fail are not called and nothing is cleared
        const int fails = g_fails, reads2 = g_last_error_reads;
        g_fail_at = 1;
        CHECK(b.alloc(256) == hipErrorOutOfMemory && !b && b.bytes == 0 && g_fails == fails && g_last_error_reads == reads2);
        CHECK(g_dev.empty() && live_bytes() == 0);
        CHECK(b.alloc(256) == hipSuccess && b.bytes == 256 && live_bytes() == 256);
        CHECK(b.alloc(16) == hipSuccess && b.bytes == 16 && g_dev.size() == 1 && live_bytes() == 16);      // exactly `need`, also downwards
    }
    CHECK(g_dev.empty() && live_bytes() == 0);
    {   // three buffers grown one by one behind no common test (the ln_3 fold's): the second allocation fails, the next round
        // allocates exactly the missing two
        DevBuf w, c, st;
        auto round = [&]() { int rc = w.grow(1000, s, "w"); if (!rc) rc = c.grow(200, s, "c"); if (!rc) rc = st.grow(30, s, "st"); return rc; };
        g_fail_at = 2;
        CHECK(round() != 0 && w && !c && !st && strstr(g_err, "(c,") && live_bytes() == 1000);
        char* wp = w.p;
        const int allocs = g_allocs;
        CHECK(round() == 0 && w.p == wp && c && st && g_allocs == allocs + 2 && g_dev.size() == 3 && live_bytes() == 1230);
        CHECK(round() == 0 && g_allocs == allocs + 2);
    }
    CHECK(g_dev.empty() && live_bytes() == 0);
    {   // ownership
        DevBuf a;
        CHECK(a.grow(10, s, "a") == 0);
        char* ap = a.p;
        DevBuf b(std::move(a));
        CHECK(!a && a.bytes == 0 && b.p == ap && b.bytes == 10 && g_dev.size() == 1 && live_bytes() == 10);
        DevBuf c;
        CHECK(c.grow(20, s, "c") == 0 && live_bytes() == 30);
        c = std::move(b);      // frees c's 20 bytes, once
        CHECK(!b && b.bytes == 0 && c.p == ap && c.bytes == 10 && g_dev.size() == 1 && live_bytes() == 10);
        c = std::move(c);
        CHECK(c.p == ap && c.bytes == 10);
        const int syncs = g_syncs;
        c.release();
        c.release();
        CHECK(!c && c.bytes == 0 && g_dev.empty() && live_bytes() == 0 && g_syncs == syncs);      // release does not synchronise
        a.release();      // a moved-from buffer
        std::unordered_map<std::string, Pair> map;
        for (const char* k : {"x", "y", "z"}) {
            Pair q;
            CHECK(q.a.grow(8, s, "a") == 0 && q.b.grow(4, s, "b") == 0);
            map.emplace(k, std::move(q));
        }
        CHECK(g_dev.size() == 6 && live_bytes() == 36);
        map.erase("y");
        CHECK(g_dev.size() == 4 && live_bytes() == 24);
        map.clear();
        CHECK(g_dev.empty() && live_bytes() == 0);
    }
    {   // the pinned flavour: through hipHostMalloc / hipHostFree, not counted
        DevBuf h(true);
        CHECK(h.grow(64, s, "pinned") == 0 && h.pinned && g_host.size() == 1 && g_dev.empty() && live_bytes() == 0);
        CHECK(h.grow(64, s, "pinned") == 0 && g_host.size() == 1);
        DevBuf k(std::move(h));
        CHECK(k.pinned && !h && g_host.size() == 1);
        g_fail_at = 1;
        CHECK(k.grow(65, s, "pinned again") != 0 && !k && g_host.empty() && strstr(g_err, "hipHostMalloc(pinned again"));
        CHECK(k.grow(65, s, "pinned again") == 0 && g_host.size() == 1 && live_bytes() == 0);
    }
    CHECK(g_dev.empty() && g_host.empty() && live_bytes() == 0);
    return 0;
}

int main() {
    if (run()) return 1;
    printf("ok: %d allocations, %d stream syncs\n", g_allocs, g_syncs);
    return 0;
}
