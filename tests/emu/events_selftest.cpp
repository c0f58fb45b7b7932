// events_selftest.cpp -- csrc/events.h on the host: a stand-alone program (its own main, no HIP library) that defines the few HIP
// entry points the header calls on top of malloc / free, with a count of live events and streams, a switch that makes the k-th
// creation fail and one that makes the next record / elapsed / synchronise fail.  Built with -fsanitize=address,undefined by
// tests/test_events_cpu.py: a double destroy, a leak or a use after destroy in the types ends the run.  Prints "ok" and exits 0, or
// names the first miss and exits 1.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "events.h"

namespace {
std::set<void*> g_events, g_streams;      // live handles of either kind
int g_creates = 0, g_records = 0, g_fails = 0;
int g_fail_at = 0;                        // > 0: the g_fail_at-th creation (event or stream) from now fails (1 = the next one)
bool g_fail_use = false;                  // the next record / elapsed / synchronise fails
unsigned g_last_flags = 0;
hipStream_t g_last_stream = nullptr;
char g_err[256] = "";

template <class H>
hipError_t stub_create(std::set<void*>& live, H* h, unsigned flags) {
    if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;      // (*h is left as it was, as the runtime leaves it)
    ++g_creates;
    g_last_flags = flags;
    void* p = malloc(1);
    live.insert(p);
    *h = static_cast<H>(p);
    return hipSuccess;
}

hipError_t stub_destroy(std::set<void*>& live, void* p) {
    if (!live.erase(p)) {
        printf("destroy of %p, which is not a live handle of this kind\n", p);
        exit(1);
    }
    free(p);
    return hipSuccess;
}

hipError_t stub_use(hipEvent_t e) {
    if (!g_events.count(e)) {
        printf("use of %p, which is not a live event\n", (void*)e);
        exit(1);
    }
    if (!g_fail_use) return hipSuccess;
    g_fail_use = false;
    return hipErrorInvalidHandle;
}
}  // namespace

// (the signatures of <hip/hip_runtime_api.h>)
extern "C" {
hipError_t hipEventCreate(hipEvent_t* e) { return stub_create(g_events, e, hipEventDefault); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) { return stub_create(g_events, e, flags); }
hipError_t hipEventDestroy(hipEvent_t e) { return stub_destroy(g_events, e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { ++g_records; g_last_stream = s; return stub_use(e); }
hipError_t hipEventSynchronize(hipEvent_t e) { return stub_use(e); }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    const hipError_t e = stub_use(a);
    if (e != hipSuccess) return e;
    *ms = 1.5f;
    return stub_use(b);
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned flags) { return stub_create(g_streams, s, flags); }
hipError_t hipStreamDestroy(hipStream_t s) { return stub_destroy(g_streams, s); }
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "invalid handle"; }
}

namespace r3g {
int fail(int code, const char* fmt, ...) {      // (g_err stands in for r3g_last_error)
    ++g_fails;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
int hip_fail(hipError_t e, const char* what) { return fail(-3, "%s: %s", what, hipGetErrorString(e)); }
}  // namespace r3g

using r3g::Event;
using r3g::PassTimer;
using r3g::Stream;

#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                              \
        }                                                          \
    } while (0)

// the model's overlap resources and how dit_forward_grouped makes them: into locals, moved in when all three are there
struct Overlap { Stream aux; Event fork, join; };

static hipError_t overlap_make(Overlap& m) {
    Stream aux;
    Event fork, join;
    hipError_t e = aux.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = fork.create(hipEventDisableTiming);
    if (e == hipSuccess) e = join.create(hipEventDisableTiming);
    if (e != hipSuccess) return e;
    m.aux = std::move(aux), m.fork = std::move(fork), m.join = std::move(join);
    return hipSuccess;
}

template <int N>
static int timer_checks() {
    hipStream_t s = reinterpret_cast<hipStream_t>(0x40);
    for (int k = 0; k < N; ++k) {      // a make that fails at its k-th create leaves nothing behind, and the next one starts over
        PassTimer<N> t;
        const int creates = g_creates;
        g_fail_at = k + 1;
        g_err[0] = 0;
        CHECK(t.make("who") != 0 && g_events.empty() && g_creates == creates + k);
        for (int i = 0; i < N; ++i) CHECK(!t.ev[i]);
        CHECK(strcmp(g_err, "hipEventCreate(who): out of memory") == 0);
        CHECK(t.make("who") == 0 && (int)g_events.size() == N && g_creates == creates + k + N && g_last_flags == hipEventDefault);
        CHECK(t.make("who") == 0 && (int)g_events.size() == N && g_creates == creates + k + N);      // made: nothing is created
        for (int i = 0; i < N; ++i) CHECK(g_events.count(t.ev[i]) == 1);
    }
    CHECK(g_events.empty());           // destruction
    {   // recording, reading, waiting; a HIP error comes back as a non-zero rc with the call and the user in the text
        PassTimer<N> t;
        CHECK(t.make("plane") == 0);
        const int records = g_records, fails = g_fails;
        for (int i = 0; i < N; ++i) CHECK(t.mark(i, s) == 0);
        CHECK(g_records == records + N && g_last_stream == s && t.sync(N - 1) == 0);
        double ms = -1.0;
        for (int a = 0; a + 1 < N; ++a) CHECK(t.elapsed(a, &ms) == 0 && ms == 1.5);
        CHECK(g_fails == fails);
        g_fail_use = true;
        CHECK(t.mark(0, s) != 0 && strcmp(g_err, "hipEventRecord(plane): invalid handle") == 0);
        ms = -1.0;
        g_fail_use = true;
        CHECK(t.elapsed(0, &ms) != 0 && ms == -1.0 && strcmp(g_err, "hipEventElapsedTime(plane): invalid handle") == 0);
        g_fail_use = true;
        CHECK(t.sync(0) != 0 && strcmp(g_err, "hipEventSynchronize(plane): invalid handle") == 0);
        CHECK(g_fails == fails + 3 && t.mark(0, s) == 0 && (int)g_events.size() == N);
        // ownership: a moved-from timer is empty and destroys nothing
        PassTimer<N> u(std::move(t));
        for (int i = 0; i < N; ++i) CHECK(!t.ev[i] && g_events.count(u.ev[i]) == 1);
        CHECK((int)g_events.size() == N && u.mark(N - 1, s) == 0);
        { PassTimer<N> gone(std::move(t)); }
        CHECK((int)g_events.size() == N);
        CHECK(t.make("again") == 0 && (int)g_events.size() == 2 * N);      // and can be made again
    }
    CHECK(g_events.empty());
    return 0;
}

static int run() {
    if (timer_checks<2>() || timer_checks<5>() || timer_checks<6>()) return 1;
    {   // Event and Stream on their own
        Event e;
        CHECK(!e && g_events.empty());
        CHECK(e.create(hipEventDisableTiming) == hipSuccess && e && g_events.size() == 1 && g_last_flags == hipEventDisableTiming);
        CHECK(e.create(hipEventDefault) == hipSuccess && g_events.size() == 1 && g_events.count(e) == 1);      // in place of the first
        g_fail_at = 1;
        const int fails = g_fails;
        CHECK(e.create(hipEventDefault) == hipErrorOutOfMemory && !e && g_events.empty() && g_fails == fails);      // the error is the caller's
        CHECK(e.create(hipEventDefault) == hipSuccess);
        Event f(std::move(e));
        CHECK(!e && f && g_events.size() == 1);
        Event g;
        CHECK(g.create(hipEventDefault) == hipSuccess && g_events.size() == 2);
        hipEvent_t kept = f;
        g = std::move(f);      // g's own event goes with f, once
        f.release();
        CHECK(!f && g == kept && g_events.size() == 1);
        g = std::move(g);
        CHECK(g == kept && g_events.size() == 1);
        g.release();
        g.release();
        CHECK(!g && g_events.empty());
        Stream st;
        CHECK(st.create(hipStreamNonBlocking) == hipSuccess && st && g_streams.size() == 1 && g_last_flags == hipStreamNonBlocking);
    }
    CHECK(g_events.empty() && g_streams.empty());
    {   // the model's path: whichever of the three creations fails, nothing is live and nothing is held, so the next forward tries
        // again instead of recording on a null event; once made, they go with their owner
        Overlap m;
        for (int k = 1; k <= 3; ++k) {
            g_fail_at = k;
            CHECK(overlap_make(m) == hipErrorOutOfMemory && !m.aux && !m.fork && !m.join && g_events.empty() && g_streams.empty());
        }
        CHECK(overlap_make(m) == hipSuccess && m.aux && m.fork && m.join && g_events.size() == 2 && g_streams.size() == 1);
        CHECK(hipEventRecord(m.fork, m.aux) == hipSuccess && hipEventRecord(m.join, m.aux) == hipSuccess);
    }
    CHECK(g_events.empty() && g_streams.empty());
    return 0;
}

int main() {
    if (run()) return 1;
    printf("ok: %d creations, %d records\n", g_creates, g_records);
    return 0;
}
