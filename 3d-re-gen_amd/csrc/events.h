// events.h -- Event, Stream and PassTimer: the one owner of a HIP event (or stream).  Every event libr3g.so keeps between calls is a
// member of the state that uses it, so it is destroyed when that state goes; nothing is destroyed by hand (prof.cpp's ring is the one
// exception: process-wide, made lazily, never destroyed).  Needs only the HIP runtime API and fail / hip_fail
// (tests/emu/events_selftest.cpp compiles it against stubs of both).
#ifndef R3G_EVENTS_H
#define R3G_EVENTS_H
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <utility>

namespace r3g {

int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

// A handle made by Create(&h, flags) and destroyed by Destroy(h): move-only (so not copyable), empty until create() succeeds
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;

    Owned() = default;
    Owned(Owned&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }      // (what was held goes with o)
    ~Owned() { release(); }
    operator H() const { return h; }

    void release() {      // does not wait for anything, like DevBuf::release
        if (h) (void)Destroy(std::exchange(h, nullptr));
    }
    // In place of whatever was held; on failure the owner is empty and the HIP error is the caller's to judge
    hipError_t create(unsigned flags) {
        release();
        const hipError_t e = Create(&h, flags);
        if (e != hipSuccess) h = nullptr;
        return e;
    }
};
using Event = Owned<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;      // flags: hipEventDefault (timing), hipEventDisableTiming
using Stream = Owned<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// N timing events around the passes of one call, all of them there or none.  Whether they bracket a complete run is the user's to
// keep (a *_timed flag beside the timer), not the timer's.  Every member returns an rc, with the user's name in the error text.
template <int N>
struct PassTimer {
    Event ev[N];
    const char* who = "";      // from make()

    // Nothing happens while the events are there.  A failing create destroys what this call made: the next call starts over.
    int make(const char* who_) {
        who = who_;
        if (ev[N - 1]) return 0;
        for (int i = 0; i < N; ++i) {
            const hipError_t e = ev[i].create(hipEventDefault);
            if (e == hipSuccess) continue;
            while (i-- > 0) ev[i].release();
            return rc(e, "hipEventCreate");
        }
        return 0;
    }
    int mark(int i, hipStream_t s) const { return rc(hipEventRecord(ev[i], s), "hipEventRecord"); }
    int sync(int i) const { return rc(hipEventSynchronize(ev[i]), "hipEventSynchronize"); }
    // the milliseconds between events a and a + 1 (*ms is left alone on failure)
    int elapsed(int a, double* ms) const {
        float t = 0.0f;
        const hipError_t e = hipEventElapsedTime(&t, ev[a], ev[a + 1]);
        if (e == hipSuccess) *ms = (double)t;
        return rc(e, "hipEventElapsedTime");
    }

    int rc(hipError_t e, const char* call) const {
        if (e == hipSuccess) return 0;
        char text[96];
        snprintf(text, sizeof text, "%s(%s)", call, who);
        return hip_fail(e, text);
    }
};

}  // namespace r3g
#endif
