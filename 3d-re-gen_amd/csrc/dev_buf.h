// dev_buf.h -- DevBuf: the one owner of a device (or pinned host) allocation and its size.  Every buffer libr3g.so keeps
// between calls is a DevBuf member of the state that uses it, so it is released when that state goes; nothing is freed by hand.
// Needs only the HIP runtime API and fail / hip_fail (tests/emu/dev_buf_selftest.cpp compiles it against stubs of both).
#ifndef R3G_DEV_BUF_H
#define R3G_DEV_BUF_H
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <cstdio>

namespace r3g {

int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

// bytes of device memory held through DevBuf right now, process-wide (r3g_get_counter("device_bytes_live")); pinned buffers do not count
inline std::atomic<int64_t> g_device_bytes_live{0};

struct DevBuf {
    char* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;      // hipHostMalloc / hipHostFree instead of hipMalloc / hipFree

    DevBuf() = default;
    explicit DevBuf(bool pinned_) : pinned(pinned_) {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; pinned = o.pinned;
            o.p = nullptr; o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    explicit operator bool() const { return p != nullptr; }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }

    // Does not wait for anything: a caller whose kernels may still use the buffer synchronises first (grow does, on its stream).
    void release() {
        if (!p) return;
        if (pinned) {
            (void)hipHostFree(p);
        } else {
            (void)hipFree(p);
            g_device_bytes_live -= (int64_t)bytes;
        }
        p = nullptr;
        bytes = 0;
    }

    // Exactly `need` bytes in place of whatever was held; on failure the buffer is empty and the HIP error is the caller's to
    // judge (and to clear with hipGetLastError): for the one caller that can do without its buffer.
    hipError_t alloc(size_t need) {
        release();
        void* q = nullptr;
        const hipError_t e = pinned ? hipHostMalloc(&q, need, hipHostMallocDefault) : hipMalloc(&q, need);
        if (e != hipSuccess) return e;
        p = static_cast<char*>(q);
        bytes = need;
        if (!pinned) g_device_bytes_live += (int64_t)need;
        return hipSuccess;
    }

    // At least `need` bytes: nothing happens while they are there.  Otherwise the stream is synchronised before a live buffer is
    // freed (its kernels may still run) and exactly `need` bytes are allocated: no geometric growth, contents are not kept.  On
    // failure the buffer is empty and the error text names it.
    int grow(size_t need, hipStream_t s, const char* what) {
        if (need <= bytes) return 0;
        char text[96];
        if (p) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                snprintf(text, sizeof text, "hipStreamSynchronize(%s)", what);
                return hip_fail(e, text);
            }
        }
        const hipError_t e = alloc(need);
        if (e == hipSuccess) return 0;
        (void)hipGetLastError();      // an allocation failure is not sticky: the next launch's check must not see it
        snprintf(text, sizeof text, "%s(%s, %zu bytes)", pinned ? "hipHostMalloc" : "hipMalloc", what, need);
        return hip_fail(e, text);
    }
};

}  // namespace r3g
#endif
