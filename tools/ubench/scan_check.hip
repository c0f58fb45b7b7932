// scan_check.hip -- csrc/scan_device.h against a host loop modulo 2^32: the device-wide exclusive scan out of place and in
// place, with and without the total, at the thread, tile and sums-loop boundaries and past 10240 tiles, and on arrays that are
// not 16-byte aligned; the popcount Load on 64-bit words; block_exclusive_scan<NW> in one block.  Prints the number of
// mismatching values.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scan_check scan_check.hip && ./scan_check
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../3d-re-gen_amd/csrc/scan_device.h"

using namespace r3g;

#define CHECK(x)                                                                              \
    do {                                                                                      \
        const hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                               \
            printf("scan: %s at line %d: %s\n", #x, __LINE__, hipGetErrorString(e_));         \
            exit(2);                                                                          \
        }                                                                                     \
    } while (0)

struct PopcLoad {
    const unsigned long long* words;
    __device__ unsigned operator()(int64_t i) const { return (unsigned)__popcll(words[i]); }
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void block_scan_kernel(unsigned* out, unsigned* total) {
    __shared__ unsigned lds[NW];
    unsigned t;
    out[threadIdx.x] = block_exclusive_scan<NW>(threadIdx.x % 5, lds, &t);
    if (threadIdx.x == NW * 64 - 1) *total = t;
}

static const int64_t kMaxN = 20971521;       // one past 256 * 40 tiles of 2048
static unsigned *d_in, *d_out, *d_sums, *d_total;
static unsigned long long* d_words;
static std::vector<unsigned> h_in, h_ref, h_out;
static long g_bad = 0, g_checked = 0;

// h_ref = exclusive prefix of h_in[0, n); returns the total
static unsigned host_scan(int64_t n) {
    unsigned run = 0;
    for (int64_t i = 0; i < n; ++i) {
        h_ref[i] = run;
        run += h_in[i];
    }
    return run;
}

static void compare(const unsigned* d_res, int64_t n, bool with_total, unsigned total) {
    CHECK(hipMemcpy(h_out.data(), d_res, 4 * (size_t)n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) g_bad += h_out[i] != h_ref[i];
    g_checked += n;
    if (with_total) {
        unsigned t;
        CHECK(hipMemcpy(&t, d_total, 4, hipMemcpyDeviceToHost));
        g_bad += t != total;
        ++g_checked;
    }
}

// h_in[0, n) is set: out of place and in place, the total asked for and not; the arrays begin `off` words into their buffers
static void check_u32(int64_t n, int off = 0) {
    const unsigned total = host_scan(n);
    unsigned *d_in = ::d_in + off, *d_out = ::d_out + off;
    for (int with_total = 0; with_total < 2; ++with_total) {
        CHECK(hipMemcpy(d_in, h_in.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
        CHECK(hipMemset(d_total, 0xA5, 4));
        CHECK(exclusive_scan(ScanLoadU32{d_in}, n, d_out, d_sums, with_total ? d_total : nullptr, 0));
        compare(d_out, n, with_total, total);
        CHECK(exclusive_scan(ScanLoadU32{d_in}, n, d_in, d_sums, with_total ? d_total : nullptr, 0));
        compare(d_in, n, with_total, total);
    }
}

static void check_popc(int64_t n) {
    std::vector<unsigned long long> w((size_t)n);
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (int64_t i = 0; i < n; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        w[i] = i % 11 == 0 ? ~0ull : (i % 5 == 0 ? 0ull : x);
        h_in[i] = (unsigned)__builtin_popcountll(w[i]);
    }
    const unsigned total = host_scan(n);
    CHECK(hipMemcpy(d_words, w.data(), 8 * (size_t)n, hipMemcpyHostToDevice));
    for (int with_total = 0; with_total < 2; ++with_total) {
        CHECK(hipMemset(d_total, 0xA5, 4));
        CHECK(exclusive_scan(PopcLoad{d_words}, n, d_out, d_sums, with_total ? d_total : nullptr, 0));
        compare(d_out, n, with_total, total);
    }
}

template <int NW>
static void check_block() {
    const int n = NW * 64;
    for (int i = 0; i < n; ++i) h_in[i] = (unsigned)(i % 5);
    const unsigned total = host_scan(n);
    hipLaunchKernelGGL(block_scan_kernel<NW>, dim3(1), dim3(n), 0, 0, d_out, d_total);
    CHECK(hipGetLastError());
    compare(d_out, n, true, total);
}

int main() {
    const int64_t T = kScanSumsThreads;
    const int64_t trip = kScanTile * T * kScanItems;        // elements behind one trip of the sums loop: 256^3
    const int64_t sizes[] = {1, 255, 256, 257, 2047, 2048, 2049, kScanTile * kScanItems, kScanTile * kScanItems + 1,
                             kScanTile * T - 1, kScanTile * T, kScanTile * T + 1, trip, trip + 1, kMaxN};
    h_in.resize(kMaxN), h_ref.resize(kMaxN), h_out.resize(kMaxN);
    CHECK(hipMalloc(&d_in, 4 * (size_t)kMaxN));
    CHECK(hipMalloc(&d_out, 4 * (size_t)kMaxN));
    CHECK(hipMalloc(&d_sums, 4 * scan_scratch_elems(kMaxN)));
    CHECK(hipMalloc(&d_total, 4));
    CHECK(hipMalloc(&d_words, 8 * (size_t)(kScanTile * T + 1)));

    for (const int64_t n : sizes) {
        for (int64_t i = 0; i < n; ++i) h_in[i] = (unsigned)(i % 7);
        check_u32(n);
        for (int64_t i = 0; i < n; ++i) h_in[i] = 1u;
        check_u32(n);
        for (int64_t i = 0; i < n; ++i) h_in[i] = (i == 0 || i % kScanTile == kScanTile - 1) ? 0x40000001u + (unsigned)i : 0u;
        check_u32(n);
        if (n <= 2049) {
            for (int64_t i = 0; i < n; ++i) h_in[i] = 0xFFFFFFFFu;
            check_u32(n);
        }
    }
    for (int64_t i = 0; i < 4097; ++i) h_in[i] = (unsigned)(i % 7);
    check_u32(4097, 1);                                     // arrays that are not 16-byte aligned
    check_popc(2049);
    check_popc(kScanTile * T + 1);
    check_block<4>();
    check_block<16>();
    CHECK(hipDeviceSynchronize());
    printf("scan: %ld of %ld mismatches\n", g_bad, g_checked);
    return g_bad != 0;
}
