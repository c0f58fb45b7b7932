// cloud_emu.cpp -- host instantiation of csrc/cloud_core.h (test only): (a) the brute force over every usable point with the
// product's float32 dist2 and k-list, (b) the grid build (csrc/grid_csr.h, host_fill_home) and the ring walk as host loops.
// Built with -ffp-contract=off, like the kernels.  With -DCLOUD_EMU_MAIN it is a stand-alone program (for a sanitizer build)
// that runs (a) and (b) on a lattice whose every point sits on a cell border and compares them.
#include <stdint.h>

#include <vector>

#include "cloud_core.h"

using namespace r3g_cl;

namespace {

// a k-list in an array: the host's store
struct ArrayStore {
    float d[kMaxK];
    int32_t i[kMaxK];
    float get_d(int j) const { return d[j]; }
    int32_t get_i(int j) const { return i[j]; }
    void set(int j, float v, int32_t x) { d[j] = v, i[j] = x; }
};

// the records kernel on the host -> skipped
int64_t make_records(const float* pts, int64_t n, std::vector<Pt>& recs, float lo[3], float hi[3]) {
    int64_t skipped = 0;
    for (int a = 0; a < 3; ++a) lo[a] = kInf, hi[a] = -kInf;
    recs.resize(n);
    for (int64_t i = 0; i < n; ++i) {
        Pt p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], (int32_t)i};
        if (pt_finite(p.x, p.y, p.z)) {
            lo[0] = fmin2(lo[0], p.x), lo[1] = fmin2(lo[1], p.y), lo[2] = fmin2(lo[2], p.z);
            hi[0] = fmax2(hi[0], p.x), hi[1] = fmax2(hi[1], p.y), hi[2] = fmax2(hi[2], p.z);
        } else {
            p.x = p.y = p.z = 0.0f;
            p.index = -1;
            ++skipped;
        }
        recs[i] = p;
    }
    return skipped;
}

}  // namespace

extern "C" {

// (a) every usable point, no grid
int r3g_emu_cloud_brute(const float* pts, int64_t n, const float* q, int64_t nq, int k, float* dist2, int32_t* index, int64_t* skipped_out) {
    if (n <= 0 || k < 1 || k > kMaxK) return -1;
    std::vector<Pt> recs;
    float lo[3], hi[3];
    const int64_t skipped = make_records(pts, n, recs, lo, hi);
    if (skipped >= n) return -1;
    for (int64_t i = 0; i < nq; ++i) {
        const float px = q[3 * i], py = q[3 * i + 1], pz = q[3 * i + 2];
        if (!pt_finite(px, py, pz)) {
            for (int j = 0; j < k; ++j) dist2[i * k + j] = quiet_nan(), index[i * k + j] = -1;
            continue;
        }
        ArrayStore st;
        KList<false, ArrayStore> list(st, k);
        for (int64_t m = 0; m < n; ++m)
            if (grid_member(recs[m])) list.offer(r3g_cl::dist2(px, py, pz, recs[m].x, recs[m].y, recs[m].z), recs[m].index);
        for (int j = 0; j < k; ++j) {
            dist2[i * k + j] = list.d_at(j);
            index[i * k + j] = list.i_at(j) == kNoIndex ? -1 : list.i_at(j);
        }
    }
    if (skipped_out) *skipped_out = skipped;
    return 0;
}

// (b) the product's build and query in host loops; `reverse_fill` fills the cells in the opposite point order (the order
// inside a cell, which integer atomics decide on the device, must not matter).  k == 1 takes the register path of the kernels.
int r3g_emu_cloud_grid(const float* pts, int64_t n, int resolution, int reverse_fill, const float* q, int64_t nq, int k, float* dist2,
                       int32_t* index, int* resolution_out, int64_t* skipped_out, int64_t* tests_out) {
    if (n <= 0 || k < 1 || k > kMaxK || resolution < 0 || resolution > kMaxRes) return -1;
    std::vector<Pt> recs;
    float lo[3], hi[3];
    const int64_t skipped = make_records(pts, n, recs, lo, hi);
    if (skipped >= n) return -1;
    const int res = resolution ? resolution : auto_resolution(n - skipped, kPointsPerCell);
    const Grid g = r3g_grid::make_grid(lo, hi, res);
    const int64_t cells = r3g_grid::cells<3>(res);
    std::vector<uint32_t> starts(cells + 1, 0), cursor(cells, 0);
    std::vector<Pt> sorted(n - skipped);
    r3g_grid::host_fill_home(g, recs.data(), n, reverse_fill != 0, starts.data(), cursor.data(), sorted.data());
    int64_t tests = 0;
    for (int64_t i = 0; i < nq; ++i) {
        uint32_t nt = 0;
        if (k == 1) {
            NoStore st;
            knn<true>(g, sorted.data(), starts.data(), q[3 * i], q[3 * i + 1], q[3 * i + 2], 1, st, dist2 + i, index + i, &nt);
        } else {
            ArrayStore st;
            knn<false>(g, sorted.data(), starts.data(), q[3 * i], q[3 * i + 1], q[3 * i + 2], k, st, dist2 + i * k, index + i * k, &nt);
        }
        tests += nt;
    }
    if (resolution_out) *resolution_out = g.res;
    if (skipped_out) *skipped_out = skipped;
    if (tests_out) *tests_out = tests;
    return 0;
}

// per_cell 0: the product's kPointsPerCell
int r3g_emu_cloud_auto_resolution(int64_t n_usable, int per_cell) { return auto_resolution(n_usable, per_cell ? per_cell : kPointsPerCell); }

}  // extern "C"

#ifdef CLOUD_EMU_MAIN
#include <stdio.h>
#include <string.h>

// the 9^3 lattice at forced resolution 8 (every point on a cell border), queried by itself and by points far outside
int main() {
    std::vector<float> pts, q;
    for (int z = 0; z < 9; ++z)
        for (int y = 0; y < 9; ++y)
            for (int x = 0; x < 9; ++x) pts.push_back(0.125f * x), pts.push_back(0.125f * y), pts.push_back(0.125f * z);
    q = pts;
    const float far[6] = {-50.0f, 0.5f, 0.5f, 3.0f, 4.0f, -7.0f};
    q.insert(q.end(), far, far + 6);
    const int64_t n = (int64_t)pts.size() / 3, nq = (int64_t)q.size() / 3;
    int bad = 0;
    for (int k : {1, 8, 32})
        for (int rev = 0; rev < 2; ++rev) {
            std::vector<float> da(nq * k), db(nq * k);
            std::vector<int32_t> ia(nq * k), ib(nq * k);
            if (r3g_emu_cloud_brute(pts.data(), n, q.data(), nq, k, da.data(), ia.data(), nullptr)) return 2;
            if (r3g_emu_cloud_grid(pts.data(), n, 8, rev, q.data(), nq, k, db.data(), ib.data(), nullptr, nullptr, nullptr)) return 2;
            bad += memcmp(da.data(), db.data(), 4 * da.size()) != 0 || memcmp(ia.data(), ib.data(), 4 * ia.size()) != 0;
        }
    printf("cloud_emu lattice: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
