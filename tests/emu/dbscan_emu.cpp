// dbscan_emu.cpp -- host instantiation of csrc/dbscan_core.h (test only): (a) all pairs of usable points with the product's
// float64 predicate and visitors, (b) the grid build (csrc/grid_csr.h, host_fill_home) and the radius walk as host loops, with
// either fill order.  Built with -ffp-contract=off, like the kernels.  (a) also takes a `mutant` number: deliberate departures
// from the definition, each of which the test clouds must expose (tests/test_dbscan_cpu.py).  With -DDBSCAN_EMU_MAIN it is a
// stand-alone program (for a sanitizer build) that runs (a) and (b) on a lattice whose every distance ties with eps.
#include <stdint.h>

#include <vector>

#include "dbscan_core.h"

using namespace r3g_db;
using r3g_cl::kInf;

namespace {

enum Mutant { kNone = 0, kStrictLess = 1, kFloat32 = 2, kNotItself = 3, kBorderMax = 4, kFirstAppearance = 5 };

// the records kernel on the host -> skipped
int64_t make_records(const float* pts, int64_t n, std::vector<Pt>& recs, float lo[3], float hi[3]) {
    int64_t skipped = 0;
    for (int a = 0; a < 3; ++a) lo[a] = kInf, hi[a] = -kInf;
    recs.resize(n);
    for (int64_t i = 0; i < n; ++i) {
        Pt p{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], (int32_t)i};
        if (r3g_cl::pt_finite(p.x, p.y, p.z)) {
            lo[0] = r3g_cl::fmin2(lo[0], p.x), lo[1] = r3g_cl::fmin2(lo[1], p.y), lo[2] = r3g_cl::fmin2(lo[2], p.z);
            hi[0] = r3g_cl::fmax2(hi[0], p.x), hi[1] = r3g_cl::fmax2(hi[1], p.y), hi[2] = r3g_cl::fmax2(hi[2], p.z);
        } else {
            p.x = p.y = p.z = 0.0f;
            p.index = -1;
            ++skipped;
        }
        recs[i] = p;
    }
    return skipped;
}

// (a): every usable point against every usable point
struct BruteWalk {
    const std::vector<Pt>& pts;
    double eps2;
    int mutant;
    bool near(const Pt& p, const Pt& q) const {
        if (mutant == kNotItself && p.index == q.index) return false;
        if (mutant == kFloat32) return (double)r3g_cl::dist2(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2;
        if (mutant == kStrictLess) {
            const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
            return ((dx * dx) + dy * dy) + dz * dz < eps2;
        }
        return neighbour(p, q, eps2);
    }
    template <class V>
    uint32_t operator()(const Pt& p, V& visit) const {
        uint32_t tests = 0;
        for (const Pt& q : pts) {
            ++tests;
            if (near(p, q) && !visit(q)) break;
        }
        return tests;
    }
};

// (b): the product's walk
struct GridWalk {
    const Grid& g;
    const std::vector<Pt>& pts;
    const std::vector<uint32_t>& starts;
    double eps, eps2;
    template <class V>
    uint32_t operator()(const Pt& p, V& visit) const {
        return radius_walk(g, pts.data(), starts.data(), p, eps, eps2, visit);
    }
};

// the union-find of the device in one thread: the larger root goes under the smaller one
struct HostUnite {
    int32_t* parent;
    int32_t find(int32_t x) const {
        while (parent[x] != x) x = parent[x];
        return x;
    }
    void operator()(int32_t a, int32_t b) {
        a = find(a), b = find(b);
        if (a == b) return;
        if (a > b) parent[a] = b;
        else parent[b] = a;
    }
};

struct BorderMaxVisitor {       // mutant
    const uint8_t* core;
    const int32_t* root;
    int32_t best;
    bool operator()(const Pt& q) {
        if (core[q.index]) best = (best == r3g_cl::kNoIndex || root[q.index] > best) ? root[q.index] : best;
        return true;
    }
};

// the passes of dbscan_kernels.hip in host loops over `pts` (the usable points, in the order the walk owns)
template <class Walk>
void run(const Walk& walk, const std::vector<Pt>& pts, int64_t n, uint32_t min_samples, bool early, int mutant, int32_t* label,
         uint32_t* count, uint8_t* core, int64_t* report, int64_t* tests_out) {
    std::vector<int32_t> root(n, -1);
    std::vector<uint32_t> number(n + 1, 0), size(n + 1, 0);
    int64_t tests = 0, n_core = 0, n_border = 0;
    for (int64_t i = 0; i < n; ++i) label[i] = -1, count[i] = 0, core[i] = 0;
    for (const Pt& p : pts) {
        CountVisitor v{0u, early ? min_samples : 0xffffffffu};
        tests += walk(p, v);
        count[p.index] = v.count;
        if (v.count >= min_samples) core[p.index] = 1, root[p.index] = p.index, ++n_core;
    }
    HostUnite unite{root.data()};
    for (const Pt& p : pts) {
        if (!core[p.index]) continue;
        LinkVisitor<HostUnite> v{core, p.index, unite};
        tests += walk(p, v);
    }
    for (int64_t i = 0; i < n; ++i)
        if (root[i] >= 0) root[i] = unite.find((int32_t)i);
    std::vector<int32_t> border(n, -1);     // written after the pass: a border point must not see another's root
    for (const Pt& p : pts) {
        if (core[p.index]) continue;
        int32_t best;
        if (mutant == kBorderMax) {
            BorderMaxVisitor v{core, root.data(), r3g_cl::kNoIndex};
            tests += walk(p, v);
            best = v.best;
        } else {
            BorderVisitor v{core, root.data(), r3g_cl::kNoIndex};
            tests += walk(p, v);
            best = v.best;
        }
        if (best != r3g_cl::kNoIndex) border[p.index] = best, ++n_border;
    }
    for (int64_t i = 0; i < n; ++i)
        if (border[i] >= 0) root[i] = border[i];
    uint32_t n_clusters = 0;
    if (mutant == kFirstAppearance) {
        std::vector<int32_t> seen(n, -1);
        for (int64_t i = 0; i < n; ++i)
            if (root[i] >= 0 && seen[root[i]] < 0) seen[root[i]] = (int32_t)n_clusters++;
        for (int64_t i = 0; i < n; ++i)
            if (seen[i] >= 0) number[i] = (uint32_t)seen[i];
    } else {
        for (int64_t i = 0; i < n; ++i) {      // the exclusive scan of the root flags
            number[i] = n_clusters;
            n_clusters += root_flag(root.data(), i);
        }
    }
    uint64_t best = 0;
    for (int64_t i = 0; i < n; ++i) {
        label[i] = label_of(root.data(), number.data(), i);
        if (label[i] >= 0) ++size[label[i]];
    }
    for (uint32_t c = 0; c < n_clusters; ++c) {
        const uint64_t b = pack_best(size[c], (int32_t)c);
        best = b > best ? b : best;
    }
    const int64_t usable = (int64_t)pts.size();
    report[0] = usable, report[1] = n_core, report[2] = n_border, report[3] = usable - n_core - n_border;
    report[4] = n_clusters, report[5] = best_label(best), report[6] = best_size(best);
    if (tests_out) *tests_out = tests;
}

}  // namespace

extern "C" {

// label int32 [n], count uint32 [n], core uint8 [n], report int64 [8].  grid == 0: (a), `mutant` applies; otherwise (b) at
// `resolution` (0 = automatic) with `reverse_fill`.  early != 0: a point stops counting at min_samples (count[] is then capped).
int r3g_emu_dbscan(const float* pts, int64_t n, double eps, int min_samples, int grid, int resolution, int reverse_fill, int early,
                   int mutant, int32_t* label, uint32_t* count, uint8_t* core, int64_t* report, int64_t* tests_out) {
    if (!(eps > 0.0) || !(eps - eps == 0.0) || min_samples < 1 || n < 0 || n >= (1ll << 31)) return -1;
    if (resolution < 0 || resolution > r3g_cl::kMaxRes) return -1;
    const int64_t zero[kReport] = {0, 0, 0, 0, 0, -1, 0, 0};
    for (int j = 0; j < kReport; ++j) report[j] = zero[j];
    if (tests_out) *tests_out = 0;
    std::vector<Pt> recs;
    float lo[3], hi[3];
    const int64_t skipped = make_records(pts, n, recs, lo, hi);
    for (int64_t i = 0; i < n; ++i) label[i] = -1, count[i] = 0, core[i] = 0;
    if (skipped >= n) return 0;
    const double eps2 = eps * eps;
    if (!grid) {
        std::vector<Pt> usable;
        for (const Pt& p : recs)
            if (r3g_cl::grid_member(p)) usable.push_back(p);
        const BruteWalk walk{usable, eps2, mutant};
        run(walk, usable, n, (uint32_t)min_samples, early != 0, mutant, label, count, core, report, tests_out);
        return 0;
    }
    const int res = resolution ? resolution : auto_resolution(lo, hi, eps, n - skipped);
    const Grid g = r3g_grid::make_grid(lo, hi, res);
    const int64_t cells = r3g_grid::cells<3>(res);
    std::vector<uint32_t> starts(cells + 1, 0), cursor(cells, 0);
    std::vector<Pt> sorted(n - skipped);
    r3g_grid::host_fill_home(g, recs.data(), n, reverse_fill != 0, starts.data(), cursor.data(), sorted.data());
    const GridWalk walk{g, sorted, starts, eps, eps2};
    run(walk, sorted, n, (uint32_t)min_samples, early != 0, kNone, label, count, core, report, tests_out);
    report[7] = res;
    return 0;
}

int r3g_emu_dbscan_auto_resolution(const float* lo, const float* hi, double eps, int64_t n_usable) { return auto_resolution(lo, hi, eps, n_usable); }

}  // extern "C"

#ifdef DBSCAN_EMU_MAIN
#include <math.h>
#include <stdio.h>
#include <string.h>

// the 9^3 lattice of spacing 0.25 at eps = 0.25 (every distance ties with eps), a non-finite row and a far point
int main() {
    std::vector<float> pts;
    for (int z = 0; z < 9; ++z)
        for (int y = 0; y < 9; ++y)
            for (int x = 0; x < 9; ++x) pts.push_back(0.25f * x), pts.push_back(0.25f * y), pts.push_back(0.25f * z);
    const float extra[6] = {NAN, 0.5f, 0.5f, 40.0f, -3.0f, 7.0f};
    pts.insert(pts.begin() + 30, extra, extra + 3);
    pts.insert(pts.end(), extra + 3, extra + 6);
    const int64_t n = (int64_t)pts.size() / 3;
    int bad = 0;
    for (int min_samples : {1, 6, 7})
        for (int early = 0; early < 2; ++early) {
            std::vector<int32_t> la(n), lb(n);
            std::vector<uint32_t> ca(n), cb(n);
            std::vector<uint8_t> ka(n), kb(n);
            int64_t ra[kReport], rb[kReport];
            if (r3g_emu_dbscan(pts.data(), n, 0.25, min_samples, 0, 0, 0, early, 0, la.data(), ca.data(), ka.data(), ra, nullptr)) return 2;
            for (int res : {0, 1, 3, 16, 256})
                for (int rev = 0; rev < 2; ++rev) {
                    if (r3g_emu_dbscan(pts.data(), n, 0.25, min_samples, 1, res, rev, early, 0, lb.data(), cb.data(), kb.data(), rb, nullptr)) return 2;
                    bad += memcmp(la.data(), lb.data(), 4 * n) != 0 || memcmp(ka.data(), kb.data(), n) != 0 || memcmp(ra, rb, 7 * 8) != 0;
                    if (!early) bad += memcmp(ca.data(), cb.data(), 4 * n) != 0;
                }
            if (min_samples == 7) bad += ra[4] != 1 || ra[1] != 343;       // the interior 7^3 points have 7 neighbours
        }
    printf("dbscan_emu lattice: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
