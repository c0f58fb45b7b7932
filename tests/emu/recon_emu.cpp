// recon_emu.cpp -- host instantiation of csrc/recon_core.h (test only): splat, divergence, the V-cycles and the sample of the
// Poisson surface as host loops over the same per-element bodies the kernels run.  Built with
// -ffp-contract=off, like the kernels.  `reverse` walks the points in the opposite order (integer sums: it must not matter).
// `mutant` breaks the solver on purpose, to show that the tests' tolerance can fail: 1 = restriction weights 1/8 on every fine
// node, 2 = no smoothing after the correction.  With -DRECON_EMU_MAIN it is a stand-alone program (for a sanitizer build).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "recon_core.h"

using namespace r3g_rc;

namespace {

int64_t nodes(int d) {
    const int64_t n = (1 << d) + 1;
    return n * n * n;
}

struct HostAdd {
    int64_t* ch;
    int64_t n3;
    void operator()(int c, int64_t at, int64_t v) { ch[c * n3 + at] += v; }
};

template <class F>
void each_node(int n, F f) {
    for (int i0 = 0; i0 < n; ++i0)
        for (int i1 = 0; i1 < n; ++i1)
            for (int i2 = 0; i2 < n; ++i2) f(i0, i1, i2);
}

// x (level depth) = `cycles` V-cycles on b from 0
void vcycles(int depth, double side, const float* b_in, int cycles, int mutant, float* x_out) {
    std::vector<std::vector<float>> x(depth + 1), t(depth + 1), b(depth + 1);
    float h2[kMaxDepth + 1], inv_h2[kMaxDepth + 1];
    for (int d = 1; d <= depth; ++d) {
        x[d].assign(nodes(d), 0.0f), t[d].assign(nodes(d), 0.0f), b[d].assign(nodes(d), 0.0f);
        level_h2(depth, side, d, &h2[d], &inv_h2[d]);
    }
    memcpy(b[depth].data(), b_in, sizeof(float) * nodes(depth));
    const float good[4] = R3G_RC_FULL_WEIGHTS, bad[4] = {0.125f, 0.125f, 0.125f, 0.125f};
    const float* w4 = mutant == 1 ? bad : good;
    auto sweeps = [&](int d) {
        const int n = (1 << d) + 1;
        each_node(n, [&](int i0, int i1, int i2) { t[d][node(n, i0, i1, i2)] = smooth_node(x[d].data(), b[d].data(), n, h2[d], i0, i1, i2); });
        each_node(n, [&](int i0, int i1, int i2) { x[d][node(n, i0, i1, i2)] = smooth_node(t[d].data(), b[d].data(), n, h2[d], i0, i1, i2); });
    };
    for (int c = 0; c < cycles; ++c) {
        for (int d = depth; d >= 2; --d) {
            sweeps(d);
            const int nf = (1 << d) + 1, nc = (nf + 1) / 2;
            each_node(nc, [&](int i0, int i1, int i2) {
                b[d - 1][node(nc, i0, i1, i2)] = restrict_node(x[d].data(), b[d].data(), nf, inv_h2[d], w4, i0, i1, i2);
                x[d - 1][node(nc, i0, i1, i2)] = 0.0f;
            });
        }
        x[1][13] = coarsest_value(b[1][13], h2[1]);
        for (int d = 2; d <= depth; ++d) {
            const int nf = (1 << d) + 1;
            each_node(nf, [&](int i0, int i1, int i2) {
                x[d][node(nf, i0, i1, i2)] = prolong_node(x[d].data(), x[d - 1].data(), nf, i0, i1, i2);
            });
            if (mutant != 2) sweeps(d);
        }
    }
    memcpy(x_out, x[depth].data(), sizeof(float) * nodes(depth));
}

}  // namespace

extern "C" {

// channels int64 [4][n^3] (zeroed here) -> usable points, or -1 for a refused argument
int64_t r3g_emu_recon_splat(const float* pts, const float* nrm, int64_t n, int depth, const double* centre, double side, int reverse,
                            int64_t* channels) {
    if (n <= 0 || depth < kMinDepth || depth > kMaxDepth || !(side > 0.0)) return -1;
    const Lattice L = make_lattice(depth, centre, side);
    const int64_t n3 = nodes(depth);
    memset(channels, 0, sizeof(int64_t) * kChannels * n3);
    HostAdd add{channels, n3};
    int64_t used = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t i = reverse ? n - 1 - j : j;
        if (!usable(pts + 3 * i, nrm + 3 * i)) continue;
        splat_point(L, pts + 3 * i, nrm + 3 * i, add);
        ++used;
    }
    return used;
}

// b float32 [n^3] from the channels
int r3g_emu_recon_rhs(const int64_t* channels, int depth, const double* centre, double side, float* b) {
    if (depth < kMinDepth || depth > kMaxDepth) return -1;
    const Lattice L = make_lattice(depth, centre, side);
    each_node(L.n, [&](int i0, int i1, int i2) { b[node(L.n, i0, i1, i2)] = rhs_node(channels, L, i0, i1, i2); });
    return 0;
}

// chi float32 [n^3] after `cycles` V-cycles on b
int r3g_emu_recon_vcycles(const float* b, int depth, double side, int cycles, int mutant, float* chi) {
    if (depth < kMinDepth || depth > kMaxDepth || cycles < 0) return -1;
    vcycles(depth, side, b, cycles, mutant, chi);
    return 0;
}

// trilinear sample of the density channel (field 0: `data` is int64 [n^3]) or of a float32 lattice (field 1) -> values [n]
// (may be null), *sum_out the fixed-point sum, return the number of points in it (-1: refused)
int64_t r3g_emu_recon_sample(int field, const void* data, int depth, const double* centre, double side, const float* pts, const float* nrm,
                             int64_t n, int reverse, float* values, int64_t* sum_out) {
    if (depth < kMinDepth || depth > kMaxDepth || n <= 0) return -1;
    const Lattice L = make_lattice(depth, centre, side);
    const int64_t* ch = (const int64_t*)data;
    const float* x = (const float*)data;
    uint64_t sum = 0;
    int64_t used = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t i = reverse ? n - 1 - j : j;
        const bool ok = finite3(pts + 3 * i) && (!nrm || usable(pts + 3 * i, nrm + 3 * i));
        float v = __builtin_nanf("");
        if (ok) {
            v = field == 0 ? sample_point(L, pts + 3 * i, [&](int64_t at) { return from_fixed(ch[at]); })
                           : sample_point(L, pts + 3 * i, [&](int64_t at) { return x[at]; });
            if (finite1(v)) ++used, sum += (uint64_t)to_fixed(v);
        }
        if (values) values[i] = v;
    }
    if (sum_out) *sum_out = (int64_t)sum;
    return used;
}

}  // extern "C"

#ifdef RECON_EMU_MAIN
#include <stdio.h>

// a small sphere at depth 3 and 4, forward and reversed: the channels and the level sum must not depend on the order, the
// solve must reduce the residual, and a sample at the box corners must stay inside the lattice
int main() {
    std::vector<float> pts, nrm;
    for (int i = 0; i < 500; ++i) {
        const double z = 1.0 - (2.0 * i + 1.0) / 500.0, r = sqrt(1.0 - z * z), a = 2.399963229728653 * i;
        const float p[3] = {(float)(r * cos(a)), (float)(r * sin(a)), (float)z};
        for (int c = 0; c < 3; ++c) pts.push_back(p[c]), nrm.push_back(2.0f * p[c]);
    }
    pts[3] = __builtin_nanf(""), nrm[7] = __builtin_inff(), nrm[9] = nrm[10] = nrm[11] = 0.0f;
    const double centre[3] = {0.0, 0.0, 0.0};
    int bad = 0;
    for (int depth = 2; depth <= 4; ++depth) {
        const int n = (1 << depth) + 1;
        const double side = 2.0 * (n - 1) / (n - 5 > 0 ? n - 5 : 1);
        const int64_t n3 = nodes(depth);
        std::vector<int64_t> a(4 * n3), b(4 * n3);
        const int64_t ua = r3g_emu_recon_splat(pts.data(), nrm.data(), 500, depth, centre, side, 0, a.data());
        const int64_t ub = r3g_emu_recon_splat(pts.data(), nrm.data(), 500, depth, centre, side, 1, b.data());
        bad += ua != 497 || ub != 497 || memcmp(a.data(), b.data(), 8 * a.size()) != 0;
        std::vector<float> rhs(n3), chi(n3), chi0(n3);
        bad += r3g_emu_recon_rhs(a.data(), depth, centre, side, rhs.data()) != 0;
        for (int m = 0; m < 3; ++m) bad += r3g_emu_recon_vcycles(rhs.data(), depth, side, 3, m, chi.data()) != 0;
        r3g_emu_recon_vcycles(rhs.data(), depth, side, 10, 0, chi.data());
        int64_t s0 = 0, s1 = 0;
        std::vector<float> v(500);
        const int64_t c0 = r3g_emu_recon_sample(1, chi.data(), depth, centre, side, pts.data(), nrm.data(), 500, 0, v.data(), &s0);
        const int64_t c1 = r3g_emu_recon_sample(1, chi.data(), depth, centre, side, pts.data(), nrm.data(), 500, 1, nullptr, &s1);
        bad += c0 != 497 || c1 != 497 || s0 != s1;
        const float corners[12] = {(float)side, (float)side, (float)side, -(float)side, 0.0f, 3e38f, -3e38f, 3e38f, 0.0f, 0.0f, 0.0f, 0.0f};
        bad += r3g_emu_recon_sample(0, a.data(), depth, centre, side, corners, nullptr, 4, 0, v.data(), &s0) != 4;
    }
    printf("recon_emu sphere: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
