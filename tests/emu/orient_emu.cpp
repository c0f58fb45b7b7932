// orient_emu.cpp -- host instantiation of csrc/orient_core.h (test only): the Boruvka rounds of the normal orientation
//  as host loops over the bodies the kernels run, on the (k + 1)-rows the caller took from the cloud twin.
// `reverse` walks every loop in the opposite order: the minima are over a total order, so the scan order must not matter.
// Built with -ffp-contract=off, like the kernels.  With -DORIENT_EMU_MAIN it is a stand-alone program (for a sanitizer build).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "orient_core.h"

using namespace r3g_or;

extern "C" {

// points, normals float32 [n][3]; rows int32 [n][k + 1] (the row of a point that is not usable is not read)
// -> sign int8 [n], tree int32 [n], report int64 [8]; -1 for a refused argument
int r3g_emu_orient(const float* pts, const float* nrm, int64_t n, int k, const int32_t* rows, int reverse, int8_t* sign, int32_t* tree,
                   int64_t* report) {
    if (n <= 0 || k < kMinK || k > kMaxK) return -1;
    std::vector<float> unit(3 * n, 0.0f);
    std::vector<int32_t> comp(n), comp2(n);
    std::vector<uint8_t> par(n, 0), par2(n);
    int64_t usable = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool ok = r3g_rc::usable(pts + 3 * i, nrm + 3 * i);
        if (ok) r3g_rc::unit_normal(nrm + 3 * i, &unit[3 * i]), ++usable;
        comp[i] = ok ? (int32_t)i : -1;
    }
    auto each = [&](auto f) {
        for (int64_t t = 0; t < n; ++t) f(reverse ? n - 1 - t : t);
    };
    std::vector<uint32_t> best_w(n);
    std::vector<uint64_t> best_pair(n);
    int64_t rounds = 0;
    while (usable > 0) {
        if (rounds >= 64) return -2;
        each([&](int64_t i) { best_w[i] = kNoWeight, best_pair[i] = kNoPair; });
        for (int pairs = 0; pairs < 2; ++pairs)
            each([&](int64_t i) {
                const int32_t ci = comp[i];
                if (ci < 0) return;
                each_neighbour(rows + i * (k + 1), k, (int32_t)i, [&](int32_t j) {
                    const int32_t cj = comp[j];
                    if (cj == ci) return;
                    const uint32_t w = weight_bits(dot3(&unit[3 * i], &unit[3 * (int64_t)j]));
                    if (!pairs) {
                        if (w < best_w[ci]) best_w[ci] = w;
                        if (w < best_w[cj]) best_w[cj] = w;
                    } else {
                        const uint64_t p = pack_pair((int32_t)i, j);
                        if (best_w[ci] == w && p < best_pair[ci]) best_pair[ci] = p;
                        if (best_w[cj] == w && p < best_pair[cj]) best_pair[cj] = p;
                    }
                });
            });
        int64_t merged = 0;
        each([&](int64_t i) {
            int32_t c = comp[i], to;
            uint8_t p = par[i], pt;
            if (c == (int32_t)i && hook((int32_t)i, best_pair[i], comp.data(), par.data(), best_pair.data(), unit.data(), &to, &pt))
                c = to, p = pt, ++merged;
            comp2[i] = c, par2[i] = p;
        });
        int steps = 1;
        while (((int64_t)1 << steps) < n) ++steps;
        steps |= 1;
        for (int t = 0; t < steps; ++t) {
            std::vector<int32_t>&from_c = t & 1 ? comp : comp2, &to_c = t & 1 ? comp2 : comp;
            std::vector<uint8_t>&from_p = t & 1 ? par : par2, &to_p = t & 1 ? par2 : par;
            each([&](int64_t i) {
                const int32_t c = from_c[i];
                to_c[i] = c < 0 ? -1 : from_c[c];
                to_p[i] = c < 0 ? (uint8_t)0 : (uint8_t)(from_p[i] ^ from_p[c]);
            });
        }
        ++rounds;
        if (!merged) break;
    }
    std::vector<int32_t> tree_min(n, 0x7fffffff);
    std::vector<uint64_t> top(n, 0);
    each([&](int64_t i) {
        const int32_t c = comp[i];
        if (c < 0) return;
        if ((int32_t)i < tree_min[c]) tree_min[c] = (int32_t)i;
        const uint64_t key = top_key(pts[3 * i + 2], (int32_t)i);
        if (key > top[c]) top[c] = key;
    });
    int64_t trees = 0, flipped = 0, bad = 0;
    each([&](int64_t i) {
        const int32_t c = comp[i];
        if (c < 0) {
            sign[i] = 0, tree[i] = -1;
            return;
        }
        const int32_t t = top_index(top[c]);
        const int bit = (nrm[3 * (int64_t)t + 2] < 0.0f ? 1 : 0) ^ par[t] ^ par[i];
        sign[i] = bit ? -1 : 1;
        tree[i] = tree_min[c];
        flipped += bit, trees += c == (int32_t)i;
    });
    each([&](int64_t i) {
        if (sign[i] == 0) return;
        each_neighbour(rows + i * (k + 1), k, (int32_t)i, [&](int32_t j) {
            if (!frustrated(sign, unit.data(), (int32_t)i, j)) return;
            if ((int32_t)i < j || !has_neighbour(rows + (int64_t)j * (k + 1), k, j, (int32_t)i)) ++bad;
        });
    });
    if (report) {
        const int64_t r[kReport] = {usable, trees, flipped, rounds, bad, 0, 0, 0};
        memcpy(report, r, sizeof r);
    }
    return 0;
}

}  // extern "C"

#ifdef ORIENT_EMU_MAIN
#include <math.h>
#include <stdio.h>

#include <algorithm>

// a 300-point sphere with coin-flipped exact normals and a few unusable points, rows by brute force, forward and reversed:
// the two runs must agree and every usable normal must end pointing outward
int main() {
    const int n = 300, k = 6;
    std::vector<float> pts, nrm;
    for (int i = 0; i < n; ++i) {
        const double z = 1.0 - (2.0 * i + 1.0) / n, r = sqrt(1.0 - z * z), a = 2.399963229728653 * i;
        const float p[3] = {(float)(r * cos(a)), (float)(r * sin(a)), (float)z};
        const float s = (i * 2654435761u >> 7) & 1 ? -1.0f : 1.0f;
        for (int c = 0; c < 3; ++c) pts.push_back(p[c]), nrm.push_back(s * p[c]);
    }
    pts[3 * 7] = __builtin_nanf(""), nrm[3 * 11] = nrm[3 * 11 + 1] = nrm[3 * 11 + 2] = 0.0f;
    std::vector<int32_t> rows((size_t)n * (k + 1), -1);
    for (int i = 0; i < n; ++i) {
        if (!r3g_rc::usable(&pts[3 * i], &nrm[3 * i])) continue;
        std::vector<std::pair<float, int32_t>> d;
        for (int j = 0; j < n; ++j) {
            if (!r3g_rc::usable(&pts[3 * j], &nrm[3 * j])) continue;
            const float dx = pts[3 * i] - pts[3 * j], dy = pts[3 * i + 1] - pts[3 * j + 1], dz = pts[3 * i + 2] - pts[3 * j + 2];
            d.push_back({(dx * dx + dy * dy) + dz * dz, j});
        }
        std::sort(d.begin(), d.end());
        for (int s = 0; s <= k && s < (int)d.size(); ++s) rows[(size_t)i * (k + 1) + s] = d[s].second;
    }
    std::vector<int8_t> sa(n), sb(n);
    std::vector<int32_t> ta(n), tb(n);
    int64_t ra[kReport], rb[kReport];
    int bad = r3g_emu_orient(pts.data(), nrm.data(), n, k, rows.data(), 0, sa.data(), ta.data(), ra) != 0;
    bad += r3g_emu_orient(pts.data(), nrm.data(), n, k, rows.data(), 1, sb.data(), tb.data(), rb) != 0;
    bad += sa != sb || ta != tb || memcmp(ra, rb, sizeof ra) != 0 || ra[0] != n - 2 || ra[1] != 1 || ra[4] != 0;
    for (int i = 0; i < n; ++i) {
        if (sa[i] == 0) continue;
        const float out = (nrm[3 * i] * pts[3 * i] + nrm[3 * i + 1] * pts[3 * i + 1]) + nrm[3 * i + 2] * pts[3 * i + 2];
        bad += !(sa[i] * out > 0.0f);
    }
    printf("orient_emu sphere: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
