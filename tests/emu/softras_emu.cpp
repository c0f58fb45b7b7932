// softras_emu.cpp -- host instantiation of csrc/softras_core.h (test only): the bin pass (faces into the 8 x 8 tiles of their
// boxes, in ascending face index), the forward per pixel over its tile's list, and the backward in the product's order: 256
// slots over the pixels of the face's box in raster order, the butterfly over each group of 64 slots, the four groups as
// ((g0 + g1) + g2) + g3, then a vertex's corners in ascending corner index.  Built with -ffp-contract=off, like the kernels.
// `mutant` selects a deliberate departure from the definition (softras_core.h, Mutant), each of which a named scene must expose
// (tests/test_softras_cpu.py).  With -DSOFTRAS_EMU_MAIN it is a stand-alone program (for a sanitizer build) that renders a
// small fan of faces and differentiates it.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "softras_core.h"

using namespace r3g_sr;

namespace {

bool args_ok(int64_t V, int64_t F, int H, int W, int K, float sigma, float blur) {
    return K >= 1 && K <= kMaxK && sigma > 0.0f && sigma - sigma == 0.0f && blur >= 0.0f && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide &&
           V >= 0 && F >= 0;
}

}  // namespace

extern "C" {

int r3g_emu_softras_forward(const float* pos, int64_t V, const int32_t* tri, int64_t F, int H, int W, int K, float sigma, float blur, int mutant,
                            float* alpha, int32_t* face, float* dist, float* zbuf, int64_t* report) {
    if (!args_ok(V, F, H, W, K, sigma, blur)) return -1;
    const float reach = sqrtf(blur);
    const int tx_n = (W + kTile - 1) / kTile, ty_n = (H + kTile - 1) / kTile;
    std::vector<std::vector<int32_t>> bins((size_t)tx_n * ty_n);
    int64_t pairs = 0, used = 0, skipped = 0;
    for (int64_t f = 0; f < F; ++f) {
        Tri T;
        float area;
        if (!load_tri(pos, V, tri, f, &T) || !face_drawn(T, &area)) {
            ++skipped;
            continue;
        }
        const Box b = face_box(T, reach, W, H, mutant);
        if (box_empty(b)) continue;
        ++used;
        for (int ty = b.y0 / kTile; ty <= b.y1 / kTile; ++ty)
            for (int tx = b.x0 / kTile; tx <= b.x1 / kTile; ++tx) bins[(size_t)ty * tx_n + tx].push_back((int32_t)f), ++pairs;
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float lpz[kMaxK], ldist[kMaxK];
            int32_t lface[kMaxK];
            int n = 0;
            for (int32_t f : bins[(size_t)(y / kTile) * tx_n + x / kTile]) {
                Tri T;
                float area;
                if (!load_tri(pos, V, tri, f, &T) || !face_drawn(T, &area)) continue;
                const Frag fr = fragment(T, area, (float)x + 0.5f, (float)y + 0.5f, blur, mutant);
                if (fr.kept) list_insert(lpz, lface, ldist, 1, &n, K, fr.pz, f, fr.dist, mutant);
            }
            const size_t pix = (size_t)y * W + x;
            alpha[pix] = blend(ldist, 1, n, sigma);
            for (int k = 0; k < K; ++k) {
                face[pix * K + k] = k < n ? lface[k] : -1;
                dist[pix * K + k] = k < n ? ldist[k] : -1.0f;
                zbuf[pix * K + k] = k < n ? lpz[k] : -1.0f;
            }
        }
    const int64_t rep[kFwdReport] = {pairs, used, skipped, (int64_t)tx_n * ty_n, 0, 0, 0, 0};
    memcpy(report, rep, sizeof rep);
    return 0;
}

int r3g_emu_softras_backward(const float* pos, int64_t V, const int32_t* tri, int64_t F, int H, int W, int K, float sigma, float blur, int mutant,
                             const int32_t* face, const float* dist, const float* grad_alpha, const int32_t* corner_start,
                             const int32_t* corner_ids, float* grad_face, float* grad_pos, int64_t* report) {
    if (!args_ok(V, F, H, W, K, sigma, blur)) return -1;
    const float reach = sqrtf(blur);
    int64_t found = 0;
    for (int64_t f = 0; f < F; ++f) {
        static float acc[kBackThreads][6];
        memset(acc, 0, sizeof acc);
        Tri T;
        float area;
        if (load_tri(pos, V, tri, f, &T) && face_drawn(T, &area)) {
            const Box b = face_box(T, reach, W, H, mutant);
            if (!box_empty(b)) {
                const int bw = b.x1 - b.x0 + 1, npix = bw * (b.y1 - b.y0 + 1);
                for (int i = 0; i < npix; ++i) {
                    const int y = b.y0 + i / bw, x = b.x0 + i % bw;
                    const size_t pix = (size_t)y * W + x;
                    found += back_pixel(T, area, (float)x + 0.5f, (float)y + 0.5f, blur, sigma, grad_alpha[pix], face + pix * K, dist + pix * K, K,
                                        (int32_t)f, acc[i % kBackThreads], mutant)
                                 ? 1
                                 : 0;
                }
            }
        }
        for (int k = 0; k < 6; ++k) {
            float g[4];
            for (int w = 0; w < 4; ++w) {
                float v[64], nv[64];
                for (int l = 0; l < 64; ++l) v[l] = acc[64 * w + l][k];
                for (int d = 32; d >= 1; d >>= 1) {
                    for (int l = 0; l < 64; ++l) nv[l] = v[l] + v[l ^ d];
                    memcpy(v, nv, sizeof v);
                }
                g[w] = v[0];
            }
            grad_face[f * 6 + k] = ((g[0] + g[1]) + g[2]) + g[3];
        }
    }
    const int64_t nc = 3 * F;
    for (int64_t v = 0; v < V; ++v) {
        int64_t c0 = corner_start[v], c1 = corner_start[v + 1];
        c0 = c0 < 0 ? 0 : c0, c1 = c1 > nc ? nc : c1;
        float gx = 0.0f, gy = 0.0f;
        for (int64_t c = c0; c < c1; ++c) {
            const int32_t id = corner_ids[c];
            if (id < 0 || id >= nc) continue;
            gx = gx + grad_face[2 * (int64_t)id], gy = gy + grad_face[2 * (int64_t)id + 1];
        }
        grad_pos[3 * v] = gx, grad_pos[3 * v + 1] = gy, grad_pos[3 * v + 2] = 0.0f;
    }
    const int64_t rep[kBwdReport] = {found, 0, 0, 0};
    memcpy(report, rep, sizeof rep);
    return 0;
}

void r3g_emu_softras_sigmoid(const float* x, int64_t n, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = sr_sigmoid(x[i]);
}

}  // extern "C"

#ifdef SOFTRAS_EMU_MAIN
#include <stdio.h>
int main() {
    const int H = 19, W = 23, K = 4, F = 6, V = 7;
    float pos[V * 3] = {11.3f, 9.1f, 1.0f};
    int32_t tri[F * 3];
    for (int i = 0; i < 6; ++i) {
        const float a = 1.0471976f * (float)i + 0.2f;
        pos[3 * (i + 1)] = 11.3f + 8.0f * cosf(a), pos[3 * (i + 1) + 1] = 9.1f + 7.0f * sinf(a), pos[3 * (i + 1) + 2] = 1.0f + 0.1f * (float)i;
        tri[3 * i] = 0, tri[3 * i + 1] = 1 + i, tri[3 * i + 2] = 1 + (i + 1) % 6;
    }
    std::vector<float> alpha(H * W), dist(H * W * K), zbuf(H * W * K), ga(H * W, 1.0f), gf(F * 6), gp(V * 3);
    std::vector<int32_t> face(H * W * K), cs(V + 1, 0), ci;
    for (int v = 0; v < V; ++v) {
        for (int c = 0; c < 3 * F; ++c)
            if (tri[c] == v) ci.push_back(c);
        cs[v + 1] = (int32_t)ci.size();
    }
    int64_t rep[8], brep[4];
    if (r3g_emu_softras_forward(pos, V, tri, F, H, W, K, 0.5f, 4.0f, 0, alpha.data(), face.data(), dist.data(), zbuf.data(), rep)) return 1;
    if (r3g_emu_softras_backward(pos, V, tri, F, H, W, K, 0.5f, 4.0f, 0, face.data(), dist.data(), ga.data(), cs.data(), ci.data(), gf.data(), gp.data(),
                                 brep))
        return 1;
    double sum = 0.0, gsum = 0.0;
    for (float a : alpha) sum += a;
    for (int v = 0; v < V; ++v) gsum += gp[3 * v] + gp[3 * v + 1];      // a translation moves no alpha off the image's inside: near 0
    printf("softras selftest: pairs %lld, found %lld, sum alpha %.6f, sum grad %.3e\n", (long long)rep[0], (long long)brep[0], sum, gsum);
    return rep[1] == F && sum > 100.0 && brep[0] > 0 ? 0 : 1;
}
#endif
