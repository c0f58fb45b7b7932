// meshdist_host.h -- the target of the distance twins (meshdist_emu.cpp, meshfit_emu.cpp; test only): triangle records and
// their bounding box the way md_records makes them.
#ifndef R3G_EMU_MESHDIST_HOST_H
#define R3G_EMU_MESHDIST_HOST_H
#include "host_grid.h"
#include "meshdist_core.h"

using Target = HostGrid<3, r3g_md::Tri>;

// -> number of skipped faces, or -2 for an index outside [0, nv)
static inline int64_t make_records(const float* v, int64_t nv, const int32_t* f, int64_t nf, std::vector<r3g_md::Tri>& tris, float lo[3],
                                   float hi[3]) {
    using namespace r3g_md;
    uint32_t elo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, ehi[3] = {0, 0, 0};
    int64_t skipped = 0;
    tris.resize(nf);
    for (int64_t i = 0; i < nf; ++i) {
        Tri t{};
        const int32_t i0 = f[3 * i], i1 = f[3 * i + 1], i2 = f[3 * i + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return -2;
        t.ax = v[3 * i0], t.ay = v[3 * i0 + 1], t.az = v[3 * i0 + 2];
        t.bx = v[3 * i1], t.by = v[3 * i1 + 1], t.bz = v[3 * i1 + 2];
        t.cx = v[3 * i2], t.cy = v[3 * i2 + 1], t.cz = v[3 * i2 + 2];
        if (tri_finite(t)) {
            t.valid = 1;
            const float c[9] = {t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz};
            for (int k = 0; k < 9; ++k) {
                const uint32_t e = r3g_grid::enc_float(c[k]);
                if (e < elo[k % 3]) elo[k % 3] = e;
                if (e > ehi[k % 3]) ehi[k % 3] = e;
            }
        } else {
            ++skipped;
        }
        tris[i] = t;
    }
    for (int a = 0; a < 3; ++a) lo[a] = r3g_grid::dec_float(elo[a]), hi[a] = r3g_grid::dec_float(ehi[a]);
    return skipped;
}
#endif
