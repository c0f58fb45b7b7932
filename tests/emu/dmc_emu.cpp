// tests/emu/dmc_emu.cpp -- TEST-ONLY host emulation of the HIP dual-marching-cubes launch structure.
//
// Runs the product's per-cell bodies (3d-re-gen_amd/csrc/dmc_cell.h) through the same four passes as
// dmc_kernels.hip -- classify + block compaction, block-offset scan, vertices + cell table, quads -- with the GPU's
// 256-cell blocks replaced by loops.  It lets the CPU suite check cases, the manifold rule, numbering and arithmetic
// against the numpy restatement without a GPU.  It is not part of the product library and never a fallback.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define R3G_DEV static inline
#include "dmc_cell.h"

using namespace r3g_dmc;

extern "C" int r3g_emu_dmc(const float* grid, int n0, int n1, int n2, double level, int manifold, const double* xf9,
                           int reversed, float** verts_out, int32_t** faces_out, int64_t* nV, int64_t* nF,
                           unsigned* flags_out, int64_t* n_flipped) {
    if (n0 < 2 || n1 < 2 || n2 < 2) return -2;
    const Dims d = {n0, n1, n2};
    const int64_t c1 = n1 - 1, c2 = n2 - 1;
    const int64_t ncells = (int64_t)(n0 - 1) * c1 * c2;
    const int64_t nblk = (ncells + 255) / 256;
    std::vector<uint32_t> rec(nblk * 256), loc(nblk * 256);
    std::vector<uint32_t> blkV(nblk), blkQ(nblk), blkA(nblk);
    unsigned flags = 0;
    int64_t flipped = 0;
    // pass 1: classify, in-block exclusive scan, compaction
    for (int64_t b = 0; b < nblk; ++b) {
        uint32_t sv = 0, sq = 0, sa = 0;
        for (int t = 0; t < 256; ++t) {
            const int64_t c = b * 256 + t;
            if (c >= ncells) break;
            const int k = (int)(c % c2), j = (int)((c / c2) % c1), i = (int)(c / (c1 * c2));
            const int cs = cell_case(grid, d, i, j, k, level, &flags);
            const unsigned r = classify_cell(grid, d, i, j, k, level, cs, manifold != 0);
            if (r) {
                if ((int)(r & 0xFFu) != cs) ++flipped;
                rec[b * 256 + sa] = r;
                loc[b * 256 + sa] = (uint32_t)t | (sv << 8) | (sq << 20);
                sv += rec_patches(r);
                sq += rec_quads(r);
                ++sa;
            }
        }
        blkV[b] = sv; blkQ[b] = sq; blkA[b] = sa;
    }
    // pass 2: exclusive scan of the block sums
    std::vector<uint32_t> offV(nblk), offQ(nblk);
    uint64_t tv = 0, tq = 0;
    for (int64_t b = 0; b < nblk; ++b) { offV[b] = (uint32_t)tv; offQ[b] = (uint32_t)tq; tv += blkV[b]; tq += blkQ[b]; }
    *nV = (int64_t)tv; *nF = (int64_t)(2 * tq); *flags_out = flags; *n_flipped = flipped;
    float* verts = (float*)malloc(sizeof(float) * 3 * (tv ? tv : 1));
    int32_t* faces = (int32_t*)malloc(sizeof(int32_t) * 6 * (tq ? tq : 1));
    CellRef poison;
    poison.vbase = 0xFFFFFFFFu; poison.ecase = 0;      // only to catch bugs: the GPU table is uninitialised
    std::vector<CellRef> ctab((size_t)ncells, poison);
    const Xform xf = r3g_surf::xform_from(xf9);
    // pass 3: vertices
    for (int64_t b = 0; b < nblk; ++b)
        for (uint32_t a = 0; a < blkA[b]; ++a) {
            const uint32_t r = rec[b * 256 + a], l = loc[b * 256 + a];
            const int64_t c = b * 256 + (l & 0xFF);
            const int k = (int)(c % c2), j = (int)((c / c2) % c1), i = (int)(c / (c1 * c2));
            emit_cell_vertices(r, offV[b] + ((l >> 8) & 0xFFF), grid, d, i, j, k, level, c, ctab.data(), verts, xf, xf9 != nullptr);
        }
    // pass 4: quads
    for (int64_t b = 0; b < nblk; ++b)
        for (uint32_t a = 0; a < blkA[b]; ++a) {
            const uint32_t r = rec[b * 256 + a], l = loc[b * 256 + a];
            if (rec_quads(r) == 0) continue;
            const int64_t c = b * 256 + (l & 0xFF);
            const int k = (int)(c % c2), j = (int)((c / c2) % c1), i = (int)(c / (c1 * c2));
            emit_cell_quads(r, offQ[b] + (l >> 20), d, i, j, k, ctab.data(), verts, faces, reversed != 0);
        }
    int bad = 0;
    for (uint64_t n = 0; n < 6 * tq; ++n) if (faces[n] < 0 || (uint64_t)faces[n] >= tv) ++bad;
    *verts_out = verts; *faces_out = faces;
    return bad ? -3 : 0;
}

extern "C" void r3g_emu_dmc_free(void* p) { free(p); }
