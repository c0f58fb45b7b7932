// host_grid.h -- what a twin holds of a grid in CSR form (test only): the records, and the build of csrc/grid_csr.h
// (resolution rule, count pass, prefix sum, fill pass) run as host loops.
#ifndef R3G_EMU_HOST_GRID_H
#define R3G_EMU_HOST_GRID_H
#include <stdint.h>

#include <vector>

#include "grid_csr.h"

template <int D, class R>
struct HostGrid {
    std::vector<R> recs;
    std::vector<uint32_t> starts;
    std::vector<int32_t> list;
    r3g_grid::GridN<D> g;
    int64_t pairs = 0;

    // lo / hi: the box of the usable records; resolution 0: from `initial` by the automatic rule
    void build(const float (&lo)[D], const float (&hi)[D], int resolution, int initial, bool reverse_fill) {
        const int64_t nf = (int64_t)recs.size();
        r3g_grid::choose_resolution(lo, hi, resolution, initial, nf, [&](const r3g_grid::GridN<D>& cand, int64_t* n) {
            *n = r3g_grid::host_pairs(cand, recs.data(), nf);
            return 0;
        }, &g, &pairs);
        const int64_t cells = r3g_grid::cells<D>(g.res);
        starts.assign(cells + 1, 0);
        list.resize(pairs);
        std::vector<uint32_t> cursor(cells, 0);
        r3g_grid::host_fill(g, recs.data(), nf, reverse_fill, starts.data(), cursor.data(), list.data());
    }
};
#endif
