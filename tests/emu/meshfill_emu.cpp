// meshfill_emu.cpp -- host instantiation of csrc/meshfill_core.h (test only; link with meshtopo_emu.cpp, whose mate table it
// starts from, as the product's plan starts from r3g_meshtopo_build): compaction, vertex pass, succ, the two pointer doublings,
// allocation, loop vertices, centroids and the emitted faces as host loops over the same definitions.  `reverse` walks the slots
// in the opposite order in every pass (the order in which the device's atomics and lanes land must not matter); the doublings
// are double-buffered exactly as on the device.  Built with -ffp-contract=off, like the kernels.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "meshfill_core.h"

extern "C" int r3g_emu_meshtopo_build(const float* v, int64_t nv, const int32_t* f, int64_t nf, int reverse, int32_t* mate, int32_t* body,
                                      uint8_t* flip, int64_t* report, int* rounds_out);

using namespace r3g_mf;

namespace {

struct State {
    std::vector<int32_t> bh, succ, lead, d, lverts, new_faces, status;
    std::vector<uint32_t> s_ord, s_start, s_fill, s_face;
    std::vector<int64_t> loop_start;
    std::vector<float> cent;
    int64_t report[16];
};

// -> 0, -1 (bad arguments) or -2 (an index outside [0, nv))
int plan(const float* v, int64_t nv, const int32_t* f, int64_t nf, int64_t max_loop, int mode, int reverse, State& st) {
    if (max_loop < kMinLoop || (mode != kModeFan && mode != kModeCentroid) || (mode == kModeCentroid && !v)) return -1;
    std::vector<int32_t> mate(3 * (size_t)(nf > 0 ? nf : 0));
    int64_t topo[16];
    const int rc = r3g_emu_meshtopo_build(v, nv, f, nf, reverse, mate.data(), nullptr, nullptr, topo, nullptr);
    if (rc) return rc;
    // compact
    st.bh.clear();
    for (int64_t h = 0; h < 3 * nf; ++h)
        if (mate[h] == -1) st.bh.push_back((int32_t)h);
    const int64_t B = (int64_t)st.bh.size();
    if (B != topo[4]) return -1;
    auto slot_at = [&](int64_t i) { return reverse ? B - 1 - i : i; };
    // vertex pass, link, succ
    std::vector<unsigned long long> deg((size_t)nv, 0);
    std::vector<int32_t> outc((size_t)nv, -1);
    for (int64_t i = 0; i < B; ++i) {
        const int64_t c = slot_at(i);
        deg[he_tail(f, st.bh[c])] += kDegOut;
        deg[he_head(f, st.bh[c])] += kDegIn;
    }
    for (int64_t i = 0; i < B; ++i) {
        const int64_t c = slot_at(i);
        const int32_t t = he_tail(f, st.bh[c]);
        if (deg_out(deg[t]) == 1u) outc[t] = (int32_t)c;
    }
    st.succ.assign(B, -1);
    std::vector<int32_t> x[2], y[2];
    for (int k = 0; k < 2; ++k) x[k].assign(B, 0), y[k].assign(B, 0);
    for (int64_t c = 0; c < B; ++c) {
        const int32_t hd = he_head(f, st.bh[c]);
        st.succ[c] = vertex_simple(deg[hd]) ? outc[hd] : -1;
        x[0][c] = (int32_t)c, y[0][c] = st.succ[c];
    }
    // minimum / open
    const int rounds = rounds_for(B);
    int cur = 0;
    for (int r = 0; r < rounds; ++r, cur ^= 1) {
        const int32_t *mi = x[cur].data(), *pi = y[cur].data();
        for (int64_t i = 0; i < B; ++i) {
            const int64_t c = slot_at(i);
            min_step([mi](int32_t j) { return mi[j]; }, [pi](int32_t j) { return pi[j]; }, mi[c], pi[c], &x[cur ^ 1][c], &y[cur ^ 1][c]);
        }
    }
    // rank
    st.lead.assign(B, -1);
    for (int64_t c = 0; c < B; ++c) {
        const bool open = y[cur][c] < 0;
        const int32_t l = open ? -1 : x[cur][c];
        const bool terminal = open || l == (int32_t)c;
        st.lead[c] = l;
        x[cur ^ 1][c] = terminal ? (int32_t)c : st.succ[c];
        y[cur ^ 1][c] = terminal ? 0 : 1;
    }
    cur ^= 1;
    for (int r = 0; r < rounds; ++r, cur ^= 1) {
        const int32_t *qi = x[cur].data(), *di = y[cur].data();
        for (int64_t i = 0; i < B; ++i) {
            const int64_t c = slot_at(i);
            rank_step([qi](int32_t j) { return qi[j]; }, [di](int32_t j) { return di[j]; }, qi[c], di[c], &x[cur ^ 1][c], &y[cur ^ 1][c]);
        }
    }
    st.d = y[cur];
    // allocate: four exclusive scans over the leaders
    Small sm{};
    st.s_ord.assign(B, 0), st.s_start.assign(B, 0), st.s_fill.assign(B, 0), st.s_face.assign(B, 0);
    for (int64_t c = 0; c < B; ++c) {
        st.s_ord[c] = (uint32_t)sm.loops, st.s_start[c] = (uint32_t)sm.loop_edges;
        st.s_fill[c] = (uint32_t)sm.filled, st.s_face[c] = (uint32_t)sm.faces_added;
        if (st.lead[c] != (int32_t)c) continue;
        const int32_t len = loop_length(st.d[st.succ[c]]);
        ++sm.loops;
        sm.loop_edges += (unsigned long long)len;
        if ((uint32_t)len > sm.longest) sm.longest = (uint32_t)len;
        if (loop_kept(len, max_loop)) {
            ++sm.filled;
            sm.faces_added += loop_faces(len, mode);
        }
    }
    const int64_t verts_added = mode == kModeCentroid ? (int64_t)sm.filled : 0;
    if (nv + verts_added >= (1ll << 31)) return -1;
    // loop vertices, the loop table, centroids, faces
    st.lverts.assign(sm.loop_edges, -1);
    st.loop_start.assign(sm.loops + 1, 0);
    st.status.assign(sm.loops, -1);
    st.loop_start[sm.loops] = (int64_t)sm.loop_edges;
    st.cent.assign(3 * (size_t)verts_added, 0.0f);
    st.new_faces.assign(3 * (size_t)sm.faces_added, -1);
    for (int64_t i = 0; i < B; ++i) {
        const int64_t c = slot_at(i);
        const int32_t l = st.lead[c];
        if (l < 0) continue;
        const int32_t len = loop_length(st.d[st.succ[l]]);
        st.lverts[st.s_start[l] + loop_rank(len, st.d[c])] = he_tail(f, st.bh[c]);
    }
    for (int64_t i = 0; i < B; ++i) {
        const int64_t c = slot_at(i);
        const int32_t l = st.lead[c];
        if (l < 0) continue;
        const int32_t len = loop_length(st.d[st.succ[l]]);
        const bool keep = loop_kept(len, max_loop);
        const int32_t* a = st.lverts.data() + st.s_start[l];
        if (l == (int32_t)c) {
            st.loop_start[st.s_ord[c]] = (int64_t)st.s_start[c];
            st.status[st.s_ord[c]] = keep ? 0 : 1;
            if (keep && mode == kModeCentroid)
                loop_centroid([v, a](int32_t j, int k) { return v[3 * (int64_t)a[j] + k]; }, len, &st.cent[3 * (size_t)st.s_fill[c]]);
        }
        if (!keep) continue;
        int32_t face[3];
        const int32_t at = loop_face([a](int32_t j) { return a[j]; }, len, loop_rank(len, st.d[c]), mode, (int32_t)(nv + st.s_fill[l]), face);
        if (at >= 0) memcpy(&st.new_faces[3 * ((size_t)st.s_face[l] + at)], face, sizeof face);
    }
    int64_t* r = st.report;
    memset(r, 0, sizeof st.report);
    r[kRepBoundary] = B, r[kRepLoops] = (int64_t)sm.loops, r[kRepTangled] = B - (int64_t)sm.loop_edges, r[kRepFilled] = (int64_t)sm.filled;
    r[kRepOversize] = (int64_t)(sm.loops - sm.filled), r[kRepLongest] = sm.longest, r[kRepLoopEdges] = (int64_t)sm.loop_edges;
    r[kRepFacesAdded] = (int64_t)sm.faces_added, r[kRepVertsAdded] = verts_added, r[kRepRounds] = rounds;
    r[kRepMaxLoop] = max_loop, r[kRepMode] = mode, r[kRepFaces] = nf, r[kRepVerts] = nv;
    return 0;
}

State g_state;
bool g_planned = false;

}  // namespace

extern "C" {

// plan; the state stays until the next plan (a failed plan leaves none)
int r3g_emu_meshfill_plan(const float* v, int64_t nv, const int32_t* f, int64_t nf, int64_t max_loop, int mode, int reverse,
                          int64_t* report) {
    g_planned = false;
    const int rc = plan(v, nv, f, nf, max_loop, mode, reverse, g_state);
    if (rc) return rc;
    g_planned = true;
    if (report) memcpy(report, g_state.report, sizeof g_state.report);
    return 0;
}

// new_faces int32 [faces_added][3], new_verts float [verts_added][3] (either may be null); -3 without a plan
int r3g_emu_meshfill_emit(int32_t* new_faces, float* new_verts) {
    if (!g_planned) return -3;
    if (new_faces && !g_state.new_faces.empty()) memcpy(new_faces, g_state.new_faces.data(), 4 * g_state.new_faces.size());
    if (new_verts && !g_state.cent.empty()) memcpy(new_verts, g_state.cent.data(), 4 * g_state.cent.size());
    return 0;
}

// loop_start int64 [loops + 1], loop_verts int32 [loop_edges], status int32 [loops]; -3 without a plan
int r3g_emu_meshfill_loops(int64_t* loop_start, int32_t* loop_verts, int32_t* status) {
    if (!g_planned) return -3;
    memcpy(loop_start, g_state.loop_start.data(), 8 * g_state.loop_start.size());
    if (!g_state.lverts.empty()) memcpy(loop_verts, g_state.lverts.data(), 4 * g_state.lverts.size());
    if (!g_state.status.empty()) memcpy(status, g_state.status.data(), 4 * g_state.status.size());
    return 0;
}

}  // extern "C"
