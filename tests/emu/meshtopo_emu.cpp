// meshtopo_emu.cpp -- host instantiation of csrc/meshtopo_core.h (test only): the product's check, edge table, classify, label
// rounds, verify, sums and apply as host loops over the same definitions.  `reverse` walks the faces in the opposite order in
// every pass (the order in which the device's atomics land must not matter).  Built with -ffp-contract=off, like the kernels.
#include <stdint.h>

#include <vector>

#include "meshtopo_core.h"

using namespace r3g_mt;

namespace {

struct State {
    std::vector<int32_t> mate, body, label;
    std::vector<uint8_t> flip, hclash, unori;
    std::vector<long long> bodyvol;
    Small sm;
    int rounds;
};

// -> 0, -1 (bad sizes / round cap) or -2 (an index outside [0, nv))
int build(const float* v, int64_t nv, const int32_t* f, int64_t nf, int reverse, State& st) {
    if (nv < 0 || nf <= 0 || nf > kMaxFaces) return -1;
    st.sm = Small{};
    Small& sm = st.sm;
    st.rounds = 0;
    st.label.assign(nf, -1);
    auto face_at = [&](int64_t i) { return reverse ? nf - 1 - i : i; };
    // check
    std::vector<uint32_t> vmark(((size_t)nv + 31) / 32 + 1, 0);
    for (int64_t i = 0; i < nf; ++i)
        for (int k = 0; k < 3; ++k)
            if (f[3 * i + k] < 0 || f[3 * i + k] >= nv) return -2;
    for (int64_t ii = 0; ii < nf; ++ii) {
        const int64_t i = face_at(ii);
        const int32_t* t = f + 3 * i;
        if (!face_usable(t[0], t[1], t[2])) {
            ++sm.skipped;
            continue;
        }
        ++sm.usable;
        st.label[i] = label_make((int32_t)i, 0);
        bool fin = true;
        for (int k = 0; k < 3; ++k) {
            const uint32_t bit = 1u << (t[k] & 31);
            if (!(vmark[t[k] >> 5] & bit)) ++sm.vref;
            vmark[t[k] >> 5] |= bit;
            if (v)
                for (int a = 0; a < 3; ++a) {
                    const float x = v[3 * (int64_t)t[k] + a];
                    if (finite_f(x)) {
                        const uint32_t b = float_bits(x) & 0x7fffffffu;
                        if (b > sm.max_bits) sm.max_bits = b;
                    } else {
                        fin = false;
                    }
                }
        }
        if (!fin) ++sm.nonfinite;
    }
    // edge insert
    const uint64_t slots = table_slots(nf), mask = slots - 1;
    std::vector<unsigned long long> keys(slots, kEdgeEmpty), counts(slots, 0);
    std::vector<int32_t> lo(slots, 0x7f7f7f7f), hi(slots, -1);
    std::vector<uint32_t> hslot(3 * (size_t)nf, 0);
    for (int64_t ii = 0; ii < nf; ++ii) {
        const int64_t i = face_at(ii);
        if (st.label[i] < 0) continue;
        for (int k = 0; k < 3; ++k) {
            const int32_t a = f[3 * i + k], b = f[3 * i + (k + 1) % 3];
            const unsigned long long key = edge_key(a, b);
            uint64_t slot = edge_hash(key) & mask;
            while (keys[slot] != kEdgeEmpty && keys[slot] != key) slot = (slot + 1) & mask;
            keys[slot] = key;
            const int32_t h = (int32_t)(3 * i + k);
            counts[slot] += count_unit(a, b);
            if (h < lo[slot]) lo[slot] = h;
            if (h > hi[slot]) hi[slot] = h;
            hslot[h] = (uint32_t)slot;
        }
    }
    // classify
    st.mate.assign(3 * (size_t)nf, kMateSkipped);
    st.hclash.assign(3 * (size_t)nf, 0);
    for (int64_t h = 0; h < 3 * nf; ++h) {
        if (st.label[h / 3] < 0) continue;
        const uint32_t slot = hslot[h];
        const uint32_t fwd = count_fwd(counts[slot]), bwd = count_bwd(counts[slot]);
        const uint64_t deg = (uint64_t)fwd + bwd;
        const bool first = lo[slot] == (int32_t)h;
        if (deg == 1) {
            st.mate[h] = kMateBoundary;
            sm.boundary += first;
        } else if (deg == 2) {
            st.mate[h] = (int32_t)((int64_t)lo[slot] + hi[slot] - h);
            st.hclash[h] = fwd != 1;
            sm.clash += first && st.hclash[h];
        } else {
            st.mate[h] = kMateNonManifold;
            sm.nonmanifold += first;
        }
        sm.edges += first;
    }
    // label rounds
    int32_t* label = st.label.data();
    auto load = [label](int32_t i) { return label[i]; };
    auto lower = [label](int32_t i, int32_t val) {
        if (val < label[i]) {
            label[i] = val;
            return true;
        }
        return false;
    };
    for (;;) {
        if (st.rounds == kMaxRounds) return -1;
        bool moved = false;
        for (int64_t ii = 0; ii < nf; ++ii) {
            const int64_t i = face_at(ii);
            if (label[i] < 0) continue;
            moved = label_round(load, lower, (int32_t)i, &st.mate[3 * i], &st.hclash[3 * i]) || moved;
        }
        ++st.rounds;
        if (!moved) break;
    }
    // verify
    st.unori.assign(nf, 0);
    for (int64_t i = 0; i < nf; ++i) {
        if (label[i] < 0) continue;
        for (int k = 0; k < 3; ++k) {
            const int32_t m = st.mate[3 * i + k];
            if (m >= 0 && (label_par(label[i]) ^ label_par(label[m / 3])) != (int)st.hclash[3 * i + k]) st.unori[label_root(label[i])] = 1;
        }
    }
    // sums
    st.body.assign(nf, -1);
    st.flip.assign(nf, 0);
    st.bodyvol.assign(nf, 0);
    const int sv = vol_scale(sm.max_bits), sa = area_scale(sm.max_bits);
    for (int64_t ii = 0; ii < nf; ++ii) {
        const int64_t i = face_at(ii);
        if (label[i] < 0) continue;
        const int32_t root = label_root(label[i]);
        const bool u = st.unori[root] != 0;
        st.body[i] = root;
        st.flip[i] = u ? 0 : (uint8_t)label_par(label[i]);
        if (root == (int32_t)i) {
            ++sm.bodies;
            sm.unorientable += u;
        }
        if (!v) continue;
        const float *a = v + 3 * (int64_t)f[3 * i], *b = v + 3 * (int64_t)f[3 * i + 1], *c = v + 3 * (int64_t)f[3 * i + 2];
        bool fin = true;
        for (int k = 0; k < 3; ++k) fin = fin && finite_f(a[k]) && finite_f(b[k]) && finite_f(c[k]);
        if (!fin) continue;
        const long long q0 = quantise(six_vol(a, b, c), sv), q = st.flip[i] ? -q0 : q0;
        sm.six_volume_q += q0;
        if (!u) sm.six_volume_fixed_q += q;
        st.bodyvol[root] += q;
        sm.two_area_q += quantise(two_area(a, b, c), sa);
    }
    return 0;
}

void apply(int32_t* f, int64_t nf, int outward, State& st) {
    const bool all = outward == 2 && st.sm.six_volume_fixed_q < 0;
    st.sm.faces_reversed = st.sm.bodies_reversed = 0;
    for (int64_t i = 0; i < nf; ++i) {
        const int32_t b = st.body[i];
        if (b < 0) continue;
        bool rev = st.flip[i] != 0;
        if (!st.unori[b] && (all || (outward == 1 && st.bodyvol[b] < 0))) {
            rev = !rev;
            st.sm.bodies_reversed += b == (int32_t)i;
        }
        if (rev) {
            const int32_t t = f[3 * i];
            f[3 * i] = f[3 * i + 2];
            f[3 * i + 2] = t;
            ++st.sm.faces_reversed;
        }
    }
}

void write_out(const State& st, bool has_verts, int64_t nf, int32_t* mate, int32_t* body, uint8_t* flip, int64_t* r) {
    const Small& sm = st.sm;
    if (mate) memcpy(mate, st.mate.data(), 12 * (size_t)nf);
    if (body) memcpy(body, st.body.data(), 4 * (size_t)nf);
    if (flip) memcpy(flip, st.flip.data(), (size_t)nf);
    if (!r) return;
    r[0] = (int64_t)sm.usable, r[1] = (int64_t)sm.skipped, r[2] = (int64_t)sm.vref, r[3] = (int64_t)sm.edges;
    r[4] = (int64_t)sm.boundary, r[5] = (int64_t)sm.clash, r[6] = (int64_t)sm.nonmanifold;
    r[7] = (int64_t)sm.bodies, r[8] = (int64_t)sm.unorientable;
    r[9] = r[2] - r[3] + r[0];
    r[10] = (int64_t)sm.nonfinite;
    r[11] = sm.six_volume_q, r[12] = vol_scale(sm.max_bits);
    r[13] = sm.two_area_q, r[14] = area_scale(sm.max_bits);
    r[15] = has_verts ? 1 : 0;
}

}  // namespace

extern "C" {

int r3g_emu_meshtopo_build(const float* v, int64_t nv, const int32_t* f, int64_t nf, int reverse, int32_t* mate, int32_t* body,
                           uint8_t* flip, int64_t* report, int* rounds_out) {
    State st;
    const int rc = build(v, nv, f, nf, reverse, st);
    if (rc) return rc;
    write_out(st, v != nullptr, nf, mate, body, flip, report);
    if (rounds_out) *rounds_out = st.rounds;
    return 0;
}

// build, apply, and (as the product does) a second build when anything was reversed; f is rewritten in place
int r3g_emu_meshtopo_orient(const float* v, int64_t nv, int32_t* f, int64_t nf, int outward, int reverse, int64_t* faces_reversed,
                            int64_t* bodies_reversed, int32_t* mate, int32_t* body, uint8_t* flip, int64_t* report) {
    if (outward < 0 || outward > 2 || (outward && !v)) return -1;
    State st;
    int rc = build(v, nv, f, nf, reverse, st);
    if (rc) return rc;
    apply(f, nf, outward, st);
    const unsigned long long nfr = st.sm.faces_reversed, nbr = st.sm.bodies_reversed;
    if (nfr && (rc = build(v, nv, f, nf, reverse, st))) return rc;
    write_out(st, v != nullptr, nf, mate, body, flip, report);
    if (faces_reversed) *faces_reversed = (int64_t)nfr;
    if (bodies_reversed) *bodies_reversed = (int64_t)nbr;
    return 0;
}

}  // extern "C"
