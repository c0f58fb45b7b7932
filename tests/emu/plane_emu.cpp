// plane_emu.cpp -- host instantiation of csrc/plane_core.h (test only): (a) every hypothesis against every point in two plain
// loops, (b) the count pass in the product's block order (blocks of kCountPoints rows, tiles of kHypTile hypotheses, four
// groups of 64 slots whose ballots are counted and met once per tile, the table split over `splits` row-blocks).  The moments
// follow the header's one summation order in both.  Built with -ffp-contract=off, like the kernels.  (a) also takes a `mutant`
// number: deliberate departures from the definition, each of which the named clouds must expose (tests/test_plane_cpu.py).
// With -DPLANE_EMU_MAIN it is a stand-alone program (for a sanitizer build) that runs (a) and (b) on a lattice whose
// distances tie with the threshold and compares them.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "plane_core.h"

using namespace r3g_pl;

namespace {

enum Mutant { kNone = 0, kLessEqual = 1, kFloat32 = 2, kLastOnTie = 3, kSkipValidity = 4 };

bool test(const Hyp& h, const float* q, double threshold, int mutant) {
    if (!usable(q[0], q[1], q[2])) return false;
    if (mutant == kFloat32) {
        const float d = fabsf((((q[0] - (float)h.p0[0]) * (float)h.n[0]) + (q[1] - (float)h.p0[1]) * (float)h.n[1]) +
                              (q[2] - (float)h.p0[2]) * (float)h.n[2]);
        return (double)d < threshold;
    }
    const double d = distance(h.p0, h.n, (double)q[0], (double)q[1], (double)q[2]);
    return mutant == kLessEqual ? d <= threshold : d < threshold;
}

// the moments of the rows with mask[i] != 0 (all rows when mask is null), in the header's order
Moments moments_of(const float* pts, int64_t n, const uint8_t* mask) {
    Moments m;
    memset(&m, 0, sizeof m);
    const int64_t nb = mom_chunks(n);
    for (int64_t i = 0; i < n; ++i)
        if (!mask || mask[i]) {
            if (usable(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2])) ++m.n;
            else ++m.skipped;
        }
    for (int pass = 0; pass < 2; ++pass) {
        const int K = pass == 0 ? 3 : 6;
        std::vector<double> partial((size_t)nb * 6, 0.0);
        for (int64_t b = 0; b < nb; ++b)
            for (int k = 0; k < K; ++k) {
                double slot[kBlock];
                for (int t = 0; t < kBlock; ++t) {
                    double acc = 0.0;
                    for (int r = 0; r < kMomChunk / kBlock; ++r) {
                        const int64_t i = b * kMomChunk + r * kBlock + t;
                        double term = 0.0;
                        if (i < n && (!mask || mask[i]) && usable(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2])) {
                            if (pass == 0) {
                                term = (double)pts[3 * i + k];
                            } else {
                                const double d[3] = {(double)pts[3 * i] - m.c[0], (double)pts[3 * i + 1] - m.c[1], (double)pts[3 * i + 2] - m.c[2]};
                                static const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
                                term = d[ia[k]] * d[ib[k]];
                            }
                        }
                        acc = acc + term;
                    }
                    slot[t] = acc;
                }
                partial[(size_t)b * 6 + k] = tree_sum256(slot);
            }
        for (int k = 0; k < K; ++k) {
            double slot[kBlock];
            for (int t = 0; t < kBlock; ++t) {
                double acc = 0.0;
                for (int64_t b = t; b < nb; b += kBlock) acc = acc + partial[(size_t)b * 6 + k];
                slot[t] = acc;
            }
            const double v = tree_sum256(slot);
            if (pass == 0) {
                m.sum[k] = v;
                m.c[k] = m.n ? v / (double)m.n : 0.0;
            } else {
                m.s[k] = v;
            }
        }
    }
    return m;
}

void count_brute(const float* pts, int64_t n, const std::vector<Hyp>& hyp, double threshold, int mutant, uint32_t* count) {
    for (size_t h = 0; h < hyp.size(); ++h) {
        uint32_t c = 0;
        if (hyp[h].valid)
            for (int64_t i = 0; i < n; ++i) c += test(hyp[h], pts + 3 * i, threshold, mutant);
        count[h] = c;
    }
}

// the count kernel as host loops: grid (row blocks, table splits), four groups a block, ballots as 64-bit words
void count_blocks(const float* pts, int64_t n, const std::vector<Hyp>& hyp, double threshold, int splits, uint32_t* count) {
    const int n_hyp = (int)hyp.size();
    for (int h = 0; h < n_hyp; ++h) count[h] = 0;
    const int64_t nbx = (n + kCountPoints - 1) / kCountPoints;
    const int tiles = (n_hyp + kHypTile - 1) / kHypTile;
    int ny = splits < 1 ? 1 : splits;
    if (ny > tiles) ny = tiles;
    if (ny < 1) ny = 1;
    const int per_y = ((tiles + ny - 1) / ny) * kHypTile;
    for (int64_t bx = 0; bx < nbx; ++bx)
        for (int by = 0; by < ny; ++by) {
            const int h_lo = by * per_y, h_hi = n_hyp < h_lo + per_y ? n_hyp : h_lo + per_y;
            for (int t0 = h_lo; t0 < h_hi; t0 += kHypTile) {
                const int m = h_hi - t0 < kHypTile ? h_hi - t0 : kHypTile;
                uint32_t sh[4][kHypTile];
                for (int wave = 0; wave < 4; ++wave)
                    for (int j = 0; j < kHypTile; ++j) {
                        uint32_t c = 0;
                        if (j < m && hyp[t0 + j].valid)
                            for (int k = 0; k < kPerLane; ++k) {
                                uint64_t ballot = 0;
                                for (int lane = 0; lane < 64; ++lane) {
                                    const int64_t i = bx * kCountPoints + (int64_t)k * kBlock + wave * 64 + lane;
                                    if (i < n && test(hyp[t0 + j], pts + 3 * i, threshold, kNone)) ballot |= 1ull << lane;
                                }
                                c += (uint32_t)__builtin_popcountll(ballot);
                            }
                        sh[wave][j] = c;
                    }
                for (int j = 0; j < m; ++j) count[t0 + j] += sh[0][j] + sh[1][j] + sh[2][j] + sh[3][j];
            }
        }
}

}  // namespace

extern "C" {

// mode 0: (a), mode 1: (b) with `splits` table splits.  count uint32 [n_hyp], mask uint8 [n] (both may be null), report int64 [8],
// plane double [16] as r3g_plane_ransac has them.
int r3g_emu_plane_ransac(const float* pts, int64_t n, const int32_t* triples, int n_hyp, double threshold, int mode, int splits, int mutant,
                         uint32_t* count_out, uint8_t* mask_out, int64_t* report, double* plane) {
    if (!(threshold > 0.0) || !(threshold - threshold == 0.0) || n_hyp < 0 || n_hyp > kMaxHyp || n < 0 || n >= (1ll << 31)) return -1;
    std::vector<Hyp> hyp((size_t)n_hyp);
    for (int h = 0; h < n_hyp; ++h) hyp[h] = make_hyp(pts, n, triples[3 * h], triples[3 * h + 1], triples[3 * h + 2], mutant == kSkipValidity);
    std::vector<uint32_t> count((size_t)n_hyp);
    if (mode == 0) count_brute(pts, n, hyp, threshold, mutant, count.data());
    else count_blocks(pts, n, hyp, threshold, splits, count.data());
    int64_t usable_n = 0, valid = 0;
    for (int64_t i = 0; i < n; ++i) usable_n += usable(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    unsigned long long key = 0;
    for (int h = 0; h < n_hyp; ++h)
        if (hyp[h].valid) {
            ++valid;
            const unsigned long long k = winner_key(count[h], (uint32_t)h);
            if (mutant == kLastOnTie ? (!key || key_count(k) >= key_count(key)) : k > key) key = k;
        }
    const int32_t best = key_h(key);
    std::vector<uint8_t> mask((size_t)n, 0);
    if (best >= 0)
        for (int64_t i = 0; i < n; ++i) mask[i] = test(hyp[best], pts + 3 * i, threshold, mutant) ? 1 : 0;
    const Moments m = moments_of(pts, n, mask.data());
    int few = 0;
    double val[3], normal[3];
    plane_of(m, val, normal, &few);
    const int64_t rep[kReport] = {usable_n, valid, best, (int64_t)key_count(key), few, 0, 0, 0};
    memcpy(report, rep, sizeof rep);
    Hyp none;
    memset(&none, 0, sizeof none);
    const Hyp& w = best >= 0 ? hyp[best] : none;
    for (int a = 0; a < 3; ++a) {
        plane[a] = w.p0[a], plane[3 + a] = w.n[a];
        plane[6 + a] = m.c[a], plane[9 + a] = normal[a], plane[12 + a] = val[a];
    }
    plane[15] = 0.0;
    if (count_out && n_hyp) memcpy(count_out, count.data(), 4 * (size_t)n_hyp);
    if (mask_out && n) memcpy(mask_out, mask.data(), (size_t)n);
    return 0;
}

// out double [16], report int64 [4] as r3g_plane_moments has them
int r3g_emu_plane_moments(const float* pts, int64_t n, const uint8_t* mask, double* out, int64_t* report) {
    if (n < 0 || n >= (1ll << 31)) return -1;
    const Moments m = moments_of(pts, n, mask);
    int few = 0;
    double val[3], normal[3];
    plane_of(m, val, normal, &few);
    out[0] = (double)m.n;
    for (int a = 0; a < 3; ++a) out[1 + a] = m.c[a], out[10 + a] = val[a], out[13 + a] = normal[a];
    for (int a = 0; a < 6; ++a) out[4 + a] = m.s[a];
    const int64_t rep[kMomReport] = {(int64_t)m.n, (int64_t)m.skipped, few, 0};
    memcpy(report, rep, sizeof rep);
    return 0;
}

int r3g_emu_plane_count_points(void) { return kCountPoints; }
}

#ifdef PLANE_EMU_MAIN
#include <stdio.h>

// a 41 x 3 x 41 lattice of spacing 0.25 (layers y = 0, 0.25, 0.5) at threshold 0.25: the neighbouring layers tie with it; a
// non-finite row, a far point, and triples that are axis-aligned, tilted, collinear, repeated and out of range
int main() {
    std::vector<float> pts;
    for (int y = 0; y < 3; ++y)
        for (int z = 0; z < 41; ++z)
            for (int x = 0; x < 41; ++x) pts.push_back(0.25f * x), pts.push_back(0.25f * y), pts.push_back(0.25f * z);
    const float extra[6] = {NAN, 0.5f, 0.5f, 40.0f, -3.0f, 7.0f};
    pts.insert(pts.begin() + 30, extra, extra + 3);
    pts.insert(pts.end(), extra + 3, extra + 6);
    const int64_t n = (int64_t)pts.size() / 3;
    std::vector<int32_t> tri;
    for (int h = 0; h < 150; ++h) {
        const int32_t a = (h * 37) % (int32_t)n, b = (h * 101 + 7) % (int32_t)n, c = (h * 211 + 3) % (int32_t)n;
        tri.push_back(a), tri.push_back(b), tri.push_back(c);
    }
    const int32_t odd[12] = {0, 1, 2, 5, 5, 9, -1, 4, 8, 3, (int32_t)n, 6};
    tri.insert(tri.end(), odd, odd + 12);
    const int n_hyp = (int)tri.size() / 3;
    int bad = 0;
    for (int64_t m : {(int64_t)0, (int64_t)2, (int64_t)1023, (int64_t)1025, n}) {
        std::vector<uint32_t> ca(n_hyp), cb(n_hyp);
        std::vector<uint8_t> ma((size_t)m + 1), mb((size_t)m + 1);
        int64_t ra[kReport], rb[kReport];
        double pa[kPlane], pb[kPlane];
        if (r3g_emu_plane_ransac(pts.data(), m, tri.data(), n_hyp, 0.25, 0, 1, 0, ca.data(), ma.data(), ra, pa)) return 2;
        for (int splits : {1, 2, 3, 64}) {
            if (r3g_emu_plane_ransac(pts.data(), m, tri.data(), n_hyp, 0.25, 1, splits, 0, cb.data(), mb.data(), rb, pb)) return 2;
            bad += memcmp(ca.data(), cb.data(), 4 * (size_t)n_hyp) != 0 || memcmp(ma.data(), mb.data(), (size_t)m) != 0;
            bad += memcmp(ra, rb, sizeof ra) != 0 || memcmp(pa, pb, sizeof pa) != 0;
        }
        double out[kMomOut];
        int64_t rep[kMomReport];
        if (r3g_emu_plane_moments(pts.data(), m, ma.data(), out, rep)) return 2;
        bad += memcmp(out + 1, pa + 6, 24) != 0 || memcmp(out + 13, pa + 9, 24) != 0 || rep[0] != (ra[2] >= 0 ? ra[3] : 0);
    }
    printf("plane_emu lattice: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
