// plane_core.h -- the definition of the plane fit: hypotheses from point triples, the float64 inlier
// test, the winner, the moments of a masked set in one fixed summation order, and the eigenpairs of the 3 x 3 scatter.
// Plain C++; compiled for the device by plane_kernels.hip, for the host by r3g_api.cpp (the eigen solver) and by the
// test twin (tests/emu/plane_emu.cpp), all with contraction off, so the three agree bit for bit.
//
// Summation order of the moments (it depends on n alone, never on a grid size or a schedule):
//   * the rows are cut into chunks of kMomChunk = 1024 consecutive rows; chunk b holds rows [1024 b, 1024 b + 1024);
//   * inside a chunk, slot t (0..255) adds the terms of rows 1024 b + t, + 256, + 512, + 768 in that order to +0.0; a row
//     outside the set, or past n, adds +0.0;
//   * the 256 slots are four groups of 64 (slots 64 w .. 64 w + 63); a group is summed by the butterfly
//         for d in 32, 16, 8, 4, 2, 1:  v[l] = v[l] + v[l ^ d]      (tree_sum64 below; every l ends with the same value)
//     and the four group sums are added as ((g0 + g1) + g2) + g3: the chunk's partial;
//   * the partials are summed the same way by one more level: slot t adds the partials t, t + 256, t + 512, ... in index
//     order to +0.0, then the butterfly and the four groups as above.
// The first pass sums (x, y, z) widened to float64; centroid = sum / n, one division each.  The second pass sums the six
// products dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz of d = p - centroid (one rounding per operation).
#ifndef R3G_PLANE_CORE_H
#define R3G_PLANE_CORE_H
#include <math.h>
#include <stdint.h>

#ifndef R3G_PL_HD
#define R3G_PL_HD static inline
#endif

namespace r3g_pl {

constexpr int kMaxHyp = 65536;
constexpr double kMinLen = 1e-6;       // a triple whose cross product is shorter spans no plane
constexpr int kBlock = 256;            // threads of every block: four waves
constexpr int kPerLane = 4;            // points a lane of the count pass keeps in registers
constexpr int kCountPoints = kBlock * kPerLane;      // points per block of the count pass
constexpr int kHypTile = 64;           // hypotheses between two exchanges through LDS: lane j keeps the count of the tile's j-th
constexpr int kMomChunk = 1024;        // rows per chunk of the moments (see above)
constexpr int kJacobiSweeps = 12;      // fixed: the twin runs the same rotations
constexpr int kReport = 8, kPlane = 16, kMomOut = 16, kMomReport = 4, kPasses = 4;

struct Hyp {
    double p0[3];
    double n[3];
    int32_t valid;
    int32_t pad;
};

// the sums of a set and what follows from them without an eigen solve
struct Moments {
    unsigned long long n;          // rows in the set: usable and selected
    unsigned long long skipped;    // selected rows with a non-finite coordinate
    double sum[3];
    double c[3];                   // sum / n; (0, 0, 0) for an empty set
    double s[6];                   // xx, xy, xz, yy, yz, zz about c
};

R3G_PL_HD bool finite_f(float v) { return v - v == 0.0f; }
R3G_PL_HD bool usable(float x, float y, float z) { return finite_f(x) && finite_f(y) && finite_f(z); }

// hypothesis (i0, i1, i2) over points float32 [n][3]
R3G_PL_HD Hyp make_hyp(const float* pts, int64_t n, int32_t i0, int32_t i1, int32_t i2, bool skip_validity = false) {
    Hyp h;
    h.p0[0] = h.p0[1] = h.p0[2] = 0.0;
    h.n[0] = h.n[1] = h.n[2] = 0.0;
    h.valid = 0;
    h.pad = 0;
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n || i1 >= n || i2 >= n) return h;
    const float* a = pts + 3 * (int64_t)i0;
    const float* b = pts + 3 * (int64_t)i1;
    const float* c = pts + 3 * (int64_t)i2;
    if (!usable(a[0], a[1], a[2]) || !usable(b[0], b[1], b[2]) || !usable(c[0], c[1], c[2])) return h;
    const double ax = (double)a[0], ay = (double)a[1], az = (double)a[2];
    const double v1x = (double)b[0] - ax, v1y = (double)b[1] - ay, v1z = (double)b[2] - az;
    const double v2x = (double)c[0] - ax, v2y = (double)c[1] - ay, v2z = (double)c[2] - az;
    const double cx = v1y * v2z - v1z * v2y;
    const double cy = v1z * v2x - v1x * v2z;
    const double cz = v1x * v2y - v1y * v2x;
    const double len = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!skip_validity && !(len >= kMinLen)) return h;
    h.p0[0] = ax, h.p0[1] = ay, h.p0[2] = az;
    h.n[0] = cx / len, h.n[1] = cy / len, h.n[2] = cz / len;
    h.valid = 1;
    return h;
}

// d(h, q) of a usable q, its coordinates already widened
R3G_PL_HD double distance(const double p0[3], const double nr[3], double qx, double qy, double qz) {
    return fabs(((qx - p0[0]) * nr[0] + (qy - p0[1]) * nr[1]) + (qz - p0[2]) * nr[2]);
}

R3G_PL_HD bool inlier(const double p0[3], const double nr[3], double qx, double qy, double qz, double threshold) {
    return distance(p0, nr, qx, qy, qz) < threshold;
}

// winner key: larger count first, then the lower h; 0 = no valid hypothesis seen
R3G_PL_HD unsigned long long winner_key(uint32_t count, uint32_t h) { return ((unsigned long long)count << 32) | (0xffffffffu - h); }
R3G_PL_HD int32_t key_h(unsigned long long key) { return key ? (int32_t)(0xffffffffu - (uint32_t)(key & 0xffffffffu)) : -1; }
R3G_PL_HD uint32_t key_count(unsigned long long key) { return (uint32_t)(key >> 32); }

R3G_PL_HD int64_t mom_chunks(int64_t n) { return (n + kMomChunk - 1) / kMomChunk; }

// the butterfly over 64 slots, on the host: v[0] afterwards (the device does it with lane exchanges)
inline double tree_sum64(double* v) {
    double w[64];
    for (int d = 32; d >= 1; d >>= 1) {
        for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ d];
        for (int l = 0; l < 64; ++l) v[l] = w[l];
    }
    return v[0];
}

// 256 slots -> one sum: four butterflies, then ((g0 + g1) + g2) + g3
inline double tree_sum256(double* v) {
    const double g0 = tree_sum64(v), g1 = tree_sum64(v + 64), g2 = tree_sum64(v + 128), g3 = tree_sum64(v + 192);
    return ((g0 + g1) + g2) + g3;
}

// Eigenpairs of the symmetric 3 x 3 matrix s = (xx, xy, xz, yy, yz, zz) by cyclic Jacobi rotations, kJacobiSweeps sweeps
// over (0,1), (0,2), (1,2); a pair whose off-diagonal entry is exactly 0 is passed over.  val ascending (ties keep the
// lower column first), vec[k] the unit eigenvector of val[k].
inline void eigen3(const double s[6], double val[3], double vec[3][3]) {
    double a[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    double e[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - sn * akq;
                    a[k][q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - sn * aqk;
                    a[q][k] = sn * apk + c * aqk;
                }
                a[p][q] = a[q][p] = 0.0;
                for (int k = 0; k < 3; ++k) {
                    const double ekp = e[k][p], ekq = e[k][q];
                    e[k][p] = c * ekp - sn * ekq;
                    e[k][q] = sn * ekp + c * ekq;
                }
            }
    int order[3] = {0, 1, 2};
    for (int i = 1; i < 3; ++i)
        for (int j = i; j > 0 && a[order[j]][order[j]] < a[order[j - 1]][order[j - 1]]; --j) {
            const int tmp = order[j];
            order[j] = order[j - 1];
            order[j - 1] = tmp;
        }
    for (int k = 0; k < 3; ++k) {
        val[k] = a[order[k]][order[k]];
        double x = e[0][order[k]], y = e[1][order[k]], z = e[2][order[k]];
        const double len = sqrt((x * x + y * y) + z * z);
        vec[k][0] = x / len, vec[k][1] = y / len, vec[k][2] = z / len;
    }
}

// From the moments of a set to its plane: eigenvalues ascending and the normal, the first eigenvector turned "up": negated
// where n_y < 0, kept where n_y >= 0 (a zero n_y of either sign included).  Fewer than 3 rows: (0, 1, 0), zero eigenvalues,
// *few = 1.
inline void plane_of(const Moments& m, double val[3], double normal[3], int* few) {
    if (m.n < 3) {
        val[0] = val[1] = val[2] = 0.0;
        normal[0] = 0.0, normal[1] = 1.0, normal[2] = 0.0;
        *few = 1;
        return;
    }
    double vec[3][3];
    eigen3(m.s, val, vec);
    const double sign = vec[0][1] < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; ++k) normal[k] = sign * vec[0][k];
    *few = 0;
}

}  // namespace r3g_pl
#endif
