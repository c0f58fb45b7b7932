// meshfit_core.h -- host solver of the mesh registration: from the sums of one fit step
// (meshdist_core.h, fit_point) to the update of the similarity.  Plain C++, float64, no device code; shared by
// r3g_api.cpp and the test twin (tests/emu/meshfit_emu.cpp).  Coordinates in the sums are relative to a centre c
// (the grid box centre); solve_* return the update in world coordinates.
#ifndef R3G_MESHFIT_CORE_H
#define R3G_MESHFIT_CORE_H
#include <math.h>

#include "meshdist_core.h"

namespace r3g_mf {

using r3g_md::Sim;

inline Sim identity() {
    Sim x;
    x.s = 1.0;
    for (int i = 0; i < 9; ++i) x.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
    x.t[0] = x.t[1] = x.t[2] = 0.0;
    return x;
}

// a after b: p -> sa Ra (sb Rb p + tb) + ta
inline Sim compose(const Sim& a, const Sim& b) {
    Sim o;
    o.s = a.s * b.s;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o.r[3 * i + j] = a.r[3 * i] * b.r[j] + a.r[3 * i + 1] * b.r[3 + j] + a.r[3 * i + 2] * b.r[6 + j];
    for (int i = 0; i < 3; ++i) o.t[i] = a.s * (a.r[3 * i] * b.t[0] + a.r[3 * i + 1] * b.t[1] + a.r[3 * i + 2] * b.t[2]) + a.t[i];
    return o;
}

// a similarity given about the centre c (q - c = s R (p - c) + t) in world coordinates
inline Sim about_centre(const Sim& x, const double c[3]) {
    Sim o = x;
    for (int i = 0; i < 3; ++i) o.t[i] = x.t[i] + c[i] - x.s * (x.r[3 * i] * c[0] + x.r[3 * i + 1] * c[1] + x.r[3 * i + 2] * c[2]);
    return o;
}

// row-major 4 x 4: [s R | t; 0 0 0 1]
inline void to_matrix(const Sim& x, double m[16]) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[4 * i + j] = x.s * x.r[3 * i + j];
        m[4 * i + 3] = x.t[i];
    }
    m[12] = m[13] = m[14] = 0.0;
    m[15] = 1.0;
}

// false when m is not a similarity: last row not (0, 0, 0, 1), determinant <= 0, or M^T M further than 1e-6 from s^2 I
inline bool from_matrix(const double m[16], Sim* out) {
    for (int i = 0; i < 16; ++i)
        if (!(m[i] - m[i] == 0.0)) return false;
    if (m[12] != 0.0 || m[13] != 0.0 || m[14] != 0.0 || m[15] != 1.0) return false;
    const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
    if (!(det > 0.0)) return false;
    const double s = cbrt(det);
    Sim x;
    x.s = s;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) x.r[3 * i + j] = m[4 * i + j] / s;
        x.t[i] = m[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = x.r[i] * x.r[j] + x.r[3 + i] * x.r[3 + j] + x.r[6 + i] * x.r[6 + j];
            if (fabs(g - (i == j ? 1.0 : 0.0)) > 1e-6) return false;
        }
    *out = x;
    return true;
}

// eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix by cyclic Jacobi rotations
inline void max_eigenvector4(double a[4][4], double v[4]) {
    double e[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) (i == j ? diag : off) += a[i][j] * a[i][j];
        if (!(off > 1e-32 * diag)) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (a[p][q] == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 4; ++k) {
                    const double ekp = e[k][p], ekq = e[k][q];
                    e[k][p] = c * ekp - s * ekq;
                    e[k][q] = s * ekp + c * ekq;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < 4; ++i)
        if (a[i][i] > a[best][best]) best = i;
    for (int k = 0; k < 4; ++k) v[k] = e[k][best];
}

// Closed form of the point method (Horn 1987, unit quaternions; scale as in Umeyama 1991): the similarity that takes the
// moved points p onto their closest points q in the least-squares sense, from the kFitPointTerms sums about c.  The rotation
// is that of the largest eigenvector of Horn's 4 x 4 matrix: a unit quaternion, so det R = +1 whatever the data (mirrored,
// coplanar or collinear correspondences get the best proper rotation; where the data leave it open, one of them).
// scale = sum (R p~) . q~ / sum |p~|^2 (p~, q~: about the weighted means).  false: W <= 0 or a non-finite sum.
inline bool solve_point(const double* sums, bool with_scale, const double c[3], Sim* out) {
    const double W = sums[0];
    for (int i = 0; i < r3g_md::kFitPointTerms; ++i)
        if (!(sums[i] - sums[i] == 0.0)) return false;
    if (!(W > 0.0)) return false;
    double mp[3], mq[3], H[3][3];
    for (int a = 0; a < 3; ++a) mp[a] = sums[1 + a] / W, mq[a] = sums[4 + a] / W;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[a][b] = sums[7 + 3 * a + b] - W * mp[a] * mq[b];
    const double pp = sums[16] - W * (mp[0] * mp[0] + mp[1] * mp[1] + mp[2] * mp[2]);
    double n[4][4] = {{H[0][0] + H[1][1] + H[2][2], H[1][2] - H[2][1], H[2][0] - H[0][2], H[0][1] - H[1][0]},
                      {0, H[0][0] - H[1][1] - H[2][2], H[0][1] + H[1][0], H[2][0] + H[0][2]},
                      {0, 0, -H[0][0] + H[1][1] - H[2][2], H[1][2] + H[2][1]},
                      {0, 0, 0, -H[0][0] - H[1][1] + H[2][2]}};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < i; ++j) n[i][j] = n[j][i];
    double qv[4];
    max_eigenvector4(n, qv);
    const double nq = sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2] + qv[3] * qv[3]);
    const double w = qv[0] / nq, x = qv[1] / nq, y = qv[2] / nq, z = qv[3] / nq;
    Sim o;
    o.r[0] = 1.0 - 2.0 * (y * y + z * z), o.r[1] = 2.0 * (x * y - w * z), o.r[2] = 2.0 * (x * z + w * y);
    o.r[3] = 2.0 * (x * y + w * z), o.r[4] = 1.0 - 2.0 * (x * x + z * z), o.r[5] = 2.0 * (y * z - w * x);
    o.r[6] = 2.0 * (x * z - w * y), o.r[7] = 2.0 * (y * z + w * x), o.r[8] = 1.0 - 2.0 * (x * x + y * y);
    o.s = 1.0;
    if (with_scale) {
        double num = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) num += o.r[3 * i + j] * H[j][i];
        if (pp > 0.0 && num > 0.0) o.s = num / pp;
    }
    for (int i = 0; i < 3; ++i) o.t[i] = mq[i] - o.s * (o.r[3 * i] * mp[0] + o.r[3 * i + 1] * mp[1] + o.r[3 * i + 2] * mp[2]);
    *out = about_centre(o, c);
    return true;
}

// One Gauss-Newton step of the point-to-plane method: x = [omega, tau, sigma] minimises sum w (r - j . x)^2, i.e. solves the
// 6 x 6 (7 x 7 with scale) normal equations A x = b held in the kFitPlaneTerms sums.  Cholesky, A = L L^T, column by column;
// FALLBACK: a column whose pivot is not above 1e-12 of its own diagonal entry -- a degree of freedom that the shape does not
// constrain beyond what the earlier columns already explain (a plane leaves its in-plane shifts and spin open, a sphere its
// rotations) -- is taken out of the system and its component of x stays 0.  The update is p -> (1 + sigma) exp([omega]x) p + tau
// about c, exp by Rodrigues' formula (exact, not the linearisation).  false: W <= 0 or a non-finite sum.
inline bool solve_plane(const double* sums, bool with_scale, const double c[3], Sim* out, int* dropped_out = nullptr) {
    for (int i = 0; i < r3g_md::kFitPlaneTerms; ++i)
        if (!(sums[i] - sums[i] == 0.0)) return false;
    if (!(sums[35] > 0.0)) return false;
    const int n = with_scale ? 7 : 6;
    double A[7][7], L[7][7] = {}, b[7], y[7], x[7] = {};
    bool keep[7];
    int k = 0, dropped = 0;
    for (int i = 0; i < 7; ++i) {
        for (int j = i; j < 7; ++j) A[i][j] = A[j][i] = sums[k++];
        b[i] = sums[28 + i];
    }
    for (int j = 0; j < n; ++j) {
        double d = A[j][j];
        for (int m = 0; m < j; ++m)
            if (keep[m]) d -= L[j][m] * L[j][m];
        keep[j] = A[j][j] > 0.0 && d > 1e-12 * A[j][j];
        if (!keep[j]) {
            ++dropped;
            continue;
        }
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < n; ++i) {
            double v = A[i][j];
            for (int m = 0; m < j; ++m)
                if (keep[m]) v -= L[i][m] * L[j][m];
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        double v = b[i];
        for (int m = 0; m < i; ++m)
            if (keep[m]) v -= L[i][m] * y[m];
        y[i] = v / L[i][i];
    }
    for (int i = n - 1; i >= 0; --i) {
        if (!keep[i]) continue;
        double v = y[i];
        for (int m = i + 1; m < n; ++m)
            if (keep[m]) v -= L[m][i] * x[m];
        x[i] = v / L[i][i];
    }
    if (dropped_out) *dropped_out = dropped;
    const double th2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2], th = sqrt(th2);
    // sin(th) / th and (1 - cos(th)) / th^2, by their series where th is tiny
    const double ka = th > 1e-4 ? sin(th) / th : 1.0 - th2 / 6.0;
    const double kb = th > 1e-4 ? (1.0 - cos(th)) / th2 : 0.5 - th2 / 24.0;
    const double K[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
    Sim o;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
            o.r[3 * i + j] = (i == j ? 1.0 : 0.0) + ka * K[3 * i + j] + kb * kk;
        }
    o.s = with_scale ? 1.0 + x[6] : 1.0;
    if (!(o.s > 0.0)) o.s = 1.0;
    for (int i = 0; i < 3; ++i) o.t[i] = x[3 + i];
    *out = about_centre(o, c);
    return true;
}

}  // namespace r3g_mf
#endif
