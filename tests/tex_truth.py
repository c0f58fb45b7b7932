"""Ground truth for the texture-stage pixel kernels, written from the contract in include/r3g.h "texture stage" and NOT from
the kernels: exact rational arithmetic (fractions.Fraction on the exact values of the float32 inputs) where a decision is
made, float64 where a bound derived below covers its error.  oracle/tex_ref.py repeats the kernels' float32 arithmetic
operation by operation, so a rule that is wrong in both passes their bit-for-bit comparison; it cannot pass this file.

Notation: u = 2^-24 is the unit roundoff of float32 (round to nearest), v = 2^-53 that of float64.

RASTERISER.  The contract: pixel (ix, iy) samples the point (ix + 1/2, iy + 1/2) of the screen X = (x/w/2 + 1/2)(W-1) + 1/2,
Y likewise with H; a face is drawn where the sample lies inside it or on its border (all w > 0, area finite and not zero)
and its depth Z = (z/w) c + 1/2, c = float32(0.49999), lies in [0, 1]; the nearest face wins, the smaller index on a tie;
the barycentrics written are the perspective-correct ones, O_k = (B_k / w_k) / sum_j (B_j / w_j), B the screen-space ones.

 (1) Screen coordinate.  float32 evaluates X with four roundings (x/w; the halving is exact; +1/2; *(W-1), W-1 exact; +1/2).
     With M = (W-1)(|x/w|/2 + 1/2) + 1/2 >= |X| every intermediate is at most M in magnitude after scaling to screen units,
     and each rounding adds at most u times that, so |X^ - X| <= 4 u M (1 + O(u)).  dX := 5 u M absorbs the O(u^2) terms.
     Z: three roundings (division, product with c, sum), |Z^ - Z| <= dZ := 4 u (|z/w|/2 + 1/2).
 (2) Cross product.  Every quantity the rasteriser decides on is C = d1 d2 - d3 d4 with d_i a difference of two coordinates
     (a pixel centre is exact, a vertex is off by dX).  With D_i = |d_i| exact and e_i = (sum of the operands' dX)(1 + u) +
     u D_i the error of the rounded difference, a rounded product errs by
         P(i, j) = e_i D_j + e_j D_i + e_i e_j + u (D_i + e_i)(D_j + e_j)
     and the final subtraction by u (|d1 d2| + |d3 d4| + P(1,2) + P(3,4)), so
         |C^ - C| <= cross_bound := (1 + u)(P(1,2) + P(3,4)) + u (D1 D2 + D3 D4).
     This holds for the edge functions in whichever order and sign they are evaluated (a swap of the endpoints changes no
     magnitude), for the numerators of the screen barycentrics and for the area.  The float64 evaluation of C and of the
     bound itself errs by a few v of the same magnitudes; the factor (1 + 2^-20) on the bound covers it 2^9 times over.
 (3) Class of a (pixel, face) pair, s = sign of the exact area: STRICTLY INSIDE when s E_k > bound_k for all three edges,
     STRICTLY OUTSIDE when s E_k < -bound_k for one, AMBIGUOUS otherwise.  No float32 evaluation within (2) can reject a
     strictly inside sample or admit a strictly outside one.
 (4) Near-degenerate faces.  A face is excluded from the value checks (and counted in the excluded share) when its exact
     area is below AREA_MIN_RATIO = 2^-10 times the square of its longest edge, or below 8 times its own cross_bound (the
     float32 area then has fewer than three good bits and its sign is not safe).  Such a face is never REQUIRED to be drawn,
     and where it is drawn it must still not be strictly outside.
 (5) Screen barycentric b_k = N_k / A (N_k as in (2), float32 division): |b^ - B| <= beta_k := (nb_k + |B_k| ab) / (|A| - ab)
     + u |B_k|, nb_k and ab the cross_bounds of numerator and area.  The kernels clamp at 0; a sample they admit has
     s E_k >= -bound_k, i.e. B_k >= -bound_k / |A|, so after the clamp the error is at most beta_k + bound_k / |A|.
     b_2 = 1 - b_0 - b_1 adds two roundings of quantities <= 1 + beta: beta_2 := beta_0 + beta_1 + 2 u (1 + beta_0 + beta_1).
 (6) Depth = sum b_k z_k (three products, two sums, all terms <= max|Z| (1 + beta)):
         dbound := sum_k (beta_k |Z_k| + dZ_k (|B_k| + beta_k)) + 5 u sum_k (|B_k| + beta_k)(|Z_k| + dZ_k).
 (7) Perspective: c_k = b_k / w_k errs by gc_k = beta_k / w_k + u (|B_k| + beta_k) / w_k; S = sum c_k by gs = sum gc_k +
     2 u (S + sum gc_k); o_k = c_k / S by  (gc_k + |O_k| gs) / (S - gs) + u |O_k|.  Their float32 sum is within 4 u of 1
     (three quotients by the same S, each within u, two additions).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
AREA_MIN_RATIO = 2.0 ** -10
C_DEPTH = float(np.float32(0.49999))
F32 = np.float32
INSIDE, AMBIGUOUS, OUTSIDE = 1, 0, -1


# ---- exact helpers ------------------------------------------------------------------------------------------------
def frac(x):
    return Fraction(float(x))


def exact_screen(p, H, W):
    """exact screen X, Y and depth Z of one clip-space vertex (four float32), as Fractions"""
    x, y, z, w = (frac(t) for t in p)
    return ((x / w / 2 + Fraction(1, 2)) * (W - 1) + Fraction(1, 2), (y / w / 2 + Fraction(1, 2)) * (H - 1) + Fraction(1, 2),
            z / w * Fraction(C_DEPTH) + Fraction(1, 2))


def exact_edges(pos, face, H, W, ix, iy):
    """the three exact edge functions of pixel (ix, iy) times the sign of the exact area (>= 0: inside or on the border)"""
    v = [exact_screen(pos[i], H, W) for i in face]
    px, py = Fraction(2 * ix + 1, 2), Fraction(2 * iy + 1, 2)
    area = (v[1][0] - v[0][0]) * (v[2][1] - v[0][1]) - (v[2][0] - v[0][0]) * (v[1][1] - v[0][1])
    s = (area > 0) - (area < 0)
    out = []
    for k in range(3):
        a, b = v[(k + 1) % 3], v[(k + 2) % 3]
        out.append(s * ((b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])))
    return out


def _cross(d, e):
    """value and cross_bound (2) of d[0] d[1] - d[2] d[3]; d exact differences (float64), e their error bounds"""
    D = [np.abs(t) for t in d]
    P = lambda i, j: e[i] * D[j] + e[j] * D[i] + e[i] * e[j] + U * (D[i] + e[i]) * (D[j] + e[j])   # noqa: E731
    bound = ((1 + U) * (P(0, 1) + P(2, 3)) + U * (D[0] * D[1] + D[2] * D[3])) * SLACK
    return d[0] * d[1] - d[2] * d[3], bound


def _diff(a, da, b, db):
    d = a - b
    return d, (da + db) * (1 + U) + U * np.abs(d)


class RasterTruth:
    """per-scene truth of the rasteriser.  Fields (image-shaped unless said):
       must_cover     some drawable face is strictly inside with its depth safely in [0, 1]
       may_cover      some face that is not near-degenerate is inside or ambiguous (a scene called closed has it everywhere)
       min_depth      smallest exact depth among those faces (inf where none), min_dbound its depth bound (6)
       pairs, ambiguous_pairs, degenerate_pairs   counts over (pixel in the face's box, face with all w > 0)
       canon[f]       smallest index of a face whose three vertices are bit-identical to f's, in order (exact depth ties)"""

    def __init__(self, pos, tri, H, W):
        pos = np.asarray(pos, F32)
        tri = np.asarray(tri, np.int64).reshape(-1, 3)
        self.H, self.W, self.pos, self.tri = H, W, pos, tri
        p = pos.astype(np.float64)
        with np.errstate(all="ignore"):
            qx, qy, qz = p[:, 0] / p[:, 3], p[:, 1] / p[:, 3], p[:, 2] / p[:, 3]
            self.X = (qx / 2 + 0.5) * (W - 1) + 0.5
            self.Y = (qy / 2 + 0.5) * (H - 1) + 0.5
            self.Z = qz * C_DEPTH + 0.5
            self.dX = 5 * U * ((W - 1) * (np.abs(qx) / 2 + 0.5) + 0.5)
            self.dY = 5 * U * ((H - 1) * (np.abs(qy) / 2 + 0.5) + 0.5)
            self.dZ = 4 * U * (np.abs(qz) / 2 + 0.5)
        self.w = p[:, 3]
        F = len(tri)
        self.front = np.array([bool((self.w[t] > 0).all() and np.isfinite(pos[t]).all()) for t in tri], bool) if F else np.zeros(0, bool)
        self.area = np.zeros(F)
        self.area_bound = np.zeros(F)
        self.degenerate = np.ones(F, bool)
        for f in np.nonzero(self.front)[0]:
            a, ab, L2 = self._area(f)
            self.area[f], self.area_bound[f] = a, ab
            # float32 must be able to form the products: a magnitude bound keeps them finite
            finite = np.isfinite(a) and np.isfinite(ab) and L2 < 2.0 ** 120
            self.degenerate[f] = not (finite and abs(a) >= AREA_MIN_RATIO * L2 and abs(a) >= 8 * ab and a != 0)
        key = {}
        self.canon = np.arange(F)
        for f in range(F):
            k = pos[tri[f]].tobytes()
            self.canon[f] = key.setdefault(k, f)
        self.must_cover = np.zeros((H, W), bool)
        self.may_cover = np.zeros((H, W), bool)
        self.min_depth = np.full((H, W), np.inf)
        self.min_dbound = np.zeros((H, W))
        self.pairs = self.ambiguous_pairs = self.degenerate_pairs = 0
        for f in np.nonzero(self.front)[0]:
            self._accumulate(f)

    def _area(self, f):
        i0, i1, i2 = self.tri[f]
        X, Y, dX, dY = self.X, self.Y, self.dX, self.dY
        d, e = zip(_diff(X[i1], dX[i1], X[i0], dX[i0]), _diff(Y[i2], dY[i2], Y[i0], dY[i0]),
                   _diff(X[i2], dX[i2], X[i0], dX[i0]), _diff(Y[i1], dY[i1], Y[i0], dY[i0]))
        a, ab = _cross(d, e)
        L2 = max((X[i] - X[j]) ** 2 + (Y[i] - Y[j]) ** 2 for i, j in ((i0, i1), (i1, i2), (i2, i0)))
        return float(a), float(ab), float(L2)

    def at(self, f, px, py):
        """face f (scalar or array) at the pixel centres (px, py) (float64 arrays): dict of class, exact depth, dbound, exact
        perspective-correct barycentrics O [.., 3] and their bound obound [.., 3]"""
        f = np.asarray(f)
        t = self.tri[f]
        X, Y, Z, w = self.X[t], self.Y[t], self.Z[t], self.w[t]            # [..., 3]
        dX, dY, dZ = self.dX[t], self.dY[t], self.dZ[t]
        A, AB = self.area[f], self.area_bound[f]
        s = np.sign(A)
        zero = np.zeros_like(px)
        with np.errstate(all="ignore"):
            E, EB, B, beta = [], [], [], []
            for k in range(3):
                a, b = (k + 1) % 3, (k + 2) % 3
                d, e = zip(_diff(X[..., b], dX[..., b], X[..., a], dX[..., a]), _diff(py, zero, Y[..., a], dY[..., a]),
                           _diff(Y[..., b], dY[..., b], Y[..., a], dY[..., a]), _diff(px, zero, X[..., a], dX[..., a]))
                ek, ebk = _cross(d, e)
                E.append(s * ek)
                EB.append(ebk)
                # the numerator of screen barycentric k as the contract's b_k = ((x_a - p)(y_b - p) - (x_b - p)(y_a - p)) / area
                d, e = zip(_diff(X[..., a], dX[..., a], px, zero), _diff(Y[..., b], dY[..., b], py, zero),
                           _diff(X[..., b], dX[..., b], px, zero), _diff(Y[..., a], dY[..., a], py, zero))
                nk, nbk = _cross(d, e)
                bk = nk / A
                B.append(bk)
                beta.append(((nbk + np.abs(bk) * AB) / (np.abs(A) - AB) + U * np.abs(bk) + ebk / np.abs(A)) * SLACK)
            beta[2] = np.maximum(beta[2], beta[0] + beta[1] + 2 * U * (1 + beta[0] + beta[1]))
            E, EB, B, beta = (np.stack(v, -1) for v in (E, EB, B, beta))
            cls = np.where((E > EB).all(-1), INSIDE, np.where((E < -EB).any(-1), OUTSIDE, AMBIGUOUS))
            depth = (B * Z).sum(-1)
            dbound = ((beta * np.abs(Z) + dZ * (np.abs(B) + beta)).sum(-1) + 5 * U * ((np.abs(B) + beta) * (np.abs(Z) + dZ)).sum(-1)) * SLACK
            c = B / w
            S = c.sum(-1, keepdims=True)
            O = c / S
            gc = beta / w + U * (np.abs(B) + beta) / w
            gs = gc.sum(-1, keepdims=True) + 2 * U * (np.abs(S) + gc.sum(-1, keepdims=True))
            obound = ((gc + np.abs(O) * gs) / (np.abs(S) - gs) + U * np.abs(O)) * SLACK
        return dict(cls=cls, depth=depth, dbound=dbound, O=O, obound=obound, E=E, EB=EB)

    def _accumulate(self, f):
        H, W = self.H, self.W
        t = self.tri[f]
        lo_x, hi_x = self.X[t].min() - self.dX[t].max() - 2, self.X[t].max() + self.dX[t].max() + 2
        lo_y, hi_y = self.Y[t].min() - self.dY[t].max() - 2, self.Y[t].max() + self.dY[t].max() + 2
        if not (hi_x >= 0 and hi_y >= 0 and lo_x <= W and lo_y <= H):
            return
        x0, x1 = int(max(0.0, np.floor(lo_x))), int(min(W - 1.0, np.ceil(hi_x)))
        y0, y1 = int(max(0.0, np.floor(lo_y))), int(min(H - 1.0, np.ceil(hi_y)))
        if x1 < x0 or y1 < y0:
            return
        gx, gy = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
        n = gx.size
        self.pairs += n
        if self.degenerate[f]:
            self.degenerate_pairs += n
            return
        r = self.at(np.full(gx.shape, f), gx + 0.5, gy + 0.5)
        self.ambiguous_pairs += int((r["cls"] == AMBIGUOUS).sum())
        self.may_cover[gy[r["cls"] != OUTSIDE], gx[r["cls"] != OUTSIDE]] = True
        sure = (r["cls"] == INSIDE) & (r["depth"] - r["dbound"] >= 0) & (r["depth"] + r["dbound"] <= 1)
        ys, xs = gy[sure], gx[sure]
        self.must_cover[ys, xs] = True
        better = r["depth"][sure] < self.min_depth[ys, xs]
        self.min_depth[ys[better], xs[better]] = r["depth"][sure][better]
        self.min_dbound[ys[better], xs[better]] = r["dbound"][sure][better]

    @property
    def excluded_share(self):
        return (self.ambiguous_pairs + self.degenerate_pairs) / max(1, self.pairs)


def check_raster(truth, findices, bary, closed=False):
    """every rasteriser check of the issue on one result; -> (list of failure strings, dict of measured figures)"""
    fi = np.asarray(findices).astype(np.int64)
    bary = np.asarray(bary, F32)
    H, W = truth.H, truth.W
    fails, m = [], {}
    assert fi.shape == (H, W) and bary.shape == (H, W, 3)
    if fi.min() < 0 or fi.max() > len(truth.tri):
        return ["face ids outside [0, F]"], m
    covered = fi > 0
    m["covered"], m["holes"] = int(covered.sum()), int((~covered).sum())
    miss = truth.must_cover & ~covered
    if miss.any():
        fails.append("cover: %d pixels strictly inside a drawable face are empty, first (y, x) = %s" % (miss.sum(), np.argwhere(miss)[0]))
    if closed and not covered.all():
        fails.append("closed mesh: %d pixels uncovered, first (y, x) = %s" % ((~covered).sum(), np.argwhere(~covered)[0]))
    if np.abs(bary[~covered]).sum() != 0:
        fails.append("barycentrics of empty pixels are not zero")
    ys, xs = np.nonzero(covered)
    m["depth_ratio"] = m["bary_ratio"] = m["sum_ulps"] = 0.0
    if len(ys):
        f = fi[ys, xs] - 1
        if not truth.front[f].all():
            fails.append("sound: a face with w <= 0 or a non-finite vertex was drawn")
            return fails, m
        if (truth.canon[f] != f).any():
            fails.append("tie: a face was drawn although a bit-identical face with a smaller index exists")
        r = truth.at(f, xs + 0.5, ys + 0.5)
        bad = r["cls"] == OUTSIDE
        if bad.any():
            fails.append("sound: %d pixels report a face that is strictly outside, first (y, x) = (%d, %d)" % (bad.sum(), ys[bad][0], xs[bad][0]))
        ok = ~truth.degenerate[f]
        with np.errstate(all="ignore"):
            dz = ((r["depth"] < -r["dbound"]) | (r["depth"] > 1 + r["dbound"])) & ok
            if dz.any():
                fails.append("sound: %d pixels report a face whose exact depth is outside [0, 1]" % dz.sum())
            near = ok & np.isfinite(truth.min_depth[ys, xs])
            slack = r["dbound"] + truth.min_dbound[ys, xs]
            excess = r["depth"] - truth.min_depth[ys, xs]
            if near.any():
                m["depth_ratio"] = float(np.max(np.where(near & (slack > 0), excess / np.where(slack > 0, slack, 1), 0)))
                far = near & (excess > slack)
                if far.any():
                    fails.append("nearest: %d pixels report a face behind a strictly covering one" % far.sum())
        b = bary[ys, xs].astype(np.float64)
        if not (b >= 0).all():                          # also false for a NaN
            fails.append("barycentrics: %d values negative or NaN" % (~(b >= 0)).sum())
        s = bary[ys, xs, 0].astype(F32) + bary[ys, xs, 1] + bary[ys, xs, 2]
        m["sum_ulps"] = float(np.nanmax(np.abs(s.astype(np.float64) - 1)) / U)
        if not m["sum_ulps"] <= 4:
            fails.append("barycentrics: sum differs from 1 by %.1f u (allowed 4)" % m["sum_ulps"])
        if ok.any():
            with np.errstate(all="ignore"):
                ratio = np.abs(b[ok] - r["O"][ok]) / r["obound"][ok]
            m["bary_ratio"] = float(np.nanmax(ratio)) if np.isfinite(ratio).any() else 0.0
            if not np.all(ratio[np.isfinite(r["obound"][ok])] <= 1):
                fails.append("barycentrics: error / bound %.3g" % np.nanmax(ratio))
    return fails, m


# ---- interpolate --------------------------------------------------------------------------------------------------
def interpolate_truth(attr, tri, findices, bary):
    """float64 value and bound: three float32 products and two sums, |err| <= 3 u sum_k |b_k a_k| (gamma_3)"""
    attr = np.asarray(attr, np.float64)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    fi = np.asarray(findices).reshape(-1).astype(np.int64)
    b = np.asarray(bary, np.float64).reshape(-1, 3)
    out = np.zeros((len(fi), attr.shape[1]))
    bound = np.zeros_like(out)
    m = fi > 0
    t = tri[fi[m] - 1]
    terms = np.stack([b[m, k:k + 1] * attr[t[:, k]] for k in range(3)])
    out[m] = terms.sum(0)
    bound[m] = 3 * U * SLACK * np.abs(terms).sum(0)
    return out, bound


# ---- view weight --------------------------------------------------------------------------------------------------
def view_weight_truth(findices, depth, normal, cos_threshold, depth_edge, view_w, power):
    """-> keep (bool), decided (bool: the exact rule is more than a rounding away from its threshold, or exactly on it),
    value float64 (view_w cos^power; NaN where the power of a negative cosine is not real).
    Rule: a covered pixel is kept when cos = n_z / |n| >= cos_threshold (a zero-length or non-finite normal has cos 0 / is
    dropped), all four neighbours exist and are covered, and no neighbour's depth differs by MORE than depth_edge.
    The comparisons are made on exact rationals; float32 forms cos through three squares, two sums, a root and a quotient,
    each within u of relative error and the squares and sums halved by the root: a cosine within 6 u of the threshold but
    not ON it is undecided; on it, it is kept -- which
    float32 reproduces when its squares and root are exact (the scenes use Pythagorean normals there).  A depth step is a
    single float32 subtraction: undecided within u of depth_edge, decided (kept) when exactly equal."""
    fi = np.asarray(findices)
    H, W = fi.shape
    d = np.asarray(depth, F32)
    n = np.asarray(normal, F32)
    thr, edge = Fraction(float(F32(cos_threshold))), Fraction(float(F32(depth_edge)))
    keep = np.zeros((H, W), bool)
    decided = np.ones((H, W), bool)
    value = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            if fi[y, x] <= 0:
                continue
            nv = n[y, x]
            if not np.isfinite(nv).all():
                ok, cos = False, 0.0                       # NaN compares false everywhere: dropped
                if np.isinf(nv).any() and not np.isnan(nv).any():
                    decided[y, x] = False                  # inf / inf: the contract does not say
            else:
                l2 = sum(frac(c) ** 2 for c in nv)
                cos = float(nv[2]) / float(l2) ** 0.5 if l2 > 0 else 0.0
                nz = frac(nv[2])
                if l2 == 0:
                    ok = thr <= 0
                else:   # nz / sqrt(l2) >= thr  on exact rationals
                    lhs_neg, rhs_neg = nz < 0, thr < 0
                    if not lhs_neg and rhs_neg:
                        ok = True
                    elif lhs_neg and not rhs_neg:
                        ok = False
                    elif not lhs_neg:
                        ok = nz * nz >= thr * thr * l2
                    else:
                        ok = nz * nz <= thr * thr * l2
                    on = nz * nz == thr * thr * l2 and lhs_neg == rhs_neg
                    if not on and abs(cos - float(thr)) <= 6 * U:
                        decided[y, x] = False
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                xx, yy = x + dx, y + dy
                if xx < 0 or yy < 0 or xx >= W or yy >= H or fi[yy, xx] <= 0:
                    ok = False
                    continue
                if not (np.isfinite(d[yy, xx]) and np.isfinite(d[y, x])):
                    continue                               # a NaN step is not "more than": kept (comparison false)
                step = abs(frac(d[yy, xx]) - frac(d[y, x]))
                if step > edge:
                    ok = False
                if step != edge and abs(float(step - edge)) <= U * float(step):
                    decided[y, x] = False
            keep[y, x] = ok
            if ok:
                with np.errstate(all="ignore"):
                    value[y, x] = float(view_w) * np.power(np.float64(cos), np.float64(F32(power)))
    return keep, decided, value


# ---- bakers -------------------------------------------------------------------------------------------------------
def _half_up(x):
    """floor(x + 1/2) of a Fraction"""
    return (2 * x.numerator + x.denominator) // (2 * x.denominator)


def weight_fixed(w):
    """the 16.16 weight of the contract: 0 unless w > 0; round-half-up of min(w, 65535) 2^16.  The kernels add 1/2 in
    float32, which is exact below 2^23 and above 2^24 only for even values: the truth refuses other weights."""
    w = float(w)
    if not w > 0:                                      # also NaN
        return 0
    x = Fraction(min(w, 65535.0)) * 65536
    if x >= 2 ** 23 and (x.denominator != 1 or (x.numerator % 2 and x < 2 ** 24)):
        raise ValueError("weight %r: float32 cannot add 1/2 to it exactly, outside this truth's domain" % w)
    return _half_up(x)


def colour_fixed(c):
    """16.16 colour: clamp to [0, 1], round-half-up of c 2^16 (float32 adds the 1/2 exactly for every c whose 2^16-fold
    has at most 8 fractional bits above 1/2, e.g. every k 2^-24; the truth refuses a colour where the sum would round)"""
    c = float(c)
    cc = min(max(c, 0.0), 1.0)
    x = Fraction(cc) * 65536 + Fraction(1, 2)
    if Fraction(float(F32(float(x)))) != x and int(F32(float(x))) != x.numerator // x.denominator:
        raise ValueError("colour %r: float32 rounds c 2^16 + 1/2 across an integer, outside this truth's domain" % c)
    return x.numerator // x.denominator


def texel_exact(u, T):
    """texel = round-half-up(u (T-1)) clamped to [0, T-1]; u a Fraction or +-inf as float; None for NaN.  Also returns
    the distance of u (T-1) + 1/2 to the nearest integer boundary (0 = exactly on a k + 1/2 rounding boundary)"""
    if isinstance(u, float):
        if u != u or (T == 1 and u in (float("inf"), float("-inf"))):
            return None, 1.0
        return (T - 1 if u > 0 else 0), 1.0
    x = u * (T - 1) + Fraction(1, 2)
    k = x.numerator // x.denominator
    return min(max(k, 0), T - 1), float(min(x - k, k + 1 - x)) if 0 < x < T - 1 else 1.0


def bake_truth(image, weight, findices, bary, uv, uv_tri, T):
    """closed-form integer accumulators of one scatter bake, Python integers [T, T, 4].  A pixel contributes when it is
    covered, its weight is > 0 and not below half a fixed-point step, no colour channel is NaN and its texture coordinate is
    not NaN.  The texture coordinate is the float32 sum b0 u0 + b1 u1 + b2 u2 (part of the interface: it is what
    interpolate() returns); the texel rule is applied to its exact value.  -> acc, on_boundary (pixels whose u (T-1) + 1/2
    sits within 3 u T of an integer without being exactly there: float32 may round either way, the caller avoids them)"""
    acc = np.zeros((T, T, 4), object)
    acc[...] = 0
    fi = np.asarray(findices).reshape(-1)
    w = np.asarray(weight, F32).reshape(-1)
    img = np.asarray(image, F32).reshape(-1, 3)
    b = np.asarray(bary, F32).reshape(-1, 3)
    uv = np.asarray(uv, F32)
    uv_tri = np.asarray(uv_tri, np.int64).reshape(-1, 3)
    on_boundary = 0
    for i in range(len(fi)):
        if fi[i] <= 0 or np.isnan(img[i]).any():
            continue
        wq = weight_fixed(w[i])
        if wq == 0:
            continue
        t = uv_tri[fi[i] - 1]
        tex = []
        for c in range(2):
            with np.errstate(all="ignore"):
                val = F32(F32(b[i, 0] * uv[t[0], c]) + F32(b[i, 1] * uv[t[1], c])) + F32(b[i, 2] * uv[t[2], c])
            k, dist = texel_exact(Fraction(float(val)) if np.isfinite(val) else float(val), T)
            if 0 < dist < 3 * U * T:
                on_boundary += 1
            tex.append(k)
        if tex[0] is None or tex[1] is None:
            continue
        for c in range(3):
            acc[tex[1], tex[0], c] += wq * colour_fixed(img[i, c])
        acc[tex[1], tex[0], 3] += wq
    return acc, on_boundary


def bake_gather_truth(findices_uv, bary_uv, clip_uv, uv_tri, image, weight, findices, depth, depth_eps):
    """float64 truth of the texel-centric bake: -> wq int [T, T] (the weight channel, exact), colour float64 [T, T, 3]
    (bilinear sample, clamped at the border; the colour channels must equal wq * round(colour 2^16) within one fixed-point
    step per unit of wq), decided bool [T, T] (False where a float32 rounding could move the texel to another pixel, across
    the depth test or across w = 0)"""
    T = np.asarray(findices_uv).shape[0]
    H, W = np.asarray(findices).shape
    fu = np.asarray(findices_uv).reshape(-1)
    bu = np.asarray(bary_uv, np.float64).reshape(-1, 3)
    cu = np.asarray(clip_uv, np.float64)
    ut = np.asarray(uv_tri, np.int64).reshape(-1, 3)
    img = np.asarray(image, np.float64)
    wgt = np.asarray(weight, F32)
    dep = np.asarray(depth, np.float64)
    wq = np.zeros(T * T, np.int64)
    col = np.zeros((T * T, 3))
    decided = np.ones(T * T, bool)
    eps = float(F32(depth_eps))
    for i in np.nonzero(fu > 0)[0]:
        t = ut[fu[i] - 1]
        with np.errstate(all="ignore"):
            p = bu[i, 0] * cu[t[0]] + bu[i, 1] * cu[t[1]] + bu[i, 2] * cu[t[2]]
            mag = np.abs(bu[i, 0] * cu[t[0]]) + np.abs(bu[i, 1] * cu[t[1]]) + np.abs(bu[i, 2] * cu[t[2]])
        if np.isnan(p).any():
            continue                                       # a NaN coordinate contributes nothing
        if not p[3] > 0:
            decided[i] = not (abs(p[3]) <= 3 * U * mag[3]) or p[3] == 0 and mag[3] == 0
            continue
        if p[3] <= 3 * U * mag[3]:
            decided[i] = False
            continue
        sx = (p[0] / p[3] / 2 + 0.5) * (W - 1) + 0.5
        sy = (p[1] / p[3] / 2 + 0.5) * (H - 1) + 0.5
        z = p[2] / p[3]
        # float32 error of sx: the interpolation (3 u mag), the division and the screen transform as in (1)
        ex = 8 * U * ((W - 1) * ((mag[0] + abs(p[0])) / p[3] / 2 + 0.5) + 0.5) * (1 + mag[3] / p[3])
        ey = 8 * U * ((H - 1) * ((mag[1] + abs(p[1])) / p[3] / 2 + 0.5) + 0.5) * (1 + mag[3] / p[3])
        ez = 8 * U * ((mag[2] + abs(p[2])) / p[3]) * (1 + mag[3] / p[3])
        if not (sx >= 0 and sy >= 0 and sx < W and sy < H):
            decided[i] = min(abs(sx), abs(sy), abs(sx - W), abs(sy - H)) > max(ex, ey) or sx in (0.0, float(W)) or sy in (0.0, float(H))
            continue
        px, py = int(np.floor(sx)), int(np.floor(sy))
        if (sx - px < ex and sx != px) or (px + 1 - sx < ex) or (sy - py < ey and sy != py) or (py + 1 - sy < ey):
            decided[i] = False
        fx, fy = sx - 0.5, sy - 0.5                        # (the bilinear form is continuous across a pixel centre: no margin needed)
        w = wgt[py, px]
        if findices[py, px] <= 0 or not w > 0:
            continue
        lim = dep[py, px] + eps
        if abs(z - lim) <= ez + 2 * U * abs(lim) and z != lim:
            decided[i] = False
        if not z <= lim:
            continue
        q = weight_fixed(w)
        if q == 0:
            continue
        x0, y0 = int(np.floor(fx)), int(np.floor(fy))
        ax, ay = fx - x0, fy - y0
        x1, y1 = min(max(x0 + 1, 0), W - 1), min(max(y0 + 1, 0), H - 1)
        x0, y0 = min(max(x0, 0), W - 1), min(max(y0, 0), H - 1)
        top = img[y0, x0] + (img[y0, x1] - img[y0, x0]) * ax
        bot = img[y1, x0] + (img[y1, x1] - img[y1, x0]) * ax
        c = top + (bot - top) * ay
        if np.isnan(c).any():
            continue
        wq[i], col[i] = q, c
    return wq.reshape(T, T), col.reshape(T, T, 3), decided.reshape(T, T)


def finalize_truth(acc):
    """acc: integers [T, T, 4] -> texture float32 (the quotient acc_c / (acc_w 2^16) rounded once to float64 and once to
    float32: within one float32 ulp of the correctly rounded quotient, which is what the check allows), mask uint8"""
    a = np.asarray(acc, object)
    T = a.shape[0]
    tex = np.zeros((T, T, 3), F32)
    mask = np.zeros((T, T), np.uint8)
    for y in range(T):
        for x in range(T):
            w = int(a[y, x, 3])
            if w:
                mask[y, x] = 1
                for c in range(3):
                    tex[y, x, c] = F32(float(Fraction(int(a[y, x, c]), w * 65536)))
    return tex, mask


def ulp_distance(a, b):
    """distance in float32 ulps between two finite float32 arrays of the same sign convention (>= 0 here)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- inpainting ---------------------------------------------------------------------------------------------------
def seeded_vertices(mask, uv, uv_tri, pos_tri, T, margin=1e-4):
    """the vertices that own a painted texel: corner c of a face looks at the texel of 3/4 of its UV + 1/4 of the chart
    triangle's centroid (exact rationals; the rule is refused within `margin` texels of a rounding boundary, where float32
    may land on the other side).  -> bool [V]"""
    uv = np.asarray(uv, F32)
    uv_c = np.asarray(uv_tri, np.int64).reshape(-1)
    pos_c = np.asarray(pos_tri, np.int64).reshape(-1)
    V = int(pos_c.max()) + 1
    seeded = np.zeros(V, bool)
    mask = np.asarray(mask)
    for c in range(len(uv_c)):
        f3 = c - c % 3
        tex = []
        for k in range(2):
            vals = [uv[uv_c[f3 + j], k] for j in range(3)]
            own = uv[uv_c[c], k]
            if not np.isfinite(vals + [own]).all():
                tex.append(None)
                continue
            cen = sum(frac(t) for t in vals) / 3
            t, dist = texel_exact(frac(own) * Fraction(3, 4) + cen / 4, T)
            if dist < margin:
                raise ValueError("corner %d sits on a texel rounding boundary: outside this truth's domain" % c)
            tex.append(t)
        if tex[0] is not None and tex[1] is not None and mask[tex[1], tex[0]]:
            seeded[pos_c[c]] = True
    return seeded


def propagation_rounds(seeded, verts, pos_tri):
    """the number of Jacobi rounds that change something = the largest breadth-first distance from the seeded vertices in
    the vertex graph, whose edges join the distinct vertices of a face that are no further apart than the weight's
    resolution: round(1024 / (d^2 + 1e-6)) >= 1, i.e. d^2 + 1e-6 <= 2048 (refused within 1e-3 relative of that).
    -> rounds, reached bool [V]"""
    verts = np.asarray(verts, np.float64)
    tri = np.asarray(pos_tri, np.int64).reshape(-1, 3)
    V = len(verts)
    nb = [set() for _ in range(V)]
    for t in tri:
        for i in range(3):
            a, b = int(t[i]), int(t[(i + 1) % 3])
            if a == b:
                continue
            d2 = float(((verts[a] - verts[b]) ** 2).sum())
            if not np.isfinite(d2):
                continue
            if abs(d2 + 1e-6 - 2048) < 2.048:
                raise ValueError("edge length on the weight's resolution limit: outside this truth's domain")
            if d2 + 1e-6 < 2048:
                nb[a].add(b)
                nb[b].add(a)
    dist = np.where(np.asarray(seeded, bool), 0, -1)
    frontier = [int(v) for v in np.nonzero(dist == 0)[0]]
    rounds = 0
    while frontier:
        nxt = []
        for a in frontier:
            for b in nb[a]:
                if dist[b] < 0:
                    dist[b] = dist[a] + 1
                    nxt.append(b)
        if nxt:
            rounds += 1
        frontier = nxt
    return rounds, dist >= 0


def dilate_truth(tex, mask, iters):
    """Jacobi dilation written per texel: after k steps exactly the texels within Chebyshev distance k of a filled one are
    filled (new ones marked 3), each with the float64 mean of its neighbours filled BEFORE that step.  -> tex float64, mask"""
    tex = np.asarray(tex, np.float64).copy()
    mask = np.asarray(mask, np.uint8).copy()
    T = mask.shape[0]
    for _ in range(iters):
        old_t, old_m = tex.copy(), mask.copy()
        for y in range(T):
            for x in range(T):
                if old_m[y, x]:
                    continue
                nb = [(yy, xx) for yy in range(max(0, y - 1), min(T, y + 2)) for xx in range(max(0, x - 1), min(T, x + 2))
                      if (yy, xx) != (y, x) and old_m[yy, xx]]
                if nb:
                    tex[y, x] = sum(old_t[p] for p in nb) / len(nb)
                    mask[y, x] = 3
    return tex, mask
