"""numpy yardstick of the a-priori LES analysis (include/iamrx.h: iamrx_mf_sgs; iamr_amd/csrc/k_sgs.hip), built from
specop_numpy.filter_reference, np.roll differences and math.fsum, in the notation of specop_numpy.py.

For a velocity f (n_x, n_y, n_z, 3) on a periodic box with side lengths L, the filter (kind, kc), ~ = filter_reference:
  U_i = u_i~, P_ij = fl(u_i u_j)~ (i <= j), tau_ij = P_ij - U_i U_j, k = 0.5 ((tau_xx + tau_yy) + tau_zz),
  A[n][d] = (U_n(x + e_d) - U_n(x - e_d)) (0.5 / dx_d) by np.roll, s_ij = A[i][j] + A[j][i],
  SS = A00^2 + A11^2 + A22^2 + 0.5 (s01^2 + s02^2 + s12^2), |S|^2 = 2 SS,
  Pi = -(((tau_xx A00 + tau_yy A11) + tau_zz A22) + ((tau_xy s01 + tau_xz s02) + tau_yz s12)),
  D_0 = Delta^2 sqrt(2 SS), D_1 = Delta^2 sqrt(0.5 sum_q (2 A_q)^2), P_m = D_m (2 SS), Delta = L_max / (2 kc),
and the 16 means of the header by math.fsum / N.  Every expression is evaluated in the order the header fixes.

The bounds, derived and not tuned.  u = 2^-53; ||.|| is the 2-norm over the cells, max|.| the largest entry of the YARDSTICK's
array, B(f) = specop_numpy.filter_bound(f) the bound on ||device - numpy|| of one filtered component.  Every quantity X of the chain
carries a bound e(X) >= ||X_device - X_numpy||, propagated to first order with the second-order term of a product kept (class Q):
  inputs     e(U_i) = B(u_i).  The product p_ij = fl(u_i u_j) is one correctly rounded IEEE multiplication on both sides, the same bits,
             so e(P_ij) = B(p_ij); 2 u ||p_ij|| is added so that the bound also covers either side against the exact product (the
             Galilean test compares two calls whose products round differently; |G| <= 1 carries the rounding through the filter).
  a + b      e(a) + e(b) + 2 u ||a + b||: each side rounds once, by at most u |a + b|, and the two roundings need not agree.
  a b        max|a| e(b) + max|b| e(a) + e(a) e(b) + 2 u ||a b||   (||da b|| <= max|b| ||da||; ||da db|| <= ||da|| ||db||).
  2^k a      |2^k| e(a), exact.   c a, c not a power of two: |c| e(a) + 4 u ||c a|| (the rounding, and c itself within u on each side).
  sqrt(a)    |sqrt(a + d) - sqrt(a)| = |d| / (sqrt(a + d) + sqrt(a)) <= |d| / sqrt(a) for every d >= -a: e(a) / sqrt(min a) +
             2 u ||sqrt(a)||.  Needs min a > e(a) (a cell's error is at most the 2-norm): cells where 2 SS or 2 A:A is below the bound
             are asserted away.
  min(a, 0)  Lipschitz with constant 1: e(a).
With these
  ||d tau_ij|| <= B(p_ij) + max|U_j| B(u_i) + max|U_i| B(u_j) + B(u_i) B(u_j) + 2 u (||p_ij|| + ||U_i U_j|| + ||tau_ij||),
  ||d A[n][d]|| <= B(u_n) / dx_d + 3 u max|U_n| sqrt(N) / dx_d: the two shifted copies of dU_n each have its norm, times 0.5 / dx_d.
             The rounding: both sides run the same three IEEE operations with the same constant 0.5 / dx_d = 0.5 fl(1 / dx_d) (a product
             with 0.5 is exact), so identical U give identical A; the difference and the product round by at most u |result| on each
             side, a worst case of 4 u max|U_n| / dx_d per cell for the two sides together.  The 3 u of the feature's specification
             is kept: it asks more, and is 1 % of the term in front of it.
  Pi, D_m, P_m and the products under the means follow by the rules above (the product rule with max-norm factors).
A mean of X errs by ||dX|| / sqrt(N) (Cauchy-Schwarz) plus N u <|X|> for the device's fixed-order sum of N terms plus u |<X>| for
the one rounding of math.fsum and the division.  A count (the cells with Pi < 0) is compared exactly; the yardstick first asserts that no
cell has |Pi| <= e(Pi), so that a tie never decides a test."""
import math
import numpy as np
import specop_numpy as SO

U = 2.0 ** -53
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
STAT_NAMES = ("Pi", "Pi2", "Pi_neg", "k_sgs", "S2", "taud2",
              "P_strain", "P2_strain", "PiP_strain", "MM_strain", "LM_strain",
              "P_gradient", "P2_gradient", "PiP_gradient", "MM_gradient", "LM_gradient")
FIELD_NAMES = ("tau_xx", "tau_xy", "tau_xz", "tau_yy", "tau_yz", "tau_zz", "k_sgs", "sgs_flux", "filtered_strain", "smag_flux")


class Q:
    """an array of the yardstick with the bound e >= ||device - yardstick||_2; strict: a root whose argument is not above its bound is an
    assertion error (False: the bound becomes inf, for callers that compare against closed forms only)"""
    strict = True

    def __init__(self, v, e):
        self.v, self.e = v, float(e)

    @property
    def mx(self):
        return float(np.max(np.abs(self.v)))

    def __add__(self, o):
        v = self.v + o.v
        return Q(v, self.e + o.e + 2.0 * U * SO.norm2(v))

    def __sub__(self, o):
        v = self.v - o.v
        return Q(v, self.e + o.e + 2.0 * U * SO.norm2(v))

    def __mul__(self, o):
        v = self.v * o.v
        return Q(v, self.mx * o.e + o.mx * self.e + self.e * o.e + 2.0 * U * SO.norm2(v))

    def __neg__(self):
        return Q(-self.v, self.e)

    def pow2(self, c):
        return Q(self.v * c, abs(c) * self.e)

    def times(self, c):
        v = self.v * c
        return Q(v, abs(c) * self.e + 4.0 * U * SO.norm2(v))

    def sqrt(self):
        v = np.sqrt(self.v)
        lo = float(np.min(self.v))
        if not lo > self.e:
            assert not Q.strict, f"a root's argument {lo:.3e} is not above its bound {self.e:.3e}"
            return Q(v, math.inf)
        return Q(v, self.e / math.sqrt(lo) + 2.0 * U * SO.norm2(v))

    def neg_part(self):
        return Q(np.minimum(self.v, 0.0), self.e)


def delta_of(L, kc):
    return max(float(v) for v in L) / (2.0 * float(kc))


def analyse(f, L, kind, kc, strict=True):
    """f (n_x, n_y, n_z, 3) -> dict: "fields" {name: Q}, "stats" (16,), "stat_bounds" (16,), "counts" (N, cells with Pi < 0), "Pi" (Q)"""
    n = f.shape[:3]
    N = n[0] * n[1] * n[2]
    keep, Q.strict = Q.strict, strict
    try:
        u = [np.ascontiguousarray(f[..., c]) for c in range(3)]
        Uf = [Q(SO.filter_reference(u[c], L, kind, kc), SO.filter_bound(u[c])) for c in range(3)]
        tau = []
        for i, j in PAIRS:
            p = u[i] * u[j]
            tau.append(Q(SO.filter_reference(p, L, kind, kc), SO.filter_bound(p) + 2.0 * U * SO.norm2(p)) - Uf[i] * Uf[j])
        txx, txy, txz, tyy, tyz, tzz = tau
        A = [[None] * 3 for _ in range(3)]
        for c in range(3):
            for d in range(3):
                h = 0.5 / (float(L[d]) / n[d])
                v = (np.roll(Uf[c].v, -1, axis=d) - np.roll(Uf[c].v, 1, axis=d)) * h
                A[c][d] = Q(v, 2.0 * h * Uf[c].e + 3.0 * U * Uf[c].mx * math.sqrt(N) * 2.0 * h)
        ksgs = ((txx + tyy) + tzz).pow2(0.5)
        s01, s02, s12 = A[0][1] + A[1][0], A[0][2] + A[2][0], A[1][2] + A[2][1]
        ss = ((A[0][0] * A[0][0] + A[1][1] * A[1][1]) + A[2][2] * A[2][2]) + ((s01 * s01 + s02 * s02) + s12 * s12).pow2(0.5)
        ss2 = ss.pow2(2.0)
        smag = ss2.sqrt()
        offd = (txy * s01 + txz * s02) + tyz * s12
        Pi = -(((txx * A[0][0] + tyy * A[1][1]) + tzz * A[2][2]) + offd)
        iso = ksgs.times(2.0 / 3.0)
        dxx, dyy, dzz = txx - iso, tyy - iso, tzz - iso
        tdtd = ((dxx * dxx + dyy * dyy) + dzz * dzz) + ((txy * txy + txz * txz) + tyz * tyz).pow2(2.0)
        tds = ((dxx * A[0][0] + dyy * A[1][1]) + dzz * A[2][2]) + offd
        delta = delta_of(L, kc)
        delta2 = delta * delta
        D0 = smag.times(delta2)
        g2 = None
        for c in range(3):
            for d in range(3):
                t = A[c][d].pow2(2.0)
                g2 = t * t if g2 is None else g2 + t * t
        D1 = g2.pow2(0.5).sqrt().times(delta2)
        cols = [Pi, Pi * Pi, Pi.neg_part(), ksgs, ss2, tdtd]
        P = []
        for D in (D0, D1):
            Pm = D * ss2
            P.append(Pm)
            cols += [Pm, Pm * Pm, Pi * Pm, (D * D) * ss2, D * tds]
        stats = np.array([math.fsum(c.v.ravel()) / N for c in cols])
        bounds = np.array([c.e / math.sqrt(N) + N * U * math.fsum(np.abs(c.v).ravel()) / N + U * abs(s) for c, s in zip(cols, stats)])
        fields = dict(zip(FIELD_NAMES, tau + [ksgs, Pi, smag, P[0]]))
        return dict(fields=fields, stats=stats, stat_bounds=bounds, counts=(N, int(np.count_nonzero(Pi.v < 0.0))), Pi=Pi, delta=delta)
    finally:
        Q.strict = keep


def no_tie(a):
    """no cell of Pi within its bound of zero: the count of Pi < 0 is then the device's exactly"""
    return float(np.min(np.abs(a["Pi"].v))) > a["Pi"].e


def ksgs_from_modes(f, L, kind, kc):
    """<k_sgs> by Parseval: 0.5 sum over the three components and all modes of (1 - G^2) |F|^2 (G(0) = 1, so the mean of a filtered field
    is the field's mean and <(u_i u_i)~ - U_i U_i> = <u_i^2> - <U_i^2>)"""
    G = SO.filter_G(f.shape[:3], L, kind, kc)
    t = 0.0
    for c in range(3):
        F = SO.np_fwd(f[..., c])
        t += math.fsum(((1.0 - G * G) * (F.real * F.real + F.imag * F.imag)).ravel())
    return 0.5 * t
