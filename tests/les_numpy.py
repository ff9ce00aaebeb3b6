"""The yardstick of the LES tests: a numpy restatement, array at a time, of the two eddy-viscosity models of NavierStokesBase::calc_mut_LES
(reference Source/NS_LES.cpp:114-211) and of the face gradients they are fed with (the tensor operator's: two-point normal difference,
four-point means of the transverse differences).  Written from the reference text in this file's own words; used as model(grads(padded
velocity)).  g[..., 3 n + e] = d u_n / d x_e -- both models are invariant under transposing the gradient, so the order is immaterial."""
import numpy as np

SMAGORINSKY, SIGMA = 0, 1


def grads(P, dx):
    """P: (nx + 2, ny + 2, nz + 2, 3), the velocity with one ghost layer (corner cells are never read).  Returns the three face arrays
    g[D] of shape (n + e_D) + (9,): every D-face of the box, the one at hi + 1 included."""
    n = [P.shape[d] - 2 for d in range(3)]
    inv = [1.0 / dx[d] for d in range(3)]
    out = []
    for D in range(3):
        def C(off):
            sl = []
            for d in range(3):
                cnt = n[d] + (1 if d == D else 0)
                sl.append(slice(1 + off[d], 1 + off[d] + cnt))
            return P[tuple(sl)]

        def o(**kw):
            v = [0, 0, 0]
            for k, q in kw.items():
                v[int(k[1])] = q
            return v
        g = np.empty(tuple(n[d] + (1 if d == D else 0) for d in range(3)) + (9,))
        for e in range(3):
            if e == D:
                d_ = (C([0, 0, 0]) - C([-1 if q == D else 0 for q in range(3)])) * inv[D]
            else:
                pp = [1 if q == e else 0 for q in range(3)]
                mp = [1 if q == e else (-1 if q == D else 0) for q in range(3)]
                pm = [-1 if q == e else 0 for q in range(3)]
                mm = [-1 if q == e else (-1 if q == D else 0) for q in range(3)]
                d_ = (C(pp) + C(mp) - C(pm) - C(mm)) * (0.25 * inv[e])
            for c in range(3):
                g[..., 3 * c + e] = d_[..., c]
        out.append(g)
    return out


def smagorinsky(g, fac):
    """fac (Cs Delta)^2.  The reference doubles every gradient component ("symij = src + src"); it does not form the symmetric part."""
    s = np.zeros(g.shape[:-1])
    for q in range(9):
        sym = g[..., q] + g[..., q]
        s = s + sym * sym
    s = 0.5 * s
    return fac * np.sqrt(s)


def sigma(g, fac, with_s1=False):
    a = [g[..., q] for q in range(9)]
    G11 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    G12 = a[0] * a[3] + a[1] * a[4] + a[2] * a[5]
    G13 = a[0] * a[6] + a[1] * a[7] + a[2] * a[8]
    G22 = a[3] * a[3] + a[4] * a[4] + a[5] * a[5]
    G23 = a[3] * a[6] + a[4] * a[7] + a[5] * a[8]
    G33 = a[6] * a[6] + a[7] * a[7] + a[8] * a[8]
    I1 = G11 + G22 + G33
    I2 = G11 * G22 - G12 * G12 + G22 * G33 - G23 * G23 + G11 * G33 - G13 * G13
    I3 = G11 * (G22 * G33 - G23 * G23) - G12 * (G33 * G12 - G13 * G23) + G13 * (G12 * G23 - G13 * G22)
    t = I1 / 3
    alpha1 = np.maximum(0., t * t - I2 / 3)
    zero = alpha1 == 0.
    a1 = np.where(zero, 1.0, alpha1)
    alpha2 = t * t * t - I1 * I2 / 6 + I3 / 2
    arg = (alpha2 * np.sqrt(1 / a1)) / a1
    arg = np.where(arg > 1., 1., np.where(arg < -1., -1., arg))
    alpha3 = np.arccos(arg) / 3
    s1 = np.sqrt(np.maximum(0., t + 2 * np.sqrt(a1) * np.cos(alpha3)))
    s2 = np.sqrt(np.maximum(0., t - 2 * np.sqrt(a1) * np.cos(np.pi / 3 + alpha3)))
    s3 = np.sqrt(np.maximum(0., t - 2 * np.sqrt(a1) * np.cos(np.pi / 3 - alpha3)))
    s2 = np.maximum(s3, s2)
    s1 = np.maximum(s2, s1)
    s1 = np.maximum(1.e-24, s1)
    mu = np.where(zero, 0., fac * ((s3 * (s1 - s2) * (s2 - s3)) / (s1 * s1)))
    if with_s1:
        return mu, np.where(zero, 0., s1)
    return mu


def model(which, g, fac, **kw):
    return smagorinsky(g, fac) if which == SMAGORINSKY else sigma(g, fac, **kw)


def mu_faces(which, P, dx, Cs, base=0.0):
    """the three face arrays base + mu_t of the padded velocity P (filter width dx[D] on a D-face)"""
    G = grads(P, dx)
    return [base + model(which, G[D], (Cs * dx[D]) * (Cs * dx[D])) for D in range(3)]


def sigma_scale(P, dx, Cs):
    """(Cs Delta)^2 sigma_1 on every face: the scale of the Sigma tolerances"""
    G = grads(P, dx)
    return [(Cs * dx[D]) * (Cs * dx[D]) * sigma(G[D], 1.0, with_s1=True)[1] for D in range(3)]


def ulp_diff(a, b):
    """distance in units in the last place between two float64 arrays of one sign pattern"""
    ia = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(ia - ib)
