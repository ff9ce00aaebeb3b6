"""numpy yardstick of the plane spectra (include/iamrx.h: iamrx_mf_plane_spectrum / iamrx_mf_plane_cospectrum; iamr_amd/csrc/k_spectrum.hip).

For a field f on n = (n_x, n_y, n_z) cells, a normal axis dir and the other two axes a < b, M = n_a n_b:
  F_p = np.fft.fftn(f, axes=(a, b)) / M, plane by plane (the normal axis is not transformed);
  signed mode numbers as spectrum_numpy.mode_numbers; L2 = max(L_a, L_b), r = L2 / L (the normal length does not enter);
  kappa = sqrt((m_a r_a)^2 + (m_b r_b)^2), the squares added left to right in double; ring s = (int)(kappa + 0.5);
  nrings = (int)(kappa(-n_a/2, -n_b/2) + 0.5) + 1; P(p, s) = math.fsum of |F_p|^2 over the ring; count(s) its modes, the same in every plane.

The bound, derived as in spectrum_numpy's docstring with M in place of N and the plane's own total P_tot(p) = sum_s P(p, s): the two
transforms along a and b act on each plane by itself, so ||dF_p||_2 <= eps ||F_p||_2 with eps = 2 * 8 log2(M) 2^-53, and
  |dP(p, s)| <= 2 eps sqrt(P(p, s) P_tot(p)) + eps^2 P_tot(p) + count(s) 2^-53 P(p, s).
Co-spectrum: the bound of cospectrum_numpy restated per plane,
  |dC(p, s)| <= eps sqrt((P_a + P_b)(p, s) (Pt_a + Pt_b)(p)) + eps^2 (Pt_a + Pt_b)(p) / 2 + count(s) 2^-53 (P_a + P_b)(p, s) / 2.

A mode whose kappa + 0.5 lies within rounding of an integer could fall into either ring; the yardstick asserts a distance above 1e-9
for every shape it is given."""
import math
import numpy as np
import spectrum_numpy as SN

TIE = SN.TIE
U = 2.0 ** -53


def axes_of(dir):
    return (1 if dir == 0 else 0), (1 if dir == 2 else 2)


def ring_index(n, L, dir):
    """-> (s (n_a, n_b) int64, nrings, the smallest distance of a kappa + 0.5 to an integer)"""
    a, b = axes_of(dir)
    L2 = max(float(L[a]), float(L[b]))
    ra, rb = L2 / float(L[a]), L2 / float(L[b])
    xa = (SN.mode_numbers(n[a]).astype(np.float64) * ra)[:, None]
    xb = (SN.mode_numbers(n[b]).astype(np.float64) * rb)[None, :]
    t = np.sqrt(xa * xa + xb * xb) + 0.5
    s = t.astype(np.int64)
    dist = float(np.min(np.minimum(t - np.floor(t), np.floor(t) + 1.0 - t)))
    ca, cb = float(-(int(n[a]) // 2)) * ra, float(-(int(n[b]) // 2)) * rb
    nrings = int(math.sqrt(ca * ca + cb * cb) + 0.5) + 1
    assert dist > TIE, (n, L, dir, dist)
    assert int(s.max()) == nrings - 1
    return s, nrings, dist


def _planes(F, dir):
    """F (n_x, n_y, n_z) -> (nplanes, n_a, n_b)"""
    return np.moveaxis(F, dir, 0)


def ring_sums(V, s, nrings):
    """V (nplanes, n_a, n_b) real -> (math.fsum per (plane, ring) (nplanes, nrings), count (nrings,) int64)"""
    order = np.argsort(s.ravel(), kind="stable")
    count = np.bincount(s.ravel(), minlength=nrings).astype(np.int64)
    ends = np.cumsum(count)
    out = np.zeros((V.shape[0], nrings))
    for p in range(V.shape[0]):
        v = V[p].ravel()
        out[p] = [math.fsum(v[order[e - c:e]]) for c, e in zip(count, ends)]
    return out, count


def transform(f, dir):
    a, b = axes_of(dir)
    return np.fft.fftn(f, axes=(a, b)) / float(f.shape[a] * f.shape[b])


def radix2(f, dir):
    """the independent radix-2 transform of spectrum_numpy.radix2 along the two axes of the plane alone -> F / M"""
    a, b = axes_of(dir)
    F = np.asarray(f, dtype=np.complex128)
    for p in range(f.shape[dir]):
        sl = [slice(None)] * 3
        sl[dir] = slice(p, p + 1)
        # a plane as a 3-D array whose normal extent is 1: radix2 transforms an axis of length 1 trivially and divides by the plane's size
        F[tuple(sl)] = SN.radix2(np.asarray(f[tuple(sl)], dtype=np.complex128))
    return F


def power_from(F, n, L, dir):
    s, nrings, _ = ring_index(n, L, dir)
    Fp = _planes(F, dir)
    return ring_sums(Fp.real * Fp.real + Fp.imag * Fp.imag, s, nrings)


def plane_spectrum_reference(f, L, dir):
    """f (n_x, n_y, n_z) -> (P (nplanes, nrings), count (nrings,))"""
    return power_from(transform(f, dir), f.shape, L, dir)


def eps_of(M):
    return 2.0 * 8.0 * math.log2(M) * U


def bound(P, count, M):
    """per plane and ring: 2 eps sqrt(P(p, s) P_tot(p)) + eps^2 P_tot(p) + count(s) 2^-53 P(p, s)"""
    eps = eps_of(M)
    Ptot = np.array([math.fsum(row) for row in P])[:, None]
    return 2.0 * eps * np.sqrt(P * Ptot) + eps * eps * Ptot + count[None, :] * U * P


def plane_cospectrum_reference(fa, fb, L, dir):
    """-> (C, P_a, P_b (nplanes, nrings), count) from two plain transforms"""
    s, nrings, _ = ring_index(fa.shape, L, dir)
    Fa, Fb = _planes(transform(fa, dir), dir), _planes(transform(fb, dir), dir)
    C, count = ring_sums((Fa * np.conj(Fb)).real, s, nrings)
    Pa, _ = ring_sums(Fa.real * Fa.real + Fa.imag * Fa.imag, s, nrings)
    Pb, _ = ring_sums(Fb.real * Fb.real + Fb.imag * Fb.imag, s, nrings)
    return C, Pa, Pb, count


def cospectrum_bound(Pa, Pb, count, M):
    eps = eps_of(M)
    Pt = (np.array([math.fsum(r) for r in Pa]) + np.array([math.fsum(r) for r in Pb]))[:, None]
    return eps * np.sqrt((Pa + Pb) * Pt) + eps * eps * Pt / 2.0 + count[None, :] * U * (Pa + Pb) / 2.0


def noise(n, seed, ncomp=1):
    return SN.noise(n, seed, ncomp)


def cosine_planes(n, dir, amp, m=(3, 4)):
    """f = A(p) cos(2 pi (m_a x_a / n_a + m_b x_b / n_b)) with amplitude amp[p] in plane p: P(p, |m|) = A(p)^2 / 2"""
    a, b = axes_of(dir)
    idx = np.meshgrid(*(np.arange(v) for v in n), indexing="ij")
    return np.asarray(amp, dtype=np.float64)[idx[dir]] * np.cos(2.0 * np.pi * (m[0] * idx[a] / n[a] + m[1] * idx[b] / n[b]))


# the shapes of the GPU tests: (n, L, dir)
U3 = (1.0, 1.0, 1.0)
SHAPES = (((8, 16, 6), U3, 2), ((16, 8, 3), (2.0, 1.0, 1.5), 2), ((1024, 4, 2), U3, 2), ((4, 1024, 2), U3, 2), ((64, 4, 1), U3, 2),
          ((8, 6, 16), U3, 1), ((1024, 2, 4), U3, 1), ((4, 3, 1024), (1.0, 5.0, 2.0), 1),
          ((6, 8, 16), U3, 0), ((3, 16, 8), (0.7, 1.0, 2.0), 0), ((2, 1024, 4), U3, 0), ((2, 4, 1024), U3, 0), ((96, 4, 4), U3, 0),
          ((65, 8, 8), U3, 0), ((1, 4, 4), U3, 0))
