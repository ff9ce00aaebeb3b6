"""numpy yardstick of the shell-summed power spectra (include/iamrx.h: iamrx_mf_spectrum; iamr_amd/csrc/k_spectrum.hip).

For a field f on n = (n_x, n_y, n_z) cells of a periodic domain with side lengths L, N = n_x n_y n_z:
  F = np.fft.fftn(f) / N; the signed mode number of index j along d is j for j < n_d / 2 and j - n_d otherwise;
  kappa = sqrt((m_x r_x)^2 + (m_y r_y)^2 + (m_z r_z)^2) with r_d = L_max / L_d, the squares added left to right in double;
  shell s = (int)(kappa + 0.5); nbins = (int)(kappa(-n/2) + 0.5) + 1; P(s) = math.fsum of |F|^2 over the shell; count(s) its modes.

The bound, derived and not tuned: a radix-2 / radix-4 FFT whose twiddles are good to a couple of ulp has ||dF||_2 <= eps1 ||F||_2 with
eps1 = 8 log2(N) 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, the FFT chapter).  Both sides err (numpy's transform
too), so eps = 2 eps1.  With P(s) = sum |F|^2 over the shell and |F + dF|^2 - |F|^2 = 2 Re(conj(F) dF) + |dF|^2, Cauchy-Schwarz over
the shell gives
  |dP(s)| <= 2 eps sqrt(P(s) P_tot) + eps^2 P_tot + count(s) 2^-53 P(s),
the last term for the summation of count(s) non-negative terms in any order.

A mode whose kappa + 0.5 lies within rounding of an integer could fall into either shell; the yardstick asserts a distance above 1e-9
for every shape it is given, so that a tie can never decide a test."""
import math
import numpy as np

TIE = 1e-9


def mode_numbers(n):
    j = np.arange(int(n))
    return np.where(j < int(n) // 2, j, j - int(n))


def shell_index(n, L):
    """-> (s (n_x, n_y, n_z) int64, nbins, the smallest distance of a kappa + 0.5 to an integer)"""
    Lmax = max(float(v) for v in L)
    r = [Lmax / float(v) for v in L]
    a = [mode_numbers(n[d]).astype(np.float64) * r[d] for d in range(3)]
    ax, ay, az = a[0][:, None, None], a[1][None, :, None], a[2][None, None, :]
    kap = np.sqrt((ax * ax + ay * ay) + az * az)
    t = kap + 0.5
    s = t.astype(np.int64)
    dist = float(np.min(np.minimum(t - np.floor(t), np.floor(t) + 1.0 - t)))
    c = [float(-(int(n[d]) // 2)) * r[d] for d in range(3)]
    nbins = int(math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + 0.5) + 1
    assert dist > TIE, (n, L, dist)
    assert int(s.max()) == nbins - 1
    return s, nbins, dist


def shell_sums(F, s, nbins):
    """math.fsum of |F|^2 per shell -> (P (nbins,), count (nbins,) int64)"""
    p = (F.real * F.real + F.imag * F.imag).ravel()
    order = np.argsort(s.ravel(), kind="stable")
    count = np.bincount(s.ravel(), minlength=nbins).astype(np.int64)
    ends = np.cumsum(count)
    P = np.array([math.fsum(p[order[e - c:e]]) for c, e in zip(count, ends)])
    return P, count


def spectrum_reference(f, L):
    """f: (n_x, n_y, n_z) -> (P (nbins,), count (nbins,))"""
    n = f.shape
    s, nbins, _ = shell_index(n, L)
    return shell_sums(np.fft.fftn(f) / float(f.size), s, nbins)


def eps_of(N):
    return 2.0 * 8.0 * math.log2(N) * 2.0 ** -53


def bound(P, count, N):
    """per shell: 2 eps sqrt(P(s) P_tot) + eps^2 P_tot + count(s) 2^-53 P(s)"""
    eps, Ptot = eps_of(N), math.fsum(P)
    return 2.0 * eps * np.sqrt(P * Ptot) + eps * eps * Ptot + count * 2.0 ** -53 * P


def radix2(f):
    """an independent transform for the CPU check of the bound: in-place radix-2 decimation in time along every axis (bit-reversed
    load, log2 n stages of butterflies (a, c) -> (a + w c, a - w c)), twiddles from numpy's cos / sin -> F = transform / N"""
    F = np.asarray(f, dtype=np.complex128)
    for ax in range(3):
        n = F.shape[ax]
        ln = n.bit_length() - 1
        assert 1 << ln == n
        rev = np.array([int(format(e, f"0{ln}b")[::-1], 2) for e in range(n)])
        A = np.moveaxis(F, ax, 0)[rev].copy()
        q = np.arange(n // 2)
        tw = np.cos(2.0 * np.pi * q / n) - 1j * np.sin(2.0 * np.pi * q / n)
        for stg in range(ln):
            h = 1 << stg
            b = np.arange(n // 2)
            pos = b & (h - 1)
            i0 = ((b >> stg) << (stg + 1)) + pos
            w = tw[pos << (ln - 1 - stg)].reshape((-1,) + (1,) * (A.ndim - 1))
            a, c = A[i0].copy(), A[i0 + h] * w
            A[i0], A[i0 + h] = a + c, a - c
        F = np.moveaxis(A, 0, ax)
    return F / float(f.size)


def noise(n, seed, ncomp=1):
    """white noise of order one with a mean of its own per component -> (n_x, n_y, n_z, ncomp)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(tuple(n) + (ncomp,)) + (0.3 + 0.2 * np.arange(ncomp))


def cosine_mode(n, m=(3, 4, 0)):
    """cos(2 pi (m . x / n)) at the cell indices: amplitude 1, P = 1/4 at +m and at -m, both in the shell of |m|"""
    i, j, k = np.meshgrid(*(np.arange(v) for v in n), indexing="ij")
    return np.cos(2.0 * np.pi * (m[0] * i / n[0] + m[1] * j / n[1] + m[2] * k / n[2]))


# the shapes of the GPU tests: (n, L)
SHAPES = (((8, 16, 32), (1.0, 1.0, 1.0)), ((16, 16, 32), (1.0, 1.0, 2.0)), ((32, 32, 32), (1.0, 1.0, 1.0)),
          ((1024, 4, 4), (1.0, 1.0, 1.0)), ((4, 1024, 4), (1.0, 1.0, 1.0)), ((4, 4, 1024), (1.0, 1.0, 1.0)),
          ((64, 4, 4), (1.0, 1.0, 1.0)), ((4, 64, 4), (1.0, 1.0, 1.0)), ((16, 16, 16), (1.0, 1.0, 1.0)))
