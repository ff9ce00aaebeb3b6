"""numpy yardstick of the structure functions and two-point correlations along the axes (include/iamrx.h: iamrx_mf_strfn;
iamr_amd/csrc/k_strfn.hip).

For a field f on n = (n_x, n_y, n_z) cells, an axis d and a separation of r cells the pairs are
  periodic axis      f and np.roll(f, -r, axis=d): all N cells, count = N (also at r = n_d / 2, where every unordered pair is met twice);
  non-periodic axis  f[..., :n_d - r, ...] and f[..., r:, ...]: the pairs inside the domain, count = (n_d - r) N / n_d;
with delta = f(x + r e_d) - f(x) the columns are
  0: f(x) f(x + r e_d);  1 .. pmax: delta^p (successive multiplication in double, term by term);  then |delta|^p for the odd p <= pmax
and every column is math.fsum over the pairs -- the exactly rounded sum of the terms -- divided by count.

The bound used by every test, derived and not measured: a column is a mean of K = count terms t_k.  A term of delta^p carries at most
p roundings (one subtraction, p - 1 multiplications; the product of column 0 one) on either side, device and yardstick.  A sum of K
terms in ANY order carries at most K - 1 roundings (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: the error of
recursive and tree summation alike is bounded by gamma_{K-1} sum |t_k|); one division follows.  Hence
  |got - ref| <= gamma_m mean|t_k|,   m = K + 2 p + 2,   gamma_m = m u / (1 - m u),   u = 2^-53.
Contracting a multiplication and an addition into a fused one only removes roundings.  The yardstick's own error is the u of its
single division (counted in the + 2).  No measured constant enters."""
import math
import numpy as np

U = 2.0 ** -53


def ncol_of(pmax):
    return 1 + pmax + (pmax + 1) // 2


def col_power(pmax, col):
    """the p of the bound for a column: 1 for the product, p for delta^p and |delta|^p"""
    if col == 0:
        return 1
    return col if col <= pmax else 2 * (col - 1 - pmax) + 1


def limit_of(n, periodic):
    return n // 2 if periodic else n - 1


def resolve(n, periodic, rmax):
    return tuple(limit_of(n[d], periodic[d]) if rmax[d] < 0 else rmax[d] for d in range(3))


def count_of(n, periodic, d, r):
    N = n[0] * n[1] * n[2]
    return N if periodic[d] else (n[d] - r) * (N // n[d])


def pairs(f, d, r, periodic):
    """(f(x), f(x + r e_d)) over the pairs of axis d at separation r, each an array"""
    if periodic:
        return f, np.roll(f, -r, axis=d)
    lo, hi = [slice(None)] * f.ndim, [slice(None)] * f.ndim
    lo[d], hi[d] = slice(0, f.shape[d] - r), slice(r, f.shape[d])
    return f[tuple(lo)], f[tuple(hi)]


def terms(a, b, pmax):
    """the ncol arrays of terms of one (axis, r)"""
    d = b - a
    out, w, powers = [a * b], d, []
    for p in range(1, pmax + 1):
        if p > 1:
            w = w * d
        powers.append(w)
    out += powers
    out += [np.abs(powers[p - 1]) for p in range(1, pmax + 1, 2)]
    return out


def reference(f, periodic, pmax=4, rmax=(-1, -1, -1)):
    """f: (n_x, n_y, n_z) -> (avg (3, ncol, rcap), count (3, rcap) int64, meanabs (3, ncol, rcap), mean): avg the fsum means, meanabs the
    mean of |t_k| of every column (what the bound scales with), mean = fsum(f) / N; zero beyond an axis's rmax and on a skipped axis"""
    n = f.shape
    rm = resolve(n, periodic, rmax)
    ncol, rcap = ncol_of(pmax), 1 + max(rm + (0,))
    avg, meanabs, count = np.zeros((3, ncol, rcap)), np.zeros((3, ncol, rcap)), np.zeros((3, rcap), dtype=np.int64)
    for d in range(3):
        if rm[d] <= 0:
            continue
        for r in range(rm[d] + 1):
            a, b = pairs(f, d, r, periodic[d])
            K = count_of(n, periodic, d, r)
            assert a.size == K
            count[d, r] = K
            for c, t in enumerate(terms(a, b, pmax)):
                avg[d, c, r] = math.fsum(t.ravel().tolist()) / K
                meanabs[d, c, r] = float(np.mean(np.abs(t)))
    return avg, count, meanabs, math.fsum(f.ravel().tolist()) / f.size


def gamma(m):
    return m * U / (1.0 - m * U)


def mean_bound(f):
    """the same reasoning for <f>: N terms without a rounding of their own, N - 1 roundings of the sum, one division on either side"""
    return gamma(f.size + 1.0) * float(np.mean(np.abs(f)))


def bound(count, meanabs, pmax):
    """gamma_{K + 2 p + 2} mean|t_k| per (axis, column, r); 0 where nothing was computed"""
    bd = np.zeros_like(meanabs)
    for c in range(meanabs.shape[1]):
        m = count.astype(np.float64) + 2.0 * col_power(pmax, c) + 2.0
        bd[:, c, :] = gamma(m) * meanabs[:, c, :]
    return bd


def noise(n, seed, ncomp=1):
    """white noise of order one with a mean of its own per component -> (n_x, n_y, n_z, ncomp)"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(tuple(n) + (ncomp,)) + (0.3 + 0.2 * np.arange(ncomp))


def cosine(n, d, m):
    """cos(2 pi m i_d / n_d): along a periodic axis d  R(r) = cos(2 pi m r / n_d) / 2, <delta^2> = 1 - cos(2 pi m r / n_d), <delta^3> = 0"""
    shape = [1, 1, 1]
    shape[d] = n[d]
    return np.broadcast_to(np.cos(2.0 * np.pi * m * np.arange(n[d]) / n[d]).reshape(shape), n).copy()


def linear(n, d):
    """4 i_d: along a non-periodic axis d every delta is 4 r, so <delta^p> = (4 r)^p exactly"""
    shape = [1, 1, 1]
    shape[d] = n[d]
    return np.broadcast_to((4.0 * np.arange(n[d])).reshape(shape), n).copy()
