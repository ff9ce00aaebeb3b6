"""numpy restatement of the plane-averaged profiles (include/iamrx.h: iamrx_amr_plane_profile; iamr_amd/csrc/k_profile.hip) on explicit
per-level arrays and box lists.

Levels 0 .. F with ratio 2, an axis `dir` and a bin level B: nbins = n_dir(level 0) * 2^B slabs of the index space of level B, one cell
thick.  The value of quantity q in a bin is the volume-weighted mean of q over the cells that no finer level covers and that meet the
slab: a cell of level l >= B lies in bin index >> (l - B) with its own volume, a cell of level l < B counts in each of the 2^(B - l) bins
it spans with volume / 2^(B - l).

The reference is exact up to two roundings per bin: cell volume over slab volume is 1 / (cells of the level in a plane * planes per bin),
so with the common denominator D = (cells of the FINEST level in a plane) * 2^(F - min(B, F)) every cell's weight is an integer power of
two m_l over D; the terms q * m_l are exact, math.fsum adds them exactly (one rounding) and the division by D rounds once more.

The error bound of a computed mean: a sum of N terms formed in any order is within (N - 1) 2^-53 sum |term| of the exact sum (first
order); per bin that is less than N * 2^-52 * mean |q| (N = counted cells of the bin), which leaves room for the one rounding of the
weight 1 / (cells in a plane), for the addition of the levels and for the two roundings of this reference."""
import math
import numpy as np

NAMES = ("one", "u", "v", "w", "rho", "c", "uu", "vv", "ww", "uv", "uw", "vw", "rhorho", "cc")


def quantities(S):
    """(..., 5) state u v w rho c -> (..., 14) in the order of NAMES; the products are the IEEE products the kernel forms"""
    u, v, w, r, c = (S[..., q] for q in range(5))
    return np.stack([np.ones_like(u), u, v, w, r, c, u * u, v * v, w * w, u * v, u * w, v * w, r * r, c * c], axis=-1)


def box_mask(boxes, n):
    m = np.zeros(tuple(n), dtype=bool)
    for lo, hi in boxes:
        m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    return m


def counted_masks(boxes, n0):
    """per level: the cells the level has and the next finer level does not cover"""
    F = len(boxes) - 1
    have = [box_mask(boxes[l], [v << l for v in n0]) for l in range(F + 1)]
    out = []
    for l in range(F + 1):
        m = have[l].copy()
        if l < F:
            m &= ~have[l + 1][::2, ::2, ::2]          # (proper nesting: a coarse cell is covered entirely or not at all)
        out.append(m)
    return out


def profile_reference(states, boxes, n0, dir, B):
    """states[l]: (n0 * 2^l, 5) array over the whole index space of level l (what lies outside the level's boxes or under a finer level
    is never read); boxes[l]: [(lo, hi), ...] of level l.  -> (mean (14, nbins), N (nbins,) counted cells per bin, meanabs (14, nbins))"""
    F = len(states) - 1
    assert 0 <= B <= F and dir in (0, 1, 2)
    nbins = n0[dir] << B
    counted = counted_masks(boxes, n0)
    perp = lambda l: int(np.prod([n0[d] << l for d in range(3) if d != dir]))
    D = perp(F) << (F - B)
    terms = [[[] for _ in range(nbins)] for _ in range(len(NAMES))]
    N = np.zeros(nbins, dtype=np.int64)
    for l in range(F + 1):
        Q = quantities(states[l][counted[l]])                      # (counted cells, 14)
        at = np.argwhere(counted[l])[:, dir]                        # their index along dir
        m = D // (perp(l) << max(l - B, 0))
        assert m * (perp(l) << max(l - B, 0)) == D and m & (m - 1) == 0       # an exact power-of-two weight
        for b in range(nbins):
            sel = at >> (l - B) == b if l >= B else at == b >> (B - l)           # fold (finer than the bins) or spread (coarser)
            if not sel.any():
                continue
            vals = Q[sel] * float(m)
            N[b] += vals.shape[0]
            for q in range(len(NAMES)):
                terms[q][b].append(vals[:, q])
    mean = np.zeros((len(NAMES), nbins))
    meanabs = np.zeros((len(NAMES), nbins))
    for q in range(len(NAMES)):
        for b in range(nbins):
            t = np.concatenate(terms[q][b]) if terms[q][b] else np.zeros(0)
            mean[q, b] = math.fsum(t) / D if not np.isnan(t).any() else np.nan
            meanabs[q, b] = math.fsum(np.abs(t)) / D if not np.isnan(t).any() else np.nan
    return mean, N, meanabs


def bound(N, meanabs):
    """N * 2^-52 * mean |q| per (quantity, bin)"""
    return N[None, :] * 2.0 ** -52 * meanabs
