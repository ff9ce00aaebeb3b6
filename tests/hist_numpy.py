"""numpy restatement of the histograms (include/iamrx.h: iamrx_mf_histogram / iamrx_amr_histogram; iamr_amd/csrc/k_hist.hip) on explicit
per-level arrays and box lists.

The binning rule, per column with lo < hi finite and inv = nbins / (hi - lo) formed once in double:
  NaN -> slot `nan`; v < lo -> slot `below`; v > hi -> slot `above`; otherwise bin min(int((v - lo) * inv), nbins - 1).
numpy forms v - lo and the product as two separate IEEE operations and astype(int64) truncates towards zero, as the kernel's conversion
does, so the restatement is exact: every comparison with it is equality of integers.

Composite weighting: levels 0 .. F with ratio 2; level l counts the cells it has and level l + 1 does not cover, each with the weight
8^(F - l): the slots are in units of finest-level cell volumes and together sum to cells(level 0) * 8^F."""
import numpy as np
from profile_numpy import box_mask, counted_masks  # noqa: F401  (the same masks as the profiles' restatement)


def slots_of(v, lo, hi, nbins):
    """slot index of every value of v: 0 .. nbins - 1 the bins, nbins below, nbins + 1 above, nbins + 2 nan"""
    v = np.asarray(v, dtype=np.float64)
    lo, hi, nbins = np.float64(lo), np.float64(hi), int(nbins)
    assert np.isfinite(lo) and np.isfinite(hi) and lo < hi and 1 <= nbins <= 4096
    inv = np.float64(nbins) / (hi - lo)
    s = np.full(v.shape, nbins + 2, dtype=np.int64)
    ok = ~np.isnan(v)
    s[ok & (v < lo)] = nbins
    s[ok & (v > hi)] = nbins + 1
    inside = ok & (v >= lo) & (v <= hi)
    with np.errstate(invalid="ignore", over="ignore"):
        b = ((v[inside] - lo) * inv).astype(np.int64)
    s[inside] = np.minimum(b, nbins - 1)
    return s


def hist1(v, lo, hi, nbins, weight=1):
    """int64 (nbins + 3,): the bins, below, above, nan of the values v, each counting `weight`"""
    return np.bincount(slots_of(v, lo, hi, nbins).ravel(), minlength=int(nbins) + 3).astype(np.int64) * int(weight)


def hist2(x, y, lo, hi, nbins, weight=1):
    """(int64 (nbx, nby), outside): a pair that is NaN or out of range on either axis goes to `outside`"""
    nbx, nby = int(nbins[0]), int(nbins[1])
    assert nbx * nby <= 16384
    sx, sy = slots_of(x, lo[0], hi[0], nbx).ravel(), slots_of(y, lo[1], hi[1], nby).ravel()
    inside = (sx < nbx) & (sy < nby)
    c = np.bincount(sx[inside] * nby + sy[inside], minlength=nbx * nby).astype(np.int64).reshape(nbx, nby) * int(weight)
    return c, int((~inside).sum()) * int(weight)


def hist_reference(fields, boxes, n0, lo, hi, nbins):
    """fields[l]: (n0 * 2^l, ncol) array over the whole index space of level l (what lies outside the level's boxes or under a finer level
    is never read); boxes[l]: [(lo, hi), ...] of level l; lo, hi: per column.  -> int64 (ncol, nbins + 3) composite counts"""
    F = len(fields) - 1
    counted = counted_masks(boxes, n0)
    ncol = fields[0].shape[-1]
    out = np.zeros((ncol, int(nbins) + 3), dtype=np.int64)
    for l in range(F + 1):
        for q in range(ncol):
            out[q] += hist1(fields[l][..., q][counted[l]], lo[q], hi[q], nbins, 8 ** (F - l))
    return out


def hist2_reference(fx, fy, boxes, n0, lo, hi, nbins):
    """fx[l], fy[l]: (n0 * 2^l) arrays -> (int64 (nbx, nby), outside) composite"""
    F = len(fx) - 1
    counted = counted_masks(boxes, n0)
    c, o = np.zeros((int(nbins[0]), int(nbins[1])), dtype=np.int64), 0
    for l in range(F + 1):
        cl, ol = hist2(fx[l][counted[l]], fy[l][counted[l]], lo, hi, nbins, 8 ** (F - l))
        c += cl
        o += ol
    return c, o
