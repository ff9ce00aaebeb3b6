"""Histograms and probability density functions of state and derived fields (include/iamrx.h: iamrx_mf_histogram / iamrx_ns_histogram /
iamrx_amr_histogram and the joint forms; kernel in csrc/k_hist.hip): the calls into the library, the automatic range, the dict the Python
layer hands out and the text file the driver writes (ns.pdf_interval, inputs.py) with its reader.

The binning rule of the library, per column with lo < hi and inv = nbins / (hi - lo): NaN -> `nan`, v < lo -> `below`, v > hi -> `above`,
otherwise bin min(int((v - lo) * inv), nbins - 1).  The counts are integers and exact."""
import ctypes as C
import numpy as np

STATE_NAMES = ("x_velocity", "y_velocity", "z_velocity", "density", "tracer")
# the derived fields of the velocity-gradient tensor (csrc/k_velgrad.hip), in the order of the library's quantity ids
VELGRAD_NAMES = ("diveru", "vort_x", "vort_y", "vort_z", "enstrophy", "strain_rate", "dissipation", "q_criterion", "r_invariant", "helicity")
# of these a two-dimensional run (on its y-periodic slab) knows the ones that do not name a direction or need the third one
VELGRAD_NAMES_2D = ("diveru", "enstrophy", "strain_rate", "dissipation", "q_criterion")
DERIVED_NAMES = ("energy", "mag_vort", "avg_pressure") + VELGRAD_NAMES
NBINS_MAX, SLOTS2_MAX = 4096, 16384


def known_names(do_trac2=False, do_temp=False):
    """the names a run with these switches knows, in the library's order"""
    return STATE_NAMES + (("tracer2",) if do_trac2 else ()) + (("temp",) if do_temp else ()) + DERIVED_NAMES


def state_comp(name, do_trac2=False, do_temp=False):
    """state component of a plotfile name, None for a derived quantity or an unknown name"""
    names = STATE_NAMES + (("tracer2",) if do_trac2 else ()) + (("temp",) if do_temp else ())
    return names.index(name) if name in names else None


def edges_of(lo, hi, nbins):
    """lo + (hi - lo) * arange(nbins + 1) / nbins"""
    return float(lo) + (float(hi) - float(lo)) * np.arange(int(nbins) + 1) / int(nbins)


def widen(lo, hi):
    """numpy's rule for an empty range: lo == hi -> (lo - 0.5, hi + 0.5)"""
    lo, hi = float(lo), float(hi)
    return (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _ranges(n, range):
    """range: one (lo, hi) pair for every column, or one pair per column -> (lo (n,), hi (n,))"""
    r = np.asarray(range, dtype=np.float64)
    if r.shape == (2,):
        r = np.tile(r, (n, 1))
    if r.shape != (n, 2):
        raise ValueError(f"histogram: range must hold one (lo, hi) pair per name ({n}), got shape {r.shape}")
    return np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])


def field_minmax(run, name):
    """(smallest, largest) value of a named field over the valid cells of all levels of a level or hierarchy (iamrx_mf_minmax on the
    state or on what derive(name) forms).  Collective."""
    mn, mx = np.inf, -np.inf
    for lev in run.levels:
        comp = state_comp(name, bool(lev.params.do_trac2), bool(lev.params.do_temp))
        a, b = lev.data(lev.S_NEW).minmax(comp, 0) if comp is not None else lev.derive(name).minmax(0, 0)
        mn, mx = min(mn, a), max(mx, b)
    return mn, mx


def mf_histogram(mf, comp=0, ncomp=1, nbins=64, range=None, cov=None, weight=1):
    """iamrx_mf_histogram: int64 (ncomp, nbins + 3) of components comp .. comp + ncomp - 1 of a cell-centred MultiFab: per column the
    bins, then below, above, nan.  range: (lo, hi) for all columns or one pair per column (required).  Collective."""
    from .lib import lib, check
    lo, hi = _ranges(max(int(ncomp), 1), range)
    counts = np.zeros((max(int(ncomp), 1), max(int(nbins), 0) + 3), dtype=np.int64)
    check(lib().iamrx_mf_histogram(mf.h, int(comp), int(ncomp), None if cov is None else cov.h, _dp(lo), _dp(hi), int(nbins),
                                   C.c_longlong(int(weight)), _lp(counts)))
    return counts


def mf_histogram2(mf, compx, compy, nbins=(32, 32), range=None, cov=None, weight=1):
    """iamrx_mf_histogram2: (int64 (nbx, nby), outside) of the pair of components; range = ((xlo, xhi), (ylo, yhi)).  Collective."""
    from .lib import lib, check
    lo, hi = _ranges(2, range)
    nb = (C.c_int * 2)(int(nbins[0]), int(nbins[1]))
    ok = 1 <= nb[0] and 1 <= nb[1] and nb[0] * nb[1] <= SLOTS2_MAX
    counts = np.zeros(nb[0] * nb[1] + 1 if ok else 1, dtype=np.int64)
    check(lib().iamrx_mf_histogram2(mf.h, int(compx), int(compy), None if cov is None else cov.h, _dp(lo), _dp(hi), nb, C.c_longlong(int(weight)), _lp(counts)))
    return counts[:-1].reshape(nb[0], nb[1]).copy(), int(counts[-1])


def as_dict(names, counts, lo, hi):
    """the library's counts (n, nbins + 3) -> {"names", "nbins", "range" (n, 2), "edges" (n, nbins + 1), "counts" (n, nbins) int64,
    "below", "above", "nan" (n,) int64, "total" (n,) int64 = all slots, "pdf" (n, nbins) = counts / (counts.sum() * binwidth)}"""
    counts = np.asarray(counts, dtype=np.int64)
    n, nbins = counts.shape[0], counts.shape[1] - 3
    h = dict(names=tuple(names), nbins=nbins, range=np.stack([np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)], axis=1))
    h["edges"] = np.stack([edges_of(lo[q], hi[q], nbins) for q in np.arange(n)])
    h["counts"] = counts[:, :nbins].copy()
    h["below"], h["above"], h["nan"] = counts[:, nbins].copy(), counts[:, nbins + 1].copy(), counts[:, nbins + 2].copy()
    h["total"] = counts.sum(axis=1)
    h["pdf"] = pdf_of(h["counts"], h["range"])
    return h


def pdf_of(counts, range):
    """counts / (counts.sum() * binwidth) per column; a column without a counted cell is all zero"""
    counts = np.asarray(counts, dtype=np.int64)
    out = np.zeros(counts.shape)
    for q in np.arange(counts.shape[0]):
        s = int(counts[q].sum())
        if s > 0:
            out[q] = counts[q] / (s * ((float(range[q][1]) - float(range[q][0])) / counts.shape[1]))
    return out


def histogram(run, entry, names, nbins=64, range=None):
    """iamrx_ns_histogram / iamrx_amr_histogram (entry: the library's function) on a level or hierarchy -> the dict of as_dict.
    range None: each field's minimum and maximum over the valid cells of all levels (widened by numpy's rule when they coincide)."""
    from .lib import check
    names = [names] if isinstance(names, str) else list(names)
    n = len(names)
    if range is None:
        mm = [widen(*field_minmax(run, nm)) for nm in names]
        lo, hi = np.array([m[0] for m in mm], dtype=np.float64), np.array([m[1] for m in mm], dtype=np.float64)
    else:
        lo, hi = _ranges(max(n, 1), range)
    arr = (C.c_char_p * max(n, 1))(*[nm.encode() for nm in names])
    counts = np.zeros((max(n, 1), max(int(nbins), 0) + 3), dtype=np.int64)
    check(entry(run.h, n, arr, _dp(lo), _dp(hi), int(nbins), _lp(counts)))
    return as_dict(names, counts, lo, hi)


def histogram2(run, entry, namex, namey, nbins=(32, 32), range=None):
    """iamrx_ns_histogram2 / iamrx_amr_histogram2 -> {"names" (namex, namey), "nbins" (nbx, nby), "range" (2, 2), "xedges", "yedges",
    "counts" (nbx, nby) int64, "outside", "total", "pdf" = counts / (counts.sum() * bin area)}"""
    from .lib import check
    if range is None:
        mm = [widen(*field_minmax(run, nm)) for nm in (namex, namey)]
        lo, hi = np.array([m[0] for m in mm], dtype=np.float64), np.array([m[1] for m in mm], dtype=np.float64)
    else:
        lo, hi = _ranges(2, range)
    nb = (C.c_int * 2)(int(nbins[0]), int(nbins[1]))
    ok = 1 <= nb[0] and 1 <= nb[1] and nb[0] * nb[1] <= SLOTS2_MAX
    counts = np.zeros(nb[0] * nb[1] + 1 if ok else 1, dtype=np.int64)
    check(entry(run.h, namex.encode(), namey.encode(), _dp(lo), _dp(hi), nb, _lp(counts)))
    c = counts[:-1].reshape(nb[0], nb[1]).copy()
    h = dict(names=(namex, namey), nbins=(nb[0], nb[1]), range=np.stack([lo, hi], axis=1), xedges=edges_of(lo[0], hi[0], nb[0]),
             yedges=edges_of(lo[1], hi[1], nb[1]), counts=c, outside=int(counts[-1]), total=int(counts.sum()))
    s = int(c.sum())
    h["pdf"] = c / (s * ((hi[0] - lo[0]) / nb[0]) * ((hi[1] - lo[1]) / nb[1])) if s > 0 else np.zeros(c.shape)
    return h


def write_pdf(path, h, step, time):
    """header lines beginning with '#' (step, time, nbins, and per field its name, range and the slots below, above, nan, total), the
    column names, then one line per bin: the bin index and per field lo_edge hi_edge count pdf.  Integers as integers, reals with 17
    significant digits: the round trip is exact."""
    n, nbins = len(h["names"]), int(h["nbins"])
    with open(path, "w") as f:
        f.write("# step = %d\n# time = %.17g\n# nbins = %d\n" % (int(step), float(time), nbins))
        f.write("# names = " + " ".join(h["names"]) + "\n")
        for q in range(n):
            f.write("# field %s = %.17g %.17g %d %d %d %d\n" % (h["names"][q], float(h["range"][q][0]), float(h["range"][q][1]), int(h["below"][q]),
                                                               int(h["above"][q]), int(h["nan"][q]), int(h["total"][q])))
        f.write("# columns = bin " + " ".join(f"{nm}:lo {nm}:hi {nm}:count {nm}:pdf" for nm in h["names"]) + "\n")
        for b in range(nbins):
            f.write("%d " % b + " ".join("%.17g %.17g %d %.17g" % (float(h["edges"][q][b]), float(h["edges"][q][b + 1]), int(h["counts"][q][b]),
                                                                  float(h["pdf"][q][b])) for q in range(n)) + "\n")


def read_pdf(path):
    """the dict write_pdf was given (as_dict's keys, the same dtypes) plus "step" and "time" """
    head, fields, rows = {}, [], []
    with open(path) as f:
        for line in f:
            if line.startswith("# field "):
                k, _, v = line[len("# field "):].partition("=")
                fields.append((k.strip(), v.split()))
            elif line.startswith("#"):
                k, _, v = line[1:].partition("=")
                head[k.strip()] = v.strip()
            elif line.strip():
                rows.append(line.split())
    names, nbins = tuple(head["names"].split()), int(head["nbins"])
    n = len(names)
    assert tuple(k for k, _ in fields) == names and len(rows) == nbins
    h = dict(names=names, nbins=nbins, step=int(head["step"]), time=float(head["time"]))
    h["range"] = np.array([[float(v[0]), float(v[1])] for _, v in fields], dtype=np.float64).reshape(n, 2)
    for q, key in ((2, "below"), (3, "above"), (4, "nan"), (5, "total")):
        h[key] = np.array([int(v[q]) for _, v in fields], dtype=np.int64)
    h["edges"] = np.array([[float(r[1 + 4 * q]) for r in rows] + [float(rows[-1][2 + 4 * q])] for q in range(n)], dtype=np.float64).reshape(n, nbins + 1)
    h["counts"] = np.array([[int(r[3 + 4 * q]) for r in rows] for q in range(n)], dtype=np.int64).reshape(n, nbins)
    h["pdf"] = np.array([[float(r[4 + 4 * q]) for r in rows] for q in range(n)], dtype=np.float64).reshape(n, nbins)
    return h
