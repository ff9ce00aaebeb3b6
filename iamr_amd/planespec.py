"""Plane spectra: ring-summed 2-D spectra along a wall-normal axis, E(k_h; z) (include/iamrx.h: iamrx_mf_plane_spectrum /
iamrx_mf_plane_cospectrum / iamrx_ns_plane_spectrum / iamrx_amr_plane_spectrum; kernels in csrc/k_spectrum.hip): the number of rings of a
geometry, the calls into the library, the dict the Python layer hands out and the text file the driver writes
(ns.plane_spectrum_interval, inputs.py) with its reader.  Only the two directions in the plane must be periodic with power-of-two
extents; the normal direction may have walls and any extent."""
import ctypes as C
import math
import numpy as np

COLUMNS = ("E", "Euu", "Evv", "Eww", "Err", "Ecc")
AXIS = "xyz"


def axes_of(dir):
    """the two transformed axes a < b of the normal axis dir"""
    dir = int(dir)
    if not 0 <= dir <= 2:
        raise ValueError(f"plane_spectrum: dir = {dir} outside 0 .. 2")
    return (1 if dir == 0 else 0), (1 if dir == 2 else 2)


def nrings_of(n, L, dir):
    """(int)(kappa(-n_a/2, -n_b/2) + 0.5) + 1 with kappa = sqrt((m_a r_a)^2 + (m_b r_b)^2), r = max(L_a, L_b) / L, the squares added left to
    right; the normal axis does not enter"""
    a, b = axes_of(dir)
    L2 = max(float(L[a]), float(L[b]))
    ca, cb = float(-(int(n[a]) // 2)) * (L2 / float(L[a])), float(-(int(n[b]) // 2)) * (L2 / float(L[b]))
    return int(math.sqrt(ca * ca + cb * cb) + 0.5) + 1


def refusal(n, periodic, dir, ndim=3):
    """why a run with these cells and periodic flags cannot take plane spectra along dir, in the library's wording, or None"""
    from .spectrum import extent_ok
    if int(ndim) != 3:
        return "a two-dimensional run: the plane spectra are three-dimensional only"
    if not 0 <= int(dir) <= 2:
        return f"dir = {int(dir)} outside 0 .. 2"
    a, b = axes_of(dir)
    for d in (a, b):
        if not int(periodic[d]):
            return f"direction {AXIS[d]} is not periodic (the two directions in the planes normal to {AXIS[int(dir)]} must be)"
    for d in (a, b):
        if not extent_ok(n[d]):
            return f"extent n_{AXIS[d]} = {int(n[d])} is not a power of two in 4 .. 1024"
    return None


def _caps(geom, dir):
    from .spectrum import _geom_nL
    n, L = _geom_nL(geom)
    ok = 0 <= int(dir) <= 2 and all(v > 0 for v in L) and all(v > 0 for v in n)
    return n, L, (int(n[int(dir)]) if ok else 1), (nrings_of(n, L, dir) if ok else 1)


def mf_plane_spectrum(geom, mf, dir, comp=0, ncomp=1):
    """iamrx_mf_plane_spectrum: (P (ncomp, nplanes, nrings) float64, count (nrings,) int64) of components comp .. comp + ncomp - 1 of a
    cell-centred MultiFab whose boxes tile the domain of geom.  Collective."""
    from .lib import lib, check
    _, _, pc, rc = _caps(geom, dir)
    out, cnt, npl, nr = np.zeros(max(int(ncomp), 1) * pc * rc), np.zeros(rc, dtype=np.int64), C.c_int(), C.c_int()
    check(lib().iamrx_mf_plane_spectrum(C.byref(geom), mf.h, int(comp), int(ncomp), int(dir), pc, rc, out.ctypes.data_as(C.POINTER(C.c_double)),
                                        cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(npl), C.byref(nr)))
    return out[:ncomp * npl.value * nr.value].reshape(ncomp, npl.value, nr.value).copy(), cnt[:nr.value].copy()


def mf_plane_cospectrum(geom, a, b, dir, acomp=0, bcomp=0):
    """iamrx_mf_plane_cospectrum: (C_ab, P_a, P_b, each (nplanes, nrings), count (nrings,)) of component acomp of a and bcomp of b,
    cell-centred MultiFabs that each tile the domain of geom (one packed transform).  Collective."""
    from .lib import lib, check
    _, _, pc, rc = _caps(geom, dir)
    out, cnt, npl, nr = np.zeros(3 * pc * rc), np.zeros(rc, dtype=np.int64), C.c_int(), C.c_int()
    check(lib().iamrx_mf_plane_cospectrum(C.byref(geom), a.h, int(acomp), b.h, int(bcomp), int(dir), pc, rc, out.ctypes.data_as(C.POINTER(C.c_double)),
                                          cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(npl), C.byref(nr)))
    o = out[:3 * npl.value * nr.value].reshape(3, npl.value, nr.value)
    return o[0].copy(), o[1].copy(), o[2].copy(), cnt[:nr.value].copy()


def plane_spectrum_bench(geom, mf, dir, comp=0, reps=1):
    """iamrx_plane_spectrum_bench: milliseconds (reps, 4) of pack, the two transform passes and the ring sums of one component"""
    from .lib import lib, check
    ms = np.zeros((int(reps), 4), dtype=np.float32)
    check(lib().iamrx_plane_spectrum_bench(C.byref(geom), mf.h, int(comp), int(dir), int(reps), ms.ctypes.data_as(C.POINTER(C.c_float))))
    return ms


def coord_of(geom, dir, nplanes):
    """the plane centres along dir in physical units"""
    lo, hi = float(geom.prob_lo[dir]), float(geom.prob_hi[dir])
    return lo + (np.arange(nplanes) + 0.5) * ((hi - lo) / nplanes)


def level_plane_spectrum(entry, handle, geom, dir):
    """iamrx_ns_plane_spectrum / iamrx_amr_plane_spectrum (entry: the library's function) on a level or hierarchy handle -> the dict of
    as_dict"""
    from .lib import lib, check
    n, L, pc, rc = _caps(geom, dir)
    nq = lib().iamrx_plane_spectrum_nq()
    out, cnt, npl, nr = np.zeros(nq * pc * rc), np.zeros(rc, dtype=np.int64), C.c_int(), C.c_int()
    check(entry(handle, int(dir), pc, rc, out.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(npl), C.byref(nr)))
    P = out[:nq * npl.value * nr.value].reshape(nq, npl.value, nr.value)
    return as_dict(P, cnt[:nr.value], n, L, dir, coord_of(geom, int(dir), npl.value))


def as_dict(P, count, n, L, dir, coord):
    """the library's five columns P_u, P_v, P_w, P_rho, P_c (5, nplanes, nrings) -> {"k": s 2 pi / L2, "count", "coord" (plane centres),
    "dir", "n", "L", and the arrays (nplanes, nrings) "E" = (P_u + P_v + P_w) / 2, "Euu" = P_u / 2, "Evv", "Eww", "Err" = P_rho / 2,
    "Ecc" = P_c / 2}"""
    P = np.asarray(P, dtype=np.float64)
    a, b = axes_of(dir)
    nr = P.shape[2]
    s = dict(k=np.arange(nr) * (2.0 * math.pi / max(float(L[a]), float(L[b]))), count=np.asarray(count, dtype=np.int64).copy(),
             coord=np.asarray(coord, dtype=np.float64).copy(), dir=int(dir))
    s["E"] = 0.5 * ((P[0] + P[1]) + P[2])
    s["Euu"], s["Evv"], s["Eww"], s["Err"], s["Ecc"] = 0.5 * P[0], 0.5 * P[1], 0.5 * P[2], 0.5 * P[3], 0.5 * P[4]
    s["n"] = tuple(int(v) for v in n)
    s["L"] = tuple(float(v) for v in L)
    return s


def write_plane_spectrum(path, s, step, time):
    """header lines beginning with '#' as write_spectrum's (step, time, n, L, the sum of E, column names) plus dir and nplanes, then one
    line per (plane, ring): p coord s k count E Euu Evv Eww Err Ecc with 17 significant digits (a double survives the round trip)"""
    npl, nr = s["E"].shape
    with open(path, "w") as f:
        f.write("# step = %d\n# time = %.17g\n" % (int(step), float(time)))
        f.write("# n = %d %d %d\n" % tuple(s["n"]))
        f.write("# L = %.17g %.17g %.17g\n" % tuple(s["L"]))
        f.write("# dir = %d\n# nplanes = %d\n" % (int(s["dir"]), npl))
        f.write("# sum_E = %.17g\n" % math.fsum(s["E"].ravel()))
        f.write("# columns = p coord s k count " + " ".join(COLUMNS) + "\n")
        for p in range(npl):
            for b in range(nr):
                f.write("%d %.17g %d %.17g %d " % (p, float(s["coord"][p]), b, float(s["k"][b]), int(s["count"][b]))
                        + " ".join("%.17g" % float(s[c][p, b]) for c in COLUMNS) + "\n")


def read_plane_spectrum(path):
    """the dict write_plane_spectrum was given (float64 arrays, int64 "count", "dir", "n", "L") plus "step", "time" and "sum_E" """
    head, rows = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                k, _, v = line[1:].partition("=")
                head[k.strip()] = v.strip()
            elif line.strip():
                rows.append(line.split())
    cols = head["columns"].split()
    npl = int(head["nplanes"])
    nr = len(rows) // npl if npl else 0
    assert npl * nr == len(rows), (path, npl, len(rows))
    q = {c: i for i, c in enumerate(cols)}
    s = dict(dir=int(head["dir"]))
    s["coord"] = np.array([float(rows[p * nr][q["coord"]]) for p in range(npl)], dtype=np.float64)
    s["k"] = np.array([float(r[q["k"]]) for r in rows[:nr]], dtype=np.float64)
    s["count"] = np.array([int(r[q["count"]]) for r in rows[:nr]], dtype=np.int64)
    for c in COLUMNS:
        s[c] = np.array([float(r[q[c]]) for r in rows], dtype=np.float64).reshape(npl, nr)
    s["n"] = tuple(int(v) for v in head["n"].split())
    s["L"] = tuple(float(v) for v in head["L"].split())
    s["step"], s["time"], s["sum_E"] = int(head["step"]), float(head["time"]), float(head["sum_E"])
    return s
