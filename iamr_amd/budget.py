"""Co-spectra and the spectral kinetic-energy budget dE(k)/dt = T(k) - D(k) + F(k) of a triply periodic level (include/iamrx.h:
iamrx_mf_cospectrum / iamrx_mf_spectrum_k2 / iamrx_ns_spectral_budget / iamrx_amr_spectral_budget; kernels in csrc/k_spectrum.hip and
csrc/k_convect.hip): the calls into the library, the dict the Python layer hands out and the text file the driver writes
(ns.budget_interval, inputs.py) with its reader.  The shells, their wavenumbers and the counts are those of spectrum.py."""
import ctypes as C
import math
import numpy as np

from .spectrum import nbins_of, _geom_nL

COLUMNS = ("E", "T", "Pi", "D", "F")


def _cap(geom):
    n, L = _geom_nL(geom)
    return (nbins_of(n, L) if all(v > 0 for v in L) and all(v > 0 for v in n) else 1), n, L


def mf_cospectrum(geom, a, b, acomp=0, bcomp=0):
    """iamrx_mf_cospectrum: (C_ab, P_a, P_b, count) per shell of component acomp of a and bcomp of b, cell-centred MultiFabs that each
    tile the domain of geom (the same array or different box layouts are fine).  Collective."""
    from .lib import lib, check
    cap, _, _ = _cap(geom)
    out, cnt, nb = np.zeros(3 * cap), np.zeros(cap, dtype=np.int64), C.c_int()
    check(lib().iamrx_mf_cospectrum(C.byref(geom), a.h, int(acomp), b.h, int(bcomp), cap, out.ctypes.data_as(C.POINTER(C.c_double)),
                                    cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nb)))
    o = out[:3 * nb.value].reshape(3, nb.value)
    return o[0].copy(), o[1].copy(), o[2].copy(), cnt[:nb.value].copy()


def mf_spectrum_k2(geom, mf, comp=0, ncomp=1):
    """iamrx_mf_spectrum_k2: W (ncomp, nbins), the k^2-weighted power of components comp .. comp + ncomp - 1 (the spectral |grad f|^2).
    Collective."""
    from .lib import lib, check
    cap, _, _ = _cap(geom)
    out, nb = np.zeros(max(int(ncomp), 1) * cap), C.c_int()
    check(lib().iamrx_mf_spectrum_k2(C.byref(geom), mf.h, int(comp), int(ncomp), cap, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nb)))
    return out[:ncomp * nb.value].reshape(ncomp, nb.value).copy()


def level_budget(entry, handle, geom, visc_coef):
    """iamrx_ns_spectral_budget / iamrx_amr_spectral_budget (entry: the library's function) on a level or hierarchy handle -> as_dict"""
    from .lib import lib, check
    cap, n, L = _cap(geom)
    nq = lib().iamrx_budget_nq()
    out, cnt, nb = np.zeros(nq * cap), np.zeros(cap, dtype=np.int64), C.c_int()
    check(entry(handle, cap, out.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nb)))
    return as_dict(out[:nq * nb.value].reshape(nq, nb.value), cnt[:nb.value], n, L, visc_coef)


def as_dict(cols, count, n, L, visc_coef):
    """the library's four columns E, T, D, F (4, nbins) -> {"k": s 2 pi / L_max, "count", "E", "T", "Pi" = -(T(0) + ... + T(s)) added
    left to right, "D", "F", "n", "L", "visc_coef"}"""
    cols = np.asarray(cols, dtype=np.float64)
    nb = cols.shape[1]
    s = dict(k=np.arange(nb) * (2.0 * math.pi / max(float(v) for v in L)), count=np.asarray(count, dtype=np.int64).copy())
    s["E"], s["T"], s["D"], s["F"] = cols[0].copy(), cols[1].copy(), cols[2].copy(), cols[3].copy()
    s["Pi"] = -np.cumsum(s["T"])
    s["n"] = tuple(int(v) for v in n)
    s["L"] = tuple(float(v) for v in L)
    s["visc_coef"] = float(visc_coef)
    return s


def write_budget(path, s, step, time):
    """header lines beginning with '#' (step, time, n, L, visc_coef, the sums of T, D and F over the shells, column names), then one line
    per shell: s k count E T Pi D F with 17 significant digits (a double survives the round trip)"""
    with open(path, "w") as f:
        f.write("# step = %d\n# time = %.17g\n" % (int(step), float(time)))
        f.write("# n = %d %d %d\n" % tuple(s["n"]))
        f.write("# L = %.17g %.17g %.17g\n" % tuple(s["L"]))
        f.write("# visc_coef = %.17g\n" % float(s["visc_coef"]))
        for c in ("T", "D", "F"):
            f.write("# sum_%s = %.17g\n" % (c, math.fsum(s[c])))
        f.write("# columns = s k count " + " ".join(COLUMNS) + "\n")
        for b in range(len(s["k"])):
            f.write("%d %.17g %d " % (b, float(s["k"][b]), int(s["count"][b])) + " ".join("%.17g" % float(s[c][b]) for c in COLUMNS) + "\n")


def read_budget(path):
    """the dict write_budget was given (float64 arrays, int64 "count", "n", "L", "visc_coef") plus "step", "time", "sum_T", "sum_D", "sum_F" """
    head, rows = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                k, _, v = line[1:].partition("=")
                head[k.strip()] = v.strip()
            elif line.strip():
                rows.append(line.split())
    cols = head["columns"].split()
    s = {}
    for q, c in enumerate(cols):
        if c == "s":
            continue
        s[c] = np.array([int(r[q]) for r in rows], dtype=np.int64) if c == "count" else np.array([float(r[q]) for r in rows], dtype=np.float64)
    s["n"] = tuple(int(v) for v in head["n"].split())
    s["L"] = tuple(float(v) for v in head["L"].split())
    s["step"], s["time"], s["visc_coef"] = int(head["step"]), float(head["time"]), float(head["visc_coef"])
    for c in ("T", "D", "F"):
        s["sum_" + c] = float(head["sum_" + c])
    return s
