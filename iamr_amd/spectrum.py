"""Shell-summed power spectra of a triply periodic level (include/iamrx.h: iamrx_mf_spectrum / iamrx_ns_spectrum / iamrx_amr_spectrum;
kernels in csrc/k_spectrum.hip): the number of shells of a geometry, the calls into the library, the dict the Python layer hands out
and the text file the driver writes (ns.spectrum_interval, inputs.py) with its reader.  Apart from `mf_spectrum`, `level_spectrum`
nothing here touches the library."""
import ctypes as C
import math
import numpy as np

COLUMNS = ("E", "Euu", "Evv", "Eww", "Ecc")
MIN_EXTENT, MAX_EXTENT = 4, 1024


def extent_ok(n):
    """a power of two in 4 .. 1024"""
    n = int(n)
    return MIN_EXTENT <= n <= MAX_EXTENT and n & (n - 1) == 0


def ratios(L):
    """r_d = L_max / L_d"""
    Lmax = max(float(v) for v in L)
    return tuple(Lmax / float(v) for v in L)


def nbins_of(n, L):
    """(int)(kappa(-n/2) + 0.5) + 1 with kappa = sqrt((m_x r_x)^2 + (m_y r_y)^2 + (m_z r_z)^2), the squares added left to right"""
    r = ratios(L)
    a = [float(-(int(n[d]) // 2)) * r[d] for d in range(3)]
    return int(math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + 0.5) + 1


def _geom_nL(geom):
    return tuple(int(v) for v in geom.n), tuple(float(geom.prob_hi[d]) - float(geom.prob_lo[d]) for d in range(3))


def mf_spectrum(geom, mf, comp=0, ncomp=1):
    """iamrx_mf_spectrum: (P (ncomp, nbins) float64, count (nbins,) int64) of components comp .. comp + ncomp - 1 of a cell-centred
    MultiFab whose boxes tile the domain of geom.  Collective."""
    from .lib import lib, check
    n, L = _geom_nL(geom)
    cap = nbins_of(n, L) if all(v > 0 for v in L) and all(v > 0 for v in n) else 1
    out, cnt, nb = np.zeros(max(int(ncomp), 1) * cap), np.zeros(cap, dtype=np.int64), C.c_int()
    check(lib().iamrx_mf_spectrum(C.byref(geom), mf.h, int(comp), int(ncomp), cap, out.ctypes.data_as(C.POINTER(C.c_double)),
                                  cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nb)))
    return out[:ncomp * nb.value].reshape(ncomp, nb.value).copy(), cnt[:nb.value].copy()


SLAB_ROW = ("kind", "peer", "box", "lo0", "lo1", "lo2", "hi0", "hi1", "hi2", "off")          # kind: 0 kept, 1 sent, 2 received
SLAB_INFO = ("path", "ranks", "max_image", "per_pass", "sent", "received", "transforms")
SLAB_BENCH_PASSES = ("scatter", "x", "y", "pack_zy", "unpack_zy", "z", "pack_yz", "unpack_yz", "shell_sums", "expand")


def host_slab_plan(geom, boxes, owners, rank, nranks):
    """iamrx_host_spectrum_slab_plan (host only, no device): is the slab-decomposed transform eligible on nranks ranks, and the scatter
    plan of `rank` for the boxes [(lo, hi)] with their owners -> (eligible, reason, rows (n, 10) int64 with the columns SLAB_ROW)"""
    from .lib import lib, check
    nb = len(boxes)
    arr = (C.c_int * (6 * max(nb, 1)))()
    for i, (lo, hi) in enumerate(boxes):
        for d in range(3):
            arr[6 * i + d], arr[6 * i + 3 + d] = int(lo[d]), int(hi[d])
    own = (C.c_int * max(nb, 1))(*[int(o) for o in owners])
    ok, n, why = C.c_int(), C.c_int(), C.create_string_buffer(256)
    f = lib().iamrx_host_spectrum_slab_plan
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    check(f(C.byref(geom), nb, arr, own, int(rank), int(nranks), C.byref(ok), why, 256, 0, None, C.byref(n)))
    rows = np.zeros((n.value, len(SLAB_ROW)), dtype=np.int64)
    check(f(C.byref(geom), nb, arr, own, int(rank), int(nranks), C.byref(ok), why, 256, n.value, rows.ctypes.data_as(C.c_void_p), C.byref(n)))
    return bool(ok.value), why.value.decode(), rows


def slab_info():
    """iamrx_spectrum_slab_info: the last shell-sum call on this rank -> dict with the keys SLAB_INFO (path 0: local or gather, 1: slab)"""
    from .lib import lib, check
    v = (C.c_long * len(SLAB_INFO))()
    check(lib().iamrx_spectrum_slab_info(v))
    return dict(zip(SLAB_INFO, (int(x) for x in v)))


def slab_bench(geom, nranks, reps):
    """iamrx_spectrum_slab_bench: milliseconds (reps, len(SLAB_BENCH_PASSES)) of the kernels one rank of nranks runs for one transform"""
    from .lib import lib, check
    ms = np.zeros((int(reps), len(SLAB_BENCH_PASSES)), dtype=np.float32)
    check(lib().iamrx_spectrum_slab_bench(C.byref(geom), int(nranks), int(reps), ms.ctypes.data_as(C.POINTER(C.c_float))))
    return ms


def level_spectrum(entry, handle, geom):
    """iamrx_ns_spectrum / iamrx_amr_spectrum (entry: the library's function) on a level or hierarchy handle -> the dict of as_dict"""
    from .lib import lib, check
    n, L = _geom_nL(geom)
    cap = nbins_of(n, L) if all(v > 0 for v in L) else 1
    nq = lib().iamrx_spectrum_nq()
    out, cnt, nb = np.zeros(nq * cap), np.zeros(cap, dtype=np.int64), C.c_int()
    check(entry(handle, cap, out.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_long)), C.byref(nb)))
    return as_dict(out[:nq * nb.value].reshape(nq, nb.value), cnt[:nb.value], n, L)


def as_dict(P, count, n, L):
    """the library's four columns P_u, P_v, P_w, P_c (4, nbins) -> {"k": s 2 pi / L_max, "count", "E" = (P_u + P_v + P_w) / 2,
    "Euu" = P_u / 2, "Evv", "Eww", "Ecc" = P_c / 2, "n", "L"}"""
    P = np.asarray(P, dtype=np.float64)
    nb = P.shape[1]
    s = dict(k=np.arange(nb) * (2.0 * math.pi / max(float(v) for v in L)), count=np.asarray(count, dtype=np.int64).copy())
    s["E"] = 0.5 * ((P[0] + P[1]) + P[2])
    s["Euu"], s["Evv"], s["Eww"], s["Ecc"] = 0.5 * P[0], 0.5 * P[1], 0.5 * P[2], 0.5 * P[3]
    s["n"] = tuple(int(v) for v in n)
    s["L"] = tuple(float(v) for v in L)
    return s


def write_spectrum(path, s, step, time):
    """header lines beginning with '#' (step, time, n, L, the sum of E over the shells, column names), then one line per shell:
    s k count E Euu Evv Eww Ecc with 17 significant digits (a double survives the round trip)"""
    with open(path, "w") as f:
        f.write("# step = %d\n# time = %.17g\n" % (int(step), float(time)))
        f.write("# n = %d %d %d\n" % tuple(s["n"]))
        f.write("# L = %.17g %.17g %.17g\n" % tuple(s["L"]))
        f.write("# sum_E = %.17g\n" % math.fsum(s["E"]))
        f.write("# columns = s k count " + " ".join(COLUMNS) + "\n")
        for b in range(len(s["k"])):
            f.write("%d %.17g %d " % (b, float(s["k"][b]), int(s["count"][b])) + " ".join("%.17g" % float(s[c][b]) for c in COLUMNS) + "\n")


def read_spectrum(path):
    """the dict write_spectrum was given (float64 arrays, int64 "count", "n", "L") plus "step", "time" and "sum_E" """
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
    s["step"], s["time"], s["sum_E"] = int(head["step"]), float(head["time"]), float(head["sum_E"])
    return s
