"""Structure functions and two-point correlations along the axes (include/iamrx.h: iamrx_mf_strfn / iamrx_ns_strfn / iamrx_amr_strfn;
kernels in csrc/k_strfn.hip): the calls into the library, the dict the Python layer hands out with what the host derives from the raw
columns, and the text file the driver writes (ns.strfn_interval, inputs.py) with its reader.  Apart from `mf_structure` and
`level_structure` nothing here touches the library.

The raw result is avg[d, c, col, r]: axis d, component c, separation r in cells, and with delta = f(x + r e_d) - f(x) the columns
  0: <f(x) f(x + r e_d)>;  1 .. pmax: <delta^p>;  then one for each odd p <= pmax: <|delta|^p>
each a mean over count[d, r] pairs (periodic axis: all N cells with wrap-around; otherwise the pairs inside the domain).  Entries
beyond an axis's rmax are zero."""
import ctypes as C
import math
import numpy as np

PMAX_MAX, MAX_EXTENT = 8, 1024
COMPONENTS = ("u", "v", "w", "c")


def ncol_of(pmax):
    """1 + pmax + ceil(pmax / 2)"""
    return 1 + int(pmax) + (int(pmax) + 1) // 2


def abs_col(pmax, p):
    """the column of <|delta|^p>, p odd"""
    return 1 + int(pmax) + (int(p) - 1) // 2


def limit_of(n, periodic):
    """the largest separation of an axis of n cells: n / 2 periodic, n - 1 otherwise"""
    return int(n) // 2 if periodic else int(n) - 1


def check_request(pmax, rmax):
    """pmax and rmax as the driver's keys give them -> (pmax, (rx, ry, rz)); ValueError names what is wrong (the limits that depend on
    the extents are the library's to check)"""
    pmax = int(pmax)
    if not 1 <= pmax <= PMAX_MAX:
        raise ValueError(f"strfn: pmax = {pmax} outside 1 .. {PMAX_MAX}")
    if rmax is None:
        rmax = -1
    r = [int(rmax)] * 3 if np.isscalar(rmax) else [int(v) for v in rmax]
    if len(r) == 1:
        r = r * 3
    if len(r) != 3:
        raise ValueError(f"strfn: rmax holds {len(r)} integers, one or three are wanted")
    for d in range(3):
        if r[d] < -1:
            raise ValueError(f"strfn: rmax_{'xyz'[d]} = {r[d]} must be -1 (the largest allowed), 0 (skip the axis) or a number of cells")
    return pmax, tuple(r)


def resolve_rmax(n, periodic, rmax):
    """-1 -> the axis's limit; ValueError names an axis whose request lies beyond it or whose extent is above 1024"""
    out = []
    for d in range(3):
        lim = limit_of(n[d], periodic[d])
        if rmax[d] > lim:
            raise ValueError(f"strfn: rmax_{'xyz'[d]} = {rmax[d]} beyond the axis's limit {lim} (n_{'xyz'[d]} = {n[d]}, "
                             f"{'periodic: n / 2' if periodic[d] else 'not periodic: n - 1'})")
        r = lim if rmax[d] < 0 else rmax[d]
        if r > 0 and n[d] > MAX_EXTENT:
            raise ValueError(f"strfn: extent n_{'xyz'[d]} = {n[d]} above {MAX_EXTENT}")
        out.append(r)
    return tuple(out)


def _geom(geom):
    n = tuple(int(v) for v in geom.n)
    L = tuple(float(geom.prob_hi[d]) - float(geom.prob_lo[d]) for d in range(3))
    return n, L, tuple(int(v) for v in geom.periodic)


def _call(entry, args, geom, ncomp, pmax, rmax):
    from .lib import check
    pmax, rmax = check_request(pmax, rmax)
    n, L, per = _geom(geom)
    # the capacity for the largest request the extents allow; a request beyond it is the library's error, which names the axis
    rcap = 1 + max([limit_of(n[d], per[d]) if rmax[d] < 0 else min(rmax[d], limit_of(n[d], per[d])) for d in range(3)] + [0])
    ncol = ncol_of(pmax)
    out, cnt, mean = np.zeros(3 * ncomp * ncol * rcap), np.zeros(3 * rcap, dtype=np.int64), np.zeros(ncomp)
    check(entry(*args, pmax, (C.c_int * 3)(*rmax), rcap, out.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_longlong)),
                mean.ctypes.data_as(C.POINTER(C.c_double))))
    rm = tuple(limit_of(n[d], per[d]) if rmax[d] < 0 else rmax[d] for d in range(3))
    return raw_dict(out.reshape(3, ncomp, ncol, rcap), cnt.reshape(3, rcap), mean, n, L, per, pmax, rm)


def raw_dict(avg, count, mean, n, L, periodic, pmax, rmax):
    """the raw arrays: "r" (cells), "dx", "count" (3, rcap) int64, "mean" (ncomp,), "n", "L", "periodic", "pmax", "rmax" (resolved, per
    axis) and "avg" (3, ncomp, ncol, rcap)"""
    avg = np.asarray(avg, dtype=np.float64)
    return dict(r=np.arange(avg.shape[3]), dx=tuple(float(L[d]) / int(n[d]) for d in range(3)), count=np.asarray(count, dtype=np.int64).copy(),
                mean=np.asarray(mean, dtype=np.float64).copy(), n=tuple(int(v) for v in n), L=tuple(float(v) for v in L),
                periodic=tuple(int(v) for v in periodic), pmax=int(pmax), rmax=tuple(int(v) for v in rmax), avg=avg.copy())


def mf_structure(geom, mf, comp=0, ncomp=1, pmax=4, rmax=None):
    """iamrx_mf_strfn on components comp .. comp + ncomp - 1 of a cell-centred MultiFab whose boxes tile the domain of geom -> the raw
    dict of raw_dict (no derived entries: the components need not be a velocity).  rmax: None / -1 the largest allowed separation of
    every axis, an integer for all three axes, or three integers (0 skips an axis).  Collective."""
    from .lib import lib
    return _call(lib().iamrx_mf_strfn, (C.byref(geom), mf.h, int(comp), int(ncomp)), geom, int(ncomp), pmax, rmax)


def level_structure(entry, handle, geom, pmax=4, rmax=None):
    """iamrx_ns_strfn / iamrx_amr_strfn (entry: the library's function) on a level or hierarchy handle -> the dict of derive"""
    from .lib import lib
    return derive(_call(entry, (handle,), geom, lib().iamrx_strfn_nq(), pmax, rmax))


def integral_scale(f, dx, rmax):
    """the trapezoid of the correlation coefficient f(r) over r = 0 .. rmax, cut at its first zero crossing (the last, partial interval
    ends where the straight line through its two values meets zero), times dx"""
    total = 0.0
    for r in range(int(rmax)):
        a, b = float(f[r]), float(f[r + 1])
        if not a > 0.0:
            break
        if b > 0.0:
            total += 0.5 * (a + b)
        else:
            total += 0.5 * a * (a / (a - b))
            break
    return total * float(dx)


def derive(s):
    """the raw dict of the four components u, v, w, c -> the same dict plus, per axis d (p = 1 .. pmax; row p = 0 is unused and zero):
      "SL"[d, p, r]   <delta^p> of the velocity component along d (longitudinal)
      "ST"[d, p, r]   the mean of <delta^p> of the other two velocity components (transverse)
      "Sc"[d, p, r]   <delta^p> of the tracer
      "SLabs", "STabs", "Scabs"   the same of <|delta|^p>, filled for the odd p
      "RL", "RT", "Rc"[d, r]      the two-point correlations <f(x) f(x + r e_d)> (RT: the mean of the two transverse ones)
      "f", "g"[d, r]  the correlation coefficients of the fluctuations, f = (RL - m^2) / (RL(0) - m^2) with m the mean of that
                      component, g the same of RT with the mean of the two m^2 (NaN where the variance is zero or the axis is skipped)
      "integral_scale"[d]   integral_scale(f) in length units: the trapezoid of f up to its first zero crossing or rmax_d
      "taylor_scale"[d]     lambda with lambda^2 = u'^2 dx^2 * 2 / S_2^L(1), u'^2 = RL(0) - m^2: the parabola fitted to f at r = 0 and
                            r = dx, since S_2^L(r) = 2 u'^2 (1 - f(r)) and f ~ 1 - r^2 / lambda^2 (NaN for a skipped axis)"""
    avg, pmax, mean = s["avg"], s["pmax"], s["mean"]
    assert avg.shape[1] == len(COMPONENTS)
    rcap = avg.shape[3]
    for k in ("SL", "ST", "Sc", "SLabs", "STabs", "Scabs"):
        s[k] = np.zeros((3, pmax + 1, rcap))
    for k in ("RL", "RT", "Rc"):
        s[k] = np.zeros((3, rcap))
    s["f"], s["g"] = np.full((3, rcap), np.nan), np.full((3, rcap), np.nan)
    s["integral_scale"], s["taylor_scale"] = np.full(3, np.nan), np.full(3, np.nan)
    for d in range(3):
        a, b = [q for q in range(3) if q != d]
        s["RL"][d], s["RT"][d], s["Rc"][d] = avg[d, d, 0], 0.5 * (avg[d, a, 0] + avg[d, b, 0]), avg[d, 3, 0]
        for p in range(1, pmax + 1):
            s["SL"][d, p], s["ST"][d, p], s["Sc"][d, p] = avg[d, d, p], 0.5 * (avg[d, a, p] + avg[d, b, p]), avg[d, 3, p]
            if p % 2:
                q = abs_col(pmax, p)
                s["SLabs"][d, p], s["STabs"][d, p], s["Scabs"][d, p] = avg[d, d, q], 0.5 * (avg[d, a, q] + avg[d, b, q]), avg[d, 3, q]
        rm = s["rmax"][d]
        if rm <= 0:
            continue
        m2L, m2T = mean[d] * mean[d], 0.5 * (mean[a] * mean[a] + mean[b] * mean[b])
        varL, varT = s["RL"][d, 0] - m2L, s["RT"][d, 0] - m2T
        if varL > 0.0:
            s["f"][d, :rm + 1] = (s["RL"][d, :rm + 1] - m2L) / varL
            s["integral_scale"][d] = integral_scale(s["f"][d], s["dx"][d], rm)
            if pmax >= 2 and s["SL"][d, 2, 1] > 0.0:
                s["taylor_scale"][d] = math.sqrt(varL * s["dx"][d] * s["dx"][d] * 2.0 / s["SL"][d, 2, 1])
        if varT > 0.0:
            s["g"][d, :rm + 1] = (s["RT"][d, :rm + 1] - m2T) / varT
    return s


def write_strfn(path, s, step, time):
    """header lines beginning with '#' (step, time, n, L, periodic, pmax, rmax, the components' means, column names), then one line per
    (axis, r), r = 0 .. rmax of every axis that is not skipped: axis r count and the columns of every component, with 17 significant
    digits (a double survives the round trip)"""
    avg = s["avg"]
    nc, ncol = avg.shape[1], avg.shape[2]
    with open(path, "w") as f:
        f.write("# step = %d\n# time = %.17g\n" % (int(step), float(time)))
        f.write("# n = %d %d %d\n" % tuple(s["n"]))
        f.write("# L = %.17g %.17g %.17g\n" % tuple(s["L"]))
        f.write("# periodic = %d %d %d\n" % tuple(s["periodic"]))
        f.write("# pmax = %d\n" % s["pmax"])
        f.write("# rmax = %d %d %d\n" % tuple(s["rmax"]))
        f.write("# mean = " + " ".join("%.17g" % float(v) for v in s["mean"]) + "\n")
        names = ["R"] + [f"S{p}" for p in range(1, s["pmax"] + 1)] + [f"A{p}" for p in range(1, s["pmax"] + 1, 2)]
        f.write("# columns = axis r count " + " ".join(f"{c}:{k}" for c in range(nc) for k in names) + "\n")
        for d in range(3):
            if s["rmax"][d] <= 0:
                continue
            for r in range(s["rmax"][d] + 1):
                f.write("%d %d %d " % (d, r, int(s["count"][d, r])) + " ".join("%.17g" % float(avg[d, c, k, r]) for c in range(nc) for k in range(ncol)) + "\n")


def read_strfn(path):
    """the dict write_strfn was given, bit for bit: the raw arrays from the file, the derived entries formed again from them when the
    file holds the four components of a level, plus "step" and "time" """
    head, rows = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                k, _, v = line[1:].partition("=")
                head[k.strip()] = v.strip()
            elif line.strip():
                rows.append(line.split())
    pmax = int(head["pmax"])
    rmax = tuple(int(v) for v in head["rmax"].split())
    mean = np.array([float(v) for v in head["mean"].split()])
    nc, ncol, rcap = len(mean), ncol_of(pmax), 1 + max(rmax + (0,))
    avg, count = np.zeros((3, nc, ncol, rcap)), np.zeros((3, rcap), dtype=np.int64)
    for row in rows:
        d, r = int(row[0]), int(row[1])
        count[d, r] = int(row[2])
        avg[d, :, :, r] = np.array([float(v) for v in row[3:]]).reshape(nc, ncol)
    s = raw_dict(avg, count, mean, [int(v) for v in head["n"].split()], [float(v) for v in head["L"].split()],
                 [int(v) for v in head["periodic"].split()], pmax, rmax)
    if nc == len(COMPONENTS):
        derive(s)
    s["step"], s["time"] = int(head["step"]), float(head["time"])
    return s
