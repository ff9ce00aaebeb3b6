"""Histograms (csrc/k_hist.hip): what one costs, against the integrated-quantity reduction that reads the same data.
  python tools/bench_hist.py [n] [out.txt]
On one n^3 box (default 256) and on the same cells cut into eight boxes it times, in this one process and on the same arrays:
  - iamrx_hist_bench (HIP events around the launches of one histogram, nothing read back) for one and five columns with 64 and 1024
    bins and for the joint 64 x 64 histogram of two columns,
  - reduce_sum_integrated through iamrx_ns_sum_integrated, the yardstick: one pass over the same five state components (events around
    the call, which ends in its read-back),
for three fields: a TaylorGreen state (smooth), uniform random values, a constant (every cell in one bin).  The cases alternate inside
every repeat; warm-up first, then the median of the repeats with their minimum and maximum.  Each case is reported as a ratio to the
yardstick and as a fraction of the 8 TB/s HBM peak on the compulsory traffic, 8 B per cell and column.  Then a (n/2)^3 time step
followed by the five state histograms with the automatic range (what ns.pdf_interval = 1 does) against the step alone.
Writes the table (default profiles/hist_bench.txt)."""
import ctypes as C
import os
import statistics
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N

HBM_PEAK = 8.0e12
WARM, REPS, STEPS = 3, 30, 6
lib.init(0)
nn = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "hist_bench.txt")
hip = C.CDLL("libamdhip64.so")
stream = C.c_void_p(lib.lib().iamrx_stream())
lines = []
NAMES5 = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer"]


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def hipcheck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def event_ms(fn, e0, e1):
    hipcheck(hip.hipEventRecord(e0, stream))
    fn()
    hipcheck(hip.hipEventRecord(e1, stream))
    hipcheck(hip.hipEventSynchronize(e1))
    t = C.c_float()
    hipcheck(hip.hipEventElapsedTime(C.byref(t), e0, e1))
    return t.value


def hist_ms(mf, ncol, lo, hi, nbins, nby=0):
    """one iamrx_hist_bench repeat: milliseconds between the two events around the launches"""
    ms = (C.c_float * 1)()
    lo, hi = np.ascontiguousarray(lo[:ncol], dtype=np.float64), np.ascontiguousarray(hi[:ncol], dtype=np.float64)
    lib.check(lib.lib().iamrx_hist_bench(mf.h, 0, ncol, None, lo.ctypes.data_as(C.POINTER(C.c_double)), hi.ctypes.data_as(C.POINTER(C.c_double)),
                                         int(nbins), int(nby), 1, ms))
    return ms[0]


def med(v):
    return statistics.median(v), min(v), max(v)


def population(tag, lay, g):
    """the three fields on one layout: every case and the yardstick on the same state, alternating"""
    n = g.n
    cells = float(n[0]) * n[1] * n[2]
    ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
    e0, e1 = C.c_void_p(), C.c_void_p()
    hipcheck(hip.hipEventCreate(C.byref(e0))); hipcheck(hip.hipEventCreate(C.byref(e1)))
    rng = np.random.default_rng(1)
    summary = {}
    for field in ("taylorgreen", "random", "constant"):
        if field == "taylorgreen":
            ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
        else:
            mf = lib.MultiFab(lay, lib.CELL, 5, 1)
            if field == "constant":
                mf.setval(0.5)
            else:
                for li in range(mf.nlocal()):
                    glo, ghi = mf.fab_box(li)
                    mf.from_numpy(rng.uniform(0.0, 1.0, size=tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (5,)), li)
            ns.set_data(ns.S_NEW, mf)
            del mf
        S = ns.data(ns.S_NEW)
        mm = [S.minmax(q, 0) for q in range(5)]
        lo = np.array([a - 0.5 if a == b else a for a, b in mm]) if field == "taylorgreen" else np.zeros(5)
        hi = np.array([b + 0.5 if a == b else b for a, b in mm]) if field == "taylorgreen" else np.ones(5)
        cases = [(f"{c} column{'s' if c > 1 else ' '} x {nb:4d} bins", c, nb, 0) for c in (1, 5) for nb in (64, 1024)] + [("joint 64 x 64        ", 2, 64, 64)]
        t = {name: [] for name, _, _, _ in cases}
        yard = []
        for r in range(WARM + REPS):
            y = event_ms(ns.sum_integrated, e0, e1)
            if r >= WARM:
                yard.append(y)
            for name, c, nb, nby in cases:
                ms = hist_ms(S, c, lo, hi, nb, nby)
                if r >= WARM:
                    t[name].append(ms)
        y = med(yard)
        say(f"  {tag}, {field}")
        say(f"    {'sum_integrated (yardstick)':28s} {y[0]:8.4f} ms (min {y[1]:.4f}, max {y[2]:.4f})  {40.0 * cells / (y[0] * 1e-3) / 1e12:5.2f} TB/s = {100 * 40.0 * cells / (y[0] * 1e-3) / HBM_PEAK:4.1f} % of peak")
        for name, c, nb, nby in cases:
            m = med(t[name])
            nbytes = 8.0 * c * cells
            say(f"    {name:28s} {m[0]:8.4f} ms (min {m[1]:.4f}, max {m[2]:.4f})  {nbytes / (m[0] * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (m[0] * 1e-3) / HBM_PEAK:4.1f} % of peak"
                f"  x{m[0] / y[0]:.2f} of the yardstick")
            summary[(field, name)] = m[0]
        del S
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    for name in sorted({k[1] for k in summary}):
        c, r_, s = summary[("constant", name)], summary[("random", name)], summary[("taylorgreen", name)]
        say(f"    {name:28s} constant / random = {c / r_:.2f}, smooth / random = {s / r_:.2f}" + ("   FINDING: the constant field costs more than the random one" if c > r_ else ""))
    del ns


def steps(step, extra):
    """median ms of a synchronised step alone and of a step followed by extra(), alternating"""
    a, b = [], []
    for _ in range(STEPS):
        for dst, more in ((a, None), (b, extra)):
            lib.sync(); t0 = time.perf_counter()
            step()
            if more:
                more()
            lib.sync(); dst.append((time.perf_counter() - t0) * 1e3)
    return med(a), med(b)


say(f"histograms, {nn}^3: {WARM} warm-up rounds, median of {REPS} alternating repeats; compulsory traffic = 8 B per cell and column (yardstick: 40 B per cell)")
n = (nn,) * 3
g = lib.Geom.make(n)
population(f"one {nn}^3 box", lib.Layout.single(n), g)
population(f"eight {nn // 2}^3 boxes", lib.Layout.decompose(n, nn // 2), g)

h = nn // 2
say(f"time step, {h}^3, TaylorGreen")
ns = N.NavierStokes(lib.Geom.make((h,) * 3), lib.Layout.single((h,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
ns.post_init()
for _ in range(2):
    ns.step()
alone, with_h = steps(ns.step, lambda: ns.histogram(NAMES5, 64))
say(f"  step alone {alone[0]:.3f} ms (min {alone[1]:.3f}, max {alone[2]:.3f}); step + five histograms with the automatic range {with_h[0]:.3f} ms "
    f"(min {with_h[1]:.3f}, max {with_h[2]:.3f}): {100 * (with_h[0] / alone[0] - 1):+.2f} %")
fixed = [(-1.5, 1.5)] * 3 + [(0.5, 1.5), (-0.5, 1.5)]
alone, with_h = steps(ns.step, lambda: ns.histogram(NAMES5, 64, fixed))
say(f"  step alone {alone[0]:.3f} ms (min {alone[1]:.3f}, max {alone[2]:.3f}); step + five histograms with a given range {with_h[0]:.3f} ms "
    f"(min {with_h[1]:.3f}, max {with_h[2]:.3f}): {100 * (with_h[0] / alone[0] - 1):+.2f} %")
del ns
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
