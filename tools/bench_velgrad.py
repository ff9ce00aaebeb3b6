"""Velocity-gradient derived fields (csrc/k_velgrad.hip): what one pass costs in its two forms, against derive_mag_vort on the same arrays.
  python tools/bench_velgrad.py [n] [out.txt]
On one n^3 box (default 256) and on the same cells cut into eight boxes, for a TaylorGreen and a random velocity (one ghost layer, filled),
it times in this one process and on the same arrays:
  - iamrx_velgrad_bench (HIP events around the launches, nothing read back) with 1, 3 and 10 outputs in the marching form (path 1) and
    the plain form (path 2), and ten single-output launches against the one ten-output launch,
  - iamrx_derive_mag_vort, the yardstick (a plain for_each over the same velocity, one output; events around the call).
The cases alternate inside every repeat; warm-up first, then the median of the repeats with their minimum and maximum.  Each case is
reported as a ratio to the yardstick and as a fraction of the 8 TB/s HBM peak on the compulsory traffic of 8 (3 + nout) bytes per cell.
Then, on a level object: ns.histogram of three gradient names (one ghost fill, one launch, one histogram pass) against three separate
derive + histogram passes (the cost structure without derive_fields), and a (n/2)^3 time step with and without the integrals of three
names (what ns.integrate_interval = 1 does).  Writes the table (default profiles/velgrad_bench.txt)."""
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
WARM, REPS, STEPS = 3, 20, 6
lib.init(0)
nn = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "velgrad_bench.txt")
hip = C.CDLL("libamdhip64.so")
stream = C.c_void_p(lib.lib().iamrx_stream())
lines = []
SETS = {1: [7], 3: [7, 8, 4], 10: list(range(10))}          # q_criterion; q_criterion r_invariant enstrophy; all ten
NAMES3 = ["q_criterion", "r_invariant", "enstrophy"]
MU = 0.001


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


def velgrad_ms(g, out, vel, ids, path, split=0):
    ms = (C.c_float * 1)()
    lib.check(lib.lib().iamrx_velgrad_bench(C.byref(g), out.h, len(ids), (C.c_int * len(ids))(*ids), vel.h, 0, C.c_double(MU), int(path), int(split), 1, ms))
    return ms[0]


def med(v):
    return statistics.median(v), min(v), max(v)


def population(tag, lay, g):
    n = g.n
    cells = float(n[0]) * n[1] * n[2]
    e0, e1 = C.c_void_p(), C.c_void_p()
    hipcheck(hip.hipEventCreate(C.byref(e0))); hipcheck(hip.hipEventCreate(C.byref(e1)))
    rng = np.random.default_rng(1)
    out = lib.MultiFab(lay, lib.CELL, 10, 0)
    vel = lib.MultiFab(lay, lib.CELL, 3, 1)
    for field in ("taylorgreen", "random"):
        if field == "taylorgreen":
            ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7, visc_coef=MU, init_iter=2))
            ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
            S = ns.data(ns.S_NEW)
            lib.parallel_copy(vel, S, 0, 0, 3)
            vel.fill_boundary(g)
            del S, ns
        else:
            for li in range(vel.nlocal()):
                glo, ghi = vel.fab_box(li)
                vel.from_numpy(rng.uniform(-1.0, 1.0, size=tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (3,)), li)
        marching = lib.velgrad_path(vel, 0) == 1
        cases = [(f"{'marching' if p == 1 else 'plain   '} {c:2d} output{'s' if c > 1 else ' '}", c, p, 0) for c in (1, 3, 10) for p in ((1, 2) if marching else (2,))]
        cases += [(f"{'marching' if p == 1 else 'plain   '} 10 x 1 output ", 10, p, 1) for p in ((1, 2) if marching else (2,))]
        t = {name: [] for name, _, _, _ in cases}
        yard = []
        for r in range(WARM + REPS):
            y = event_ms(lambda: lib.derive_mag_vort(g, out, vel), e0, e1)
            if r >= WARM:
                yard.append(y)
            for name, c, p, split in cases:
                ms = velgrad_ms(g, out, vel, SETS[c], p, split)
                if r >= WARM:
                    t[name].append(ms)
        y = med(yard)
        say(f"  {tag}, {field} (path 0 takes the {'marching' if marching else 'plain'} form)")
        say(f"    {'derive_mag_vort (yardstick)':26s} {y[0]:8.4f} ms (min {y[1]:.4f}, max {y[2]:.4f})  {32.0 * cells / (y[0] * 1e-3) / 1e12:5.2f} TB/s = {100 * 32.0 * cells / (y[0] * 1e-3) / HBM_PEAK:4.1f} % of peak")
        for name, c, p, split in cases:
            m = med(t[name])
            nbytes = 8.0 * (3 + c) * cells                      # (the split case is charged the fused pass's traffic: what it ought to cost)
            say(f"    {name:26s} {m[0]:8.4f} ms (min {m[1]:.4f}, max {m[2]:.4f})  {nbytes / (m[0] * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (m[0] * 1e-3) / HBM_PEAK:4.1f} % of peak"
                f"  x{m[0] / y[0]:.2f} of the yardstick")
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    del out, vel


def wall_ms(fn):
    lib.sync(); t0 = time.perf_counter()
    fn()
    lib.sync()
    return (time.perf_counter() - t0) * 1e3


def histograms(tag, lay, g):
    """ns.histogram of three gradient names against three separate derive + histogram passes; given ranges, host clock around each"""
    ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7, visc_coef=MU, init_iter=2))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    from iamr_amd.pdf import widen
    ranges = [widen(*ns.derive(nm).minmax(0, 0)) for nm in NAMES3]          # (r_invariant of this field is identically zero: w = 0)

    def fused():
        ns.histogram(NAMES3, 64, ranges)

    def separate():
        for nm, r in zip(NAMES3, ranges):
            lib.mf_histogram(ns.derive(nm), 0, 1, 64, r)
    a, b = [], []
    for r in range(WARM + 10):
        x, y = wall_ms(fused), wall_ms(separate)
        if r >= WARM:
            a.append(x); b.append(y)
    a, b = med(a), med(b)
    say(f"  {tag}: ns.histogram of {' '.join(NAMES3)} {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); three derive + histogram passes {b[0]:.3f} ms "
        f"(min {b[1]:.3f}, max {b[2]:.3f}): x{b[0] / a[0]:.2f}")
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


say(f"velocity-gradient fields, {nn}^3: {WARM} warm-up rounds, median of {REPS} alternating repeats; compulsory traffic = 8 (3 + nout) B per cell (yardstick: 32 B per cell)")
n = (nn,) * 3
g = lib.Geom.make(n)
population(f"one {nn}^3 box", lib.Layout.single(n), g)
population(f"eight {nn // 2}^3 boxes", lib.Layout.decompose(n, nn // 2), g)
say(f"histograms of three gradient names, {nn}^3, TaylorGreen, 64 bins, given ranges (host clock, synchronised)")
histograms(f"one {nn}^3 box", lib.Layout.single(n), g)
histograms(f"eight {nn // 2}^3 boxes", lib.Layout.decompose(n, nn // 2), g)

h = nn // 2
say(f"time step, {h}^3, TaylorGreen")
ns = N.NavierStokes(lib.Geom.make((h,) * 3), lib.Layout.single((h,) * 3), N.ns_params(cfl=0.7, visc_coef=MU, init_iter=2))
ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
ns.post_init()
for _ in range(2):
    ns.step()
names = ["energy", "enstrophy", "dissipation"]
alone, with_i = steps(ns.step, lambda: ns.integrate(names))
say(f"  step alone {alone[0]:.3f} ms (min {alone[1]:.3f}, max {alone[2]:.3f}); step + integrals of {' '.join(names)} {with_i[0]:.3f} ms "
    f"(min {with_i[1]:.3f}, max {with_i[2]:.3f}): {100 * (with_i[0] / alone[0] - 1):+.2f} %")
del ns
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
