"""Plane spectra (csrc/k_spectrum.hip): what each pass costs, the ring pass of every direction against the shell-sum pass of the 3-D
spectrum on the same image, a whole call against a whole spectrum call, and the diagnostic against a step of the flow it is for.
  python tools/bench_plane_spectrum.py [out.txt] [n ...]
For every n (default 256 128), on one n^3 box and on eight (n/2)^3 boxes, in this one process:
  - the four passes of one component -- pack, the first and the second transform pass, the ring sums with their slot sum -- through
    iamrx_plane_spectrum_bench for each normal direction, and the five passes of iamrx_spectrum_bench on the same array, the four calls
    alternating in every round; the first repeats of every call are warm-up, the rest are pooled: the median with minimum and maximum.
    Each pass is reported as a fraction of the 8 TB/s HBM peak on its compulsory traffic: the pack reads 8 and writes 16 B per cell, a
    transform pass reads and writes 16, the ring pass reads 16 once;
  - one full five-column plane spectrum (NavierStokes.plane_spectrum, ends in a read-back: host clock around the synchronised call) of
    every direction against one full four-column spectrum of the same TaylorGreen level, alternating.
Then a step of the flow of tests/golden/inputs.3d.rayleightaylor_planes16 at 128^3 against the plane spectrum along z that
ns.plane_spectrum_interval = 1 adds to every step, alternating.  Writes the table (default profiles/plane_spectrum_bench.txt)."""
import ctypes as C
import os
import statistics
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N, planespec, run as R
from iamr_amd.inputs import Inputs

HBM_PEAK = 8.0e12
ROUNDS, WARM, REPS, STEPS = 5, 2, 6, 6
PLANE_PASSES = (("pack", 24.0), ("transform 1", 32.0), ("transform 2", 32.0), ("ring sums", 16.0))
SPEC_PASSES = (("pack", 24.0), ("x transform", 32.0), ("y transform", 32.0), ("z transform", 32.0), ("shell sums", 16.0))
RT16 = os.path.join(ROOT, "tests", "golden", "inputs.3d.rayleightaylor_planes16")
lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "plane_spectrum_bench.txt")
sizes = [int(v) for v in sys.argv[2:]] or [256, 128]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return statistics.median(v), min(v), max(v)


def noise_mf(nn, max_grid_size):
    n = (nn,) * 3
    lay = lib.Layout.single(n) if max_grid_size is None else lib.Layout.decompose(n, max_grid_size)
    mf = lib.MultiFab(lay, lib.CELL, 1, 0)
    rng = np.random.default_rng(1)
    for li in range(mf.nlocal()):
        lo, hi = mf.fab_box(li)
        mf.from_numpy(rng.standard_normal(tuple(hi[d] - lo[d] + 1 for d in range(3)) + (1,)) + 0.3, li)
    return mf, lay


def passes(g, mf, cells, tag):
    """-> the median of the shell-sum pass and of the ring pass of every direction"""
    pool = {"spec": [], 0: [], 1: [], 2: []}
    for _ in range(ROUNDS):
        ms = (C.c_float * (5 * (WARM + REPS)))()
        lib.check(lib.lib().iamrx_spectrum_bench(C.byref(g), mf.h, 0, WARM + REPS, ms))
        pool["spec"] += [[ms[5 * r + p] for p in range(5)] for r in range(WARM, WARM + REPS)]
        for dir in (0, 1, 2):
            pool[dir] += planespec.plane_spectrum_bench(g, mf, dir, 0, WARM + REPS)[WARM:].tolist()
    last = {}
    for key, names in (("spec", SPEC_PASSES), (2, PLANE_PASSES), (1, PLANE_PASSES), (0, PLANE_PASSES)):
        what = "3-D spectrum" if key == "spec" else f"planes normal to {'xyz'[key]}"
        total = 0.0
        for p, (name, bpc) in enumerate(names):
            m, lo, hi = med([row[p] for row in pool[key]])
            total += m
            rate = bpc * cells / (m * 1e-3)
            say(f"  {tag:12s} {what:19s} {name:12s} {m:8.4f} ms (min {lo:.4f}, max {hi:.4f})  {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of peak on {bpc:.0f} B per cell")
            last[key] = m
        say(f"  {tag:12s} {what:19s} {'one component':12s} {total:8.4f} ms (sum of the medians)")
    for dir in (2, 1, 0):
        say(f"  {tag:12s} ring pass normal to {'xyz'[dir]} / shell-sum pass = {last[dir] / last['spec']:.2f}")


def alternate(fns):
    t = [[] for _ in fns]
    for _ in range(STEPS):
        for q, fn in enumerate(fns):
            lib.sync(); t0 = time.perf_counter()
            fn()
            lib.sync(); t[q].append((time.perf_counter() - t0) * 1e3)
    return [med(v) for v in t]


say(f"plane spectra: {ROUNDS} rounds of the four calls alternating, {WARM} warm-up repeats per call, median of {ROUNDS * REPS}; HBM peak {HBM_PEAK / 1e12:.0f} TB/s")
for nn in sizes:
    cells = float(nn) ** 3
    g = lib.Geom.make((nn,) * 3)
    say(f"{nn}^3")
    for tag, mgs in (("one box", None), ("eight boxes", nn // 2)):
        mf, lay = noise_mf(nn, mgs)
        passes(g, mf, cells, tag)
        del mf
    ns = N.NavierStokes(g, lib.Layout.single((nn,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    for _ in range(2):
        ns.spectrum()
        for dir in (0, 1, 2):
            ns.plane_spectrum(dir)
    s, p0, p1, p2 = alternate([ns.spectrum, lambda: ns.plane_spectrum(0), lambda: ns.plane_spectrum(1), lambda: ns.plane_spectrum(2)])
    say(f"  one four-column spectrum {s[0]:.3f} ms (min {s[1]:.3f}, max {s[2]:.3f}) = {s[0] / 4:.3f} per column")
    for dir, p in ((2, p2), (1, p1), (0, p0)):
        say(f"  one five-column plane spectrum normal to {'xyz'[dir]} {p[0]:.3f} ms (min {p[1]:.3f}, max {p[2]:.3f}) = {p[0] / 5:.3f} per column: "
            f"{(p[0] / 5) / (s[0] / 4):.2f} of a spectrum's column")
    del ns
# the flow the diagnostic is for: the RayleighTaylor fixture at 128^3 (cubic cells as in config C5), one level, one box
inp = Inputs([RT16], ["amr.n_cell=128 128 128", "geometry.prob_hi=53.5 53.5 88.5", "amr.max_grid_size=128", "max_step=100"])
ns = R.build(inp, lib, N)[0]
ns.post_init(1.0)
for _ in range(2):
    ns.step()
    ns.plane_spectrum(2)
a, b = alternate([ns.step, lambda: ns.plane_spectrum(2)])
say(f"RayleighTaylor 128^3 (periodic x, y; slip walls z): one step {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); one five-column plane spectrum "
    f"normal to z {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f}): a step with the diagnostic at every step {a[0] + b[0]:.3f} ms, +{100 * b[0] / a[0]:.1f} %")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
