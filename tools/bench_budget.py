"""Co-spectra and the spectral energy budget (csrc/k_spectrum.hip, csrc/k_convect.hip): what a packed pair costs against a plain
component, the nonlinear term against derive_velgrad, and a whole budget against a whole spectrum and against a time step.
  python tools/bench_budget.py [out.txt] [n]
At n^3 (default 256), on one box and on eight (n/2)^3 boxes, it times in this one process:
  - the five passes of one packed pair (iamrx_cospectrum_bench: pack of two fields, three transforms, the shell sums that read every
    mode with its mirror mode) against the five passes of one plain component (iamrx_spectrum_bench), alternating inside every repeat:
    HIP events between the passes on the library's stream, nothing read back; warm-up first, then the median of the repeats with their
    minimum and maximum.  The shell sums of the pair are reported as a fraction of the 8 TB/s HBM peak on 2 x 16 B per cell (the mode and
    its mirror), those of the plain component on 16; the pair's pack reads 16 and writes 32 B per cell (two launches);
  - the nonlinear term (iamrx_convective_bench, three outputs) against derive_velgrad with three outputs in the form the layout takes
    and in the plain form, on the same random velocity (the reads are the same: 8 (3 + 3) B per cell compulsory);
  - one NavierStokes.spectral_budget() against one four-column NavierStokes.spectrum() (each ends in a read-back: host clock around the
    synchronised call), alternating; the spectrum's time is set beside the value profiles/spectrum_bench.txt holds for the same size;
  - at 128^3: a time step alone and a step followed by a budget (what ns.budget_interval = 1 does), alternating.
Writes the table (default profiles/budget_bench.txt)."""
import ctypes as C
import os
import re
import statistics
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N

HBM_PEAK = 8.0e12
WARM, REPS, STEPS = 5, 30, 6
PLAIN = (("pack", 24.0), ("x transform", 32.0), ("y transform", 32.0), ("z transform", 32.0), ("shell sums", 16.0))
PAIR = (("pack", 48.0), ("x transform", 32.0), ("y transform", 32.0), ("z transform", 32.0), ("shell sums", 32.0))
lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "budget_bench.txt")
nn = int(sys.argv[2]) if len(sys.argv) > 2 else 256
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return statistics.median(v), min(v), max(v)


def random_mf(lay, ncomp, ngrow, seed):
    mf = lib.MultiFab(lay, lib.CELL, ncomp, ngrow)
    rng = np.random.default_rng(seed)
    for li in range(mf.nlocal()):
        lo, hi = mf.fab_box(li)
        mf.from_numpy(rng.uniform(-1.0, 1.0, size=tuple(hi[d] - lo[d] + 1 for d in range(3)) + (ncomp,)) + 0.3, li)
    return mf


def passes(g, mf, cells, tag):
    """the pair (components 0 and 1) and the plain component 0, one call each per repeat"""
    t = {"pair": [[] for _ in range(5)], "plain": [[] for _ in range(5)]}
    ms = (C.c_float * 5)()
    for r in range(WARM + REPS):
        lib.check(lib.lib().iamrx_cospectrum_bench(C.byref(g), mf.h, 0, mf.h, 1, 1, ms))
        if r >= WARM:
            for p in range(5):
                t["pair"][p].append(ms[p])
        lib.check(lib.lib().iamrx_spectrum_bench(C.byref(g), mf.h, 0, 1, ms))
        if r >= WARM:
            for p in range(5):
                t["plain"][p].append(ms[p])
    tot = {}
    for kind, table in (("plain", PLAIN), ("pair", PAIR)):
        tot[kind] = 0.0
        for p, (name, bpc) in enumerate(table):
            m, lo, hi = med(t[kind][p])
            tot[kind] += m
            rate = bpc * cells / (m * 1e-3)
            say(f"  {tag:12s} {kind:5s} {name:12s} {m:8.4f} ms (min {lo:.4f}, max {hi:.4f})  {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of peak on {bpc:.0f} B per cell")
        say(f"  {tag:12s} {kind:5s} {'all five':12s} {tot[kind]:8.4f} ms (sum of the medians)")
    say(f"  {tag:12s} one packed pair = x{tot['pair'] / tot['plain']:.2f} of one plain component (two plain components: x2.00)")


def stencils(g, lay, cells, tag):
    vel = random_mf(lay, 3, 1, 2)
    out = lib.MultiFab(lay, lib.CELL, 3, 0)
    ids = (C.c_int * 3)(7, 8, 4)
    forms = [("derive_velgrad, 3 outputs, layout's form", 0), ("derive_velgrad, 3 outputs, plain form", 2)]
    t = {name: [] for name, _ in forms}
    t["convective term"] = []
    ms = (C.c_float * 1)()
    for r in range(WARM + REPS):
        for name, path in forms:
            lib.check(lib.lib().iamrx_velgrad_bench(C.byref(g), out.h, 3, ids, vel.h, 0, C.c_double(0.001), path, 0, 1, ms))
            if r >= WARM:
                t[name].append(ms[0])
        lib.check(lib.lib().iamrx_convective_bench(C.byref(g), out.h, vel.h, 0, 1, ms))
        if r >= WARM:
            t["convective term"].append(ms[0])
    base = med(t[forms[0][0]])[0]
    for name, v in t.items():
        m, lo, hi = med(v)
        rate = 48.0 * cells / (m * 1e-3)
        say(f"  {tag:12s} {name:42s} {m:8.4f} ms (min {lo:.4f}, max {hi:.4f})  {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of peak on 48 B per cell  x{m / base:.2f}")


def wall_ms(fn):
    lib.sync(); t0 = time.perf_counter()
    fn()
    lib.sync()
    return (time.perf_counter() - t0) * 1e3


def parent_spectrum_ms(n):
    """the four-column spectrum time profiles/spectrum_bench.txt holds for n^3, or None"""
    try:
        txt = open(os.path.join(ROOT, "profiles", "spectrum_bench.txt")).read()
    except OSError:
        return None
    m = re.search(rf"^{n}\^3\n(?:  .*\n)*?  one step .*?one four-column spectrum ([0-9.]+) ms \(min ([0-9.]+), max ([0-9.]+)\)", txt, flags=re.M)
    return tuple(float(v) for v in m.groups()) if m else None


say(f"co-spectra and the spectral budget, {nn}^3: {WARM} warm-up repeats, median of {REPS} alternating repeats; HBM peak {HBM_PEAK / 1e12:.0f} TB/s")
n3 = (nn,) * 3
g = lib.Geom.make(n3)
cells = float(nn) ** 3
for tag, mgs in (("one box", None), ("eight boxes", nn // 2)):
    lay = lib.Layout.single(n3) if mgs is None else lib.Layout.decompose(n3, mgs)
    mf = random_mf(lay, 2, 0, 1)
    passes(g, mf, cells, tag)
    del mf
    stencils(g, lay, cells, tag)

say(f"whole calls, {nn}^3, one box, TaylorGreen after two steps (host clock, synchronised, each ends in a read-back)")
ns = N.NavierStokes(g, lib.Layout.single(n3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
ns.post_init()
for _ in range(2):
    ns.step()
    ns.spectrum()
    ns.spectral_budget()
a, b = [], []
for _ in range(WARM + 10):
    a.append(wall_ms(ns.spectrum)); b.append(wall_ms(ns.spectral_budget))
a, b = med(a[WARM:]), med(b[WARM:])
say(f"  four-column spectrum {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); spectral budget (three packed pairs + the nonlinear term) {b[0]:.3f} ms "
    f"(min {b[1]:.3f}, max {b[2]:.3f}): x{b[0] / a[0]:.2f}")
par = parent_spectrum_ms(nn)
if par:
    say(f"  the four-column spectrum in profiles/spectrum_bench.txt (before the bin kernel took value functors): {par[0]:.3f} ms (min {par[1]:.3f}, max {par[2]:.3f}); "
        f"now {100 * (a[0] / par[0] - 1):+.1f} %, the spread of the repeats above is {100 * (a[2] - a[1]) / a[0]:.1f} % of the median")
del ns

h = 128
say(f"time step, {h}^3, one box, TaylorGreen")
ns = N.NavierStokes(lib.Geom.make((h,) * 3), lib.Layout.single((h,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
ns.post_init()
for _ in range(2):
    ns.step()
    ns.spectral_budget()
a, b = [], []
for _ in range(STEPS):
    a.append(wall_ms(ns.step))
    b.append(wall_ms(lambda: (ns.step(), ns.spectral_budget())))
a, b = med(a), med(b)
say(f"  step alone {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); step + spectral budget {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f}): {100 * (b[0] / a[0] - 1):+.2f} %")
del ns
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
