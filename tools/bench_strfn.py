"""Structure functions (csrc/k_strfn.hip): what each axis costs and what a whole call costs against a time step.
  python tools/bench_strfn.py [out.txt] [n ...]
For every n (default 128 256), on one n^3 box and on eight (n/2)^3 boxes of a periodic domain, for rmax = 16, 64, n/2 and pmax = 2, 4,
8, it times in this one process:
  - the four passes of one component -- pack, then the pair launch of x, y and z with its finish kernel -- through iamrx_strfn_bench:
    HIP events between the passes on the library's stream, nothing read back, the passes alternating inside every repeat; warm-up
    first, then the median of the repeats with their minimum and maximum.  Each axis is set against two rooflines:
      fp64 issue   N (rmax + 1) pairs times the fp64 instructions of a pair (1 subtraction, 2 for the product column, per power an
                   addition and from the second on a multiplication, per odd power the addition of the absolute value: 7 / 12 / 22
                   for pmax 2 / 4 / 8) over 39.3e12 lane-instructions per second (the instruction audit);
      LDS          10 bytes per pair (the partner, and f(x) shared by the four separations a thread carries) over 150 TB/s;
  - one full four-component call (NavierStokes.structure_functions, ends in a read-back: host clock around the synchronised call)
    against one time step of the same TaylorGreen run, alternating, for rmax = n/2 and pmax = 4.
Writes the table (default profiles/strfn_bench.txt)."""
import ctypes as C
import os
import statistics
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N

FP64_ISSUE = 39.3e12          # lane-instructions per second
LDS_RATE = 150.0e12           # bytes per second, every CU streaming
FP64_PER_PAIR = {2: 7, 4: 12, 8: 22}
LDS_PER_PAIR = 10.0
WARM, REPS, STEPS = 2, 10, 6
lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strfn_bench.txt")
sizes = [int(v) for v in sys.argv[2:]] or [128, 256]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return statistics.median(v), min(v), max(v)


def noise_mf(nn, max_grid_size):
    """one component of white noise on nn^3, one box or boxes of max_grid_size"""
    n = (nn,) * 3
    lay = lib.Layout.single(n) if max_grid_size is None else lib.Layout.decompose(n, max_grid_size)
    mf = lib.MultiFab(lay, lib.CELL, 1, 0)
    rng = np.random.default_rng(1)
    for li in range(mf.nlocal()):
        lo, hi = mf.fab_box(li)
        mf.from_numpy(rng.standard_normal(tuple(hi[d] - lo[d] + 1 for d in range(3)) + (1,)) + 0.3, li)
    return mf, lay


def passes(g, mf, nn, rmax, pmax, tag):
    ms = (C.c_float * (4 * (WARM + REPS)))()
    lib.check(lib.lib().iamrx_strfn_bench(C.byref(g), mf.h, 0, pmax, (C.c_int * 3)(rmax, rmax, rmax), WARM + REPS, ms))
    pairs = float(nn) ** 3 * (rmax + 1)
    t_fp, t_lds = pairs * FP64_PER_PAIR[pmax] / FP64_ISSUE * 1e3, pairs * LDS_PER_PAIR / LDS_RATE * 1e3
    row = []
    for p in range(4):
        m, lo, hi = med([ms[4 * r + p] for r in range(WARM, WARM + REPS)])
        row.append(m)
        if p == 0:
            say(f"  {tag:12s} rmax {rmax:3d} pmax {pmax}  pack {m:7.4f} ms (min {lo:.4f}, max {hi:.4f})")
        else:
            say(f"  {tag:12s} rmax {rmax:3d} pmax {pmax}  {'xyz'[p - 1]}    {m:7.4f} ms (min {lo:.4f}, max {hi:.4f})  "
                f"{100 * t_fp / m:5.1f} % of the fp64 issue rate, {100 * t_lds / m:5.1f} % of the LDS rate")
    say(f"  {tag:12s} rmax {rmax:3d} pmax {pmax}  one component {sum(row):8.4f} ms (sum of the medians)")


say(f"structure functions: {WARM} warm-up repeats, median of {REPS}; fp64 issue {FP64_ISSUE / 1e12:.1f} T lane-instructions/s, LDS {LDS_RATE / 1e12:.0f} TB/s")
for nn in sizes:
    g = lib.Geom.make((nn,) * 3)
    say(f"{nn}^3")
    for tag, mgs in (("one box", None), ("eight boxes", nn // 2)):
        mf, lay = noise_mf(nn, mgs)
        for rmax in sorted({16, 64, nn // 2}):
            for pmax in (2, 4, 8):
                passes(g, mf, nn, rmax, pmax, tag)
        del mf
    ns = N.NavierStokes(g, lib.Layout.single((nn,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    for _ in range(2):
        ns.step()
        ns.structure_functions()
    a, b = [], []
    for _ in range(STEPS):
        for dst, fn in ((a, ns.step), (b, ns.structure_functions)):
            lib.sync(); t0 = time.perf_counter()
            fn()
            lib.sync(); dst.append((time.perf_counter() - t0) * 1e3)
    a, b = med(a), med(b)
    say(f"  one step {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); one four-component call, rmax {nn // 2}, pmax 4: {b[0]:.3f} ms "
        f"(min {b[1]:.3f}, max {b[2]:.3f}): {100 * b[0] / a[0]:.1f} % of a step")
    del ns
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
