"""Shell-summed spectra (csrc/k_spectrum.hip): what each pass costs and what a whole spectrum costs against a time step.
  python tools/bench_spectrum.py [out.txt] [n ...]
For every n (default 128 256), on one n^3 box and on eight (n/2)^3 boxes, it times in this one process:
  - the five passes of one component -- pack, x transform, y transform, z transform, shell sums -- through iamrx_spectrum_bench: HIP
    events between the passes on the library's stream, nothing read back, the passes alternating inside every repeat; warm-up first,
    then the median of the repeats with their minimum and maximum.  Each pass is reported as a fraction of the 8 TB/s HBM peak on its
    compulsory traffic: the pack reads 8 and writes 16 B per cell, a transform pass reads and writes 16, the shell sums read 16;
  - on the one-box case the same passes under other sizes of the LDS image (SPECTRUM_TILE_ELEMS: complex numbers per workgroup) and
    with one butterfly stage per barrier instead of two (SPECTRUM_PAIR_STAGES = 0);
  - one full four-column spectrum (NavierStokes.spectrum, ends in a read-back: host clock around the synchronised call) against one
    time step of the same TaylorGreen run, alternating.
Writes the table (default profiles/spectrum_bench.txt)."""
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
WARM, REPS, STEPS = 5, 30, 6
DEFAULT_ELEMS = 2048          # k_spectrum.hip: SPECTRUM_TILE_ELEMS
PASSES = (("pack", 24.0), ("x transform", 32.0), ("y transform", 32.0), ("z transform", 32.0), ("shell sums", 16.0))
lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spectrum_bench.txt")
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


def passes(g, mf, cells, tag):
    ms = (C.c_float * (5 * (WARM + REPS)))()
    lib.check(lib.lib().iamrx_spectrum_bench(C.byref(g), mf.h, 0, WARM + REPS, ms))
    total = 0.0
    for p, (name, bpc) in enumerate(PASSES):
        m, lo, hi = med([ms[5 * r + p] for r in range(WARM, WARM + REPS)])
        total += m
        rate = bpc * cells / (m * 1e-3)
        say(f"  {tag:26s} {name:12s} {m:8.4f} ms (min {lo:.4f}, max {hi:.4f})  {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f} % of peak on {bpc:.0f} B per cell")
    say(f"  {tag:26s} {'one component':12s} {total:8.4f} ms (sum of the medians)")
    return total


say(f"shell-summed spectra: {WARM} warm-up repeats, median of {REPS}; HBM peak {HBM_PEAK / 1e12:.0f} TB/s")
for nn in sizes:
    cells = float(nn) ** 3
    g = lib.Geom.make((nn,) * 3)
    say(f"{nn}^3")
    for tag, mgs in (("one box", None), ("eight boxes", nn // 2)):
        mf, lay = noise_mf(nn, mgs)
        passes(g, mf, cells, tag)
        if mgs is None:
            for elems in (512, 1024, 4096):
                lib.tuning_set("SPECTRUM_TILE_ELEMS", elems)
                passes(g, mf, cells, f"one box, LDS image {elems}")
            lib.tuning_set("SPECTRUM_TILE_ELEMS", DEFAULT_ELEMS)
            lib.tuning_set("SPECTRUM_PAIR_STAGES", 0)
            passes(g, mf, cells, "one box, single stages")
            lib.tuning_set("SPECTRUM_PAIR_STAGES", 1)
            passes(g, mf, cells, "one box (again)")
        del mf
    ns = N.NavierStokes(g, lib.Layout.single((nn,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    for _ in range(2):
        ns.step()
        ns.spectrum()
    a, b = [], []
    for _ in range(STEPS):
        for dst, fn in ((a, ns.step), (b, ns.spectrum)):
            lib.sync(); t0 = time.perf_counter()
            fn()
            lib.sync(); dst.append((time.perf_counter() - t0) * 1e3)
    a, b = med(a), med(b)
    say(f"  one step {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); one four-column spectrum {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f}): "
        f"{100 * b[0] / a[0]:.1f} % of a step")
    del ns
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
