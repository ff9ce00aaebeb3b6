"""Spectral filters and the synthetic field (csrc/k_spectrum.hip): what each pass costs and what a whole synthesis costs against a step.
  python tools/bench_filter.py [out.txt] [n ...]
For every n (default 256), on one n^3 box and on eight (n/2)^3 boxes, it times in this one process through iamrx_specop_bench -- HIP
events between the passes on the library's stream, nothing read back, all passes inside every repeat (so they alternate); warm-up
first, then the median of the repeats with their minimum and maximum:
  - the nine passes of one Gaussian filter -- pack, 3 forward transforms, the multiplier, 3 inverse transforms, unpack -- each as a
    fraction of the 8 TB/s HBM peak on its compulsory traffic: the pack reads 8 and writes 16 B per cell, the unpack reads 16 (the
    16-byte mode, of which it keeps the real part) and writes 8, every other pass reads and writes 16;
  - the multiplier and the unpack against dense_pack alone in the same repeat (the streaming yardstick of this library);
  - each inverse pass against the forward pass of the same axis (the same kernel on the same array: they should agree within the
    run-to-run spread, printed as the mean relative distance of a repeat from the median);
  - the seven steps of one synthesis (three components: noise, 9 forward passes, projection, 3 shell sums and a(s), shell scale,
    9 inverse passes, 3 unpacks), and their sum against one time step of a TaylorGreen run of the same size (host clock around the
    synchronised call), alternating.
Writes the table (default profiles/filter_bench.txt)."""
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
FILTER = (("pack", 24.0), ("forward x", 32.0), ("forward y", 32.0), ("forward z", 32.0), ("multiplier", 32.0), ("inverse x", 32.0),
          ("inverse y", 32.0), ("inverse z", 32.0), ("unpack", 24.0))
# bytes per cell of the three components together
SYNTH = (("noise", 48.0), ("9 forward passes", 288.0), ("projection", 96.0), ("shell sums, a(s)", 48.0), ("shell scale", 96.0),
         ("9 inverse passes", 288.0), ("3 unpacks", 72.0))
lib.init(0)
NP = lib.lib().iamrx_specop_bench_np()
assert NP == len(FILTER) + len(SYNTH) + 1
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "filter_bench.txt")
sizes = [int(v) for v in sys.argv[2:]] or [256]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    m = statistics.median(v)
    return m, min(v), max(v), statistics.mean(abs(x - m) for x in v) / m


def noise_mf(nn, max_grid_size, ncomp):
    n = (nn,) * 3
    lay = lib.Layout.single(n) if max_grid_size is None else lib.Layout.decompose(n, max_grid_size)
    mf = lib.MultiFab(lay, lib.CELL, ncomp, 0)
    lib.mf_noise(lib.Geom.make(n), mf, 1, 0, ncomp)
    return mf


def row(tag, name, v, bpc, cells, extra=""):
    m, lo, hi, spread = med(v)
    rate = bpc * cells / (m * 1e-3)
    say(f"  {tag:12s} {name:18s} {m:8.4f} ms (min {lo:.4f}, max {hi:.4f}, spread {100 * spread:4.1f} %)  {rate / 1e12:5.2f} TB/s = "
        f"{100 * rate / HBM_PEAK:4.1f} % of peak on {bpc:.0f} B per cell{extra}")
    return m


say(f"spectral filter and synthesis: {WARM} warm-up repeats, median of {REPS}; HBM peak {HBM_PEAK / 1e12:.0f} TB/s")
for nn in sizes:
    cells = float(nn) ** 3
    g = lib.Geom.make((nn,) * 3)
    say(f"{nn}^3")
    synth_ms = None
    for tag, mgs in (("one box", None), ("eight boxes", nn // 2)):
        src, dst = noise_mf(nn, mgs, 1), noise_mf(nn, mgs, 3)
        ms = (C.c_float * (NP * (WARM + REPS)))()
        lib.check(lib.lib().iamrx_specop_bench(C.byref(g), dst.h, src.h, 0, 2, C.c_double(nn / 8.0), 1, WARM + REPS, ms))
        col = lambda p: [ms[NP * r + p] for r in range(WARM, WARM + REPS)]
        dense = row(tag, "dense_pack alone", col(NP - 1), 24.0, cells)
        m = {}
        for p, (name, bpc) in enumerate(FILTER):
            extra = ""
            if name in ("multiplier", "unpack"):
                extra = f"; {med(col(p))[0] / dense:.2f} x dense_pack"
            if name.startswith("inverse"):
                extra = f"; {med(col(p))[0] / m['forward ' + name[-1]]:.3f} x forward {name[-1]}"
            m[name] = row(tag, name, col(p), bpc, cells, extra)
        say(f"  {tag:12s} {'one filter':18s} {sum(m.values()):8.4f} ms (sum of the medians)")
        tot = 0.0
        for p, (name, bpc) in enumerate(SYNTH):
            tot += row(tag, name, col(len(FILTER) + p), bpc, cells)
        say(f"  {tag:12s} {'one synthesis':18s} {tot:8.4f} ms (sum of the medians)")
        synth_ms = tot if synth_ms is None else synth_ms
        del src, dst
    ns = N.NavierStokes(g, lib.Layout.single((nn,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    vel = lib.MultiFab(lib.Layout.single((nn,) * 3), lib.CELL, 3, 0)
    from iamr_amd.spectral import hit_spectrum
    from iamr_amd.spectrum import nbins_of
    E = hit_spectrum(nbins_of((nn,) * 3, (1.0,) * 3), (1.0,) * 3, 4.0, 1.0, n=(nn,) * 3)
    for _ in range(2):
        ns.step()
        lib.mf_synthesize(g, vel, E)
    a, b = [], []
    for _ in range(STEPS):
        for dst, fn in ((a, ns.step), (b, lambda: lib.mf_synthesize(g, vel, E))):
            lib.sync(); t0 = time.perf_counter()
            fn()
            lib.sync(); dst.append((time.perf_counter() - t0) * 1e3)
    a, b = med(a), med(b)
    say(f"  one step {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); one synthesis call (host clock, tables and the error flag's read-back "
        f"included) {b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f}): {100 * b[0] / a[0]:.1f} % of a step; its passes by events {synth_ms:.3f} ms")
    del ns, vel
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
