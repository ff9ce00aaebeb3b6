"""A-priori LES analysis (csrc/k_sgs.hip, driver in csrc/k_spectrum.hip): what each pass costs, against a yardstick timed in the same run.
  python tools/bench_sgs.py [out.txt] [n ...]
For every n (default 256), on one n^3 box and on eight (n/2)^3 boxes, it times in this one process through iamrx_sgs_bench -- HIP events
between the passes on the library's stream, nothing read back, all passes inside every repeat; warm-up first, then the median of the
repeats with their minimum, maximum and spread (the mean relative distance of a repeat from the median):
  - the product pack (two 8-byte reads and one 16-byte write per cell: 32 B) against the plain pack (24 B) and dense_pack alone;
  - k_sgs_point with its finish kernel in three configurations -- all ten fields, statistics only, one field -- against its compulsory
    traffic at the 8 TB/s HBM peak (nine 16-byte reads per cell plus 8 B per field written) and against derive_velgrad with ten outputs,
    the nearest existing kernel (the same stencil on three components, through the three-plane LDS ring);
  - the 54 transform passes and nine multipliers against nine times the one-component filter of iamrx_specop_bench (the same kernels);
  - a whole statistics-only call on the host clock against one time step of a TaylorGreen run of the same size, alternating.
Writes the table (default profiles/sgs_bench.txt)."""
import ctypes as C
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N

HBM_PEAK = 8.0e12
WARM, REPS, STEPS = 5, 30, 6
lib.init(0)
NP = lib.lib().iamrx_sgs_bench_np()
NPF = lib.lib().iamrx_specop_bench_np()
assert NP == 6
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sgs_bench.txt")
sizes = [int(v) for v in sys.argv[2:]] or [256]
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    m = statistics.median(v)
    return m, min(v), max(v), statistics.mean(abs(x - m) for x in v) / m


def layout(nn, mgs):
    n = (nn,) * 3
    return lib.Layout.single(n) if mgs is None else lib.Layout.decompose(n, mgs)


def row(tag, name, v, bpc, cells, extra=""):
    m, lo, hi, spread = med(v)
    rate = bpc * cells / (m * 1e-3)
    say(f"  {tag:12s} {name:30s} {m:8.4f} ms (min {lo:.4f}, max {hi:.4f}, spread {100 * spread:4.1f} %)  {rate / 1e12:5.2f} TB/s = "
        f"{100 * rate / HBM_PEAK:4.1f} % of peak on {bpc:.0f} B per cell{extra}")
    return m, spread


say(f"a-priori LES analysis: {WARM} warm-up repeats, median of {REPS}; HBM peak {HBM_PEAK / 1e12:.0f} TB/s; Gaussian filter, kc = n / 8")
for nn in sizes:
    cells = float(nn) ** 3
    g = lib.Geom.make((nn,) * 3)
    kc = C.c_double(nn / 8.0)
    say(f"{nn}^3")
    for tag, mgs in (("one box", None), ("eight boxes", nn // 2)):
        lay = layout(nn, mgs)
        vel = lib.MultiFab(lay, lib.CELL, 3, 1)
        lib.mf_noise(g, vel, 1, 0, 3)
        vel.fill_boundary(g)
        out = lib.MultiFab(lay, lib.CELL, 10, 0)
        point = {}
        for cfg, ids in (("all ten fields", list(range(10))), ("statistics only", []), ("one field (sgs_flux)", [7])):
            ms = (C.c_float * (NP * (WARM + REPS)))()
            which = (C.c_int * max(len(ids), 1))(*ids)
            lib.check(lib.lib().iamrx_sgs_bench(C.byref(g), out.h if ids else None, vel.h, 0, 2, kc, len(ids), which if ids else None, WARM + REPS, ms))
            col = lambda p: [ms[NP * r + p] for r in range(WARM, WARM + REPS)]
            if cfg == "all ten fields":
                dense, _ = row(tag, "dense_pack alone", col(5), 24.0, cells)
                plain, sp = row(tag, "3 plain packs", col(0), 72.0, cells, f"; per image {med(col(0))[0] / 3 / dense:.2f} x dense_pack")
                prod, sq = row(tag, "6 product packs", col(1), 192.0, cells)
                say(f"  {tag:12s} product pack / plain pack per image: {(prod / 6) / (plain / 3):.3f} (traffic ratio 32 / 24 = 1.333; spreads {100 * sp:.1f} % and {100 * sq:.1f} %)")
                trans, spt = row(tag, "54 transforms + 9 multipliers", col(2), 9 * 7 * 32.0, cells)
                row(tag, "unpack of ten fields", col(4), 240.0, cells)
            point[cfg], _ = row(tag, "k_sgs_point, " + cfg, col(3), 144.0 + 8.0 * len(ids), cells)
        # derive_velgrad with ten outputs in the same run: the marching form where it applies (path 0 decides as a call does)
        ids = list(range(10))
        msv = (C.c_float * (WARM + REPS))()
        lib.check(lib.lib().iamrx_velgrad_bench(C.byref(g), out.h, 10, (C.c_int * 10)(*ids), vel.h, 0, C.c_double(0.001), 0, 0, WARM + REPS, msv))
        vg, _ = row(tag, "derive_velgrad, ten outputs", list(msv)[WARM:], 24.0 + 80.0, cells)
        for cfg, m in point.items():
            say(f"  {tag:12s} k_sgs_point, {cfg}: {m / vg:.2f} x derive_velgrad with ten outputs")
        # nine times the one-component filter of iamrx_specop_bench: its passes 1 .. 7 (3 forward, the multiplier, 3 inverse)
        src, dst = lib.MultiFab(lay, lib.CELL, 1, 0), lib.MultiFab(lay, lib.CELL, 3, 0)
        lib.mf_noise(g, src, 1, 0, 1)
        msf = (C.c_float * (NPF * (WARM + REPS)))()
        lib.check(lib.lib().iamrx_specop_bench(C.byref(g), dst.h, src.h, 0, 2, kc, 1, WARM + REPS, msf))
        one = [sum(msf[NPF * r + p] for p in range(1, 8)) for r in range(WARM, WARM + REPS)]
        m1 = med(one)
        say(f"  {tag:12s} one-component filter, 6 transforms + multiplier {m1[0]:8.4f} ms (min {m1[1]:.4f}, max {m1[2]:.4f}, spread {100 * m1[3]:4.1f} %); "
            f"nine of them {9 * m1[0]:.4f} ms; the analysis' 54 + 9 passes are {trans / (9 * m1[0]):.3f} x that (spread {100 * spt:.1f} %)")
        del vel, out, src, dst
    ns = N.NavierStokes(g, lib.Layout.single((nn,) * 3), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    for _ in range(2):
        ns.step()
        ns.sgs("gaussian", nn / 8.0)
    a, b = [], []
    for _ in range(STEPS):
        for dst, fn in ((a, ns.step), (b, lambda: ns.sgs("gaussian", nn / 8.0))):
            lib.sync(); t0 = time.perf_counter()
            fn()
            lib.sync(); dst.append((time.perf_counter() - t0) * 1e3)
    a, b = med(a), med(b)
    say(f"  one step {a[0]:.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); one statistics-only call (host clock, tables and the read-back included) "
        f"{b[0]:.3f} ms (min {b[1]:.3f}, max {b[2]:.3f}): {100 * b[0] / a[0]:.1f} % of a step")
    del ns
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
