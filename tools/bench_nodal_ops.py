"""nodal residual, interpolation, restriction and divergence at n^3 cells (periodic box, variable sigma) through the C-ABI; run under
rocprofv3 --kernel-trace --stats for the per-kernel times.  The forms behind NODAL_RES_TILE, NODAL_INTERP_LDS (0: per coarse node, 1: LDS
tile), NODAL_RESTRICT_TILE and NODAL_DIVU_ZM are looped over, ten calls each.  python tools/bench_nodal_ops.py [n]

python tools/bench_nodal_ops.py kc [calls]: the z-chunk length of the z-marching residual (IAMRX_NODAL_RES_KC) scanned at 16^3 .. 256^3 cells
(17^3 .. 257^3 nodes) in the form the multigrid cycle runs (image reads, right-hand side, no norm): microseconds per call of an isolated
loop of `calls` launches, the best of five loops, 0 = the library's own choice.
python tools/bench_nodal_ops.py images [calls]: residual and restriction with ghost reads against image reads, the same way."""
import sys, os, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N
lib.init(0)


def kc_scan(calls):
    rng = np.random.default_rng(5)
    for m in (16, 32, 64, 128, 256):
        n = (m,) * 3
        g, lay = lib.Geom.make(n), lib.Layout.single(n)
        sig = lib.MultiFab(lay, lib.CELL, 1, 1)
        sig.set_from_global(1.0 + 0.3 * rng.random(tuple(v + 2 for v in n) + (1,)), (-1, -1, -1))
        x, r, out = lib.MultiFab(lay, lib.NODE, 1, 1), lib.MultiFab(lay, lib.NODE, 1, 1), lib.MultiFab(lay, lib.NODE, 1, 1)
        x.set_from_global(rng.standard_normal(tuple(v + 3 for v in n) + (1,)), (-1, -1, -1))
        r.set_from_global(rng.standard_normal(tuple(v + 3 for v in n) + (1,)), (-1, -1, -1))
        call = lambda: lib.check(lib.lib().iamrx_nodal_residual_images(C.byref(g), out.h, x.h, sig.h, r.h, lib.i3((0, 0, 0)), lib.i3((0, 0, 0)), None))
        ref, line = None, []
        for kc in (0, 1, 2, 4, 8, 16, 32, 64):
            if kc > m + 1: continue
            lib.tuning_set("NODAL_RES_KC", kc)
            best = 1e30
            for _ in range(6):                       # (the first loop warms up)
                lib.sync(); t0 = time.perf_counter()
                for _ in range(calls): call()
                lib.sync(); best = min(best, (time.perf_counter() - t0) / calls * 1e6)
            got = out.gather_valid(n)
            if ref is None: ref = got
            line.append("kc %2d: %6.1f us%s" % (kc, best, "" if np.array_equal(got, ref) else " DIFFERENT"))
        print("%3d^3 nodes  " % (m + 1) + "  ".join(line), flush=True)
    lib.tuning_set("NODAL_RES_KC", 0)


def images_scan(calls):
    """residual and restriction with ghost reads against image reads (same kernels, the run-time argument off / on) in isolated loops"""
    rng = np.random.default_rng(5)
    z = lib.i3((0, 0, 0))
    for m in (64, 128, 256):
        n, nc = (m,) * 3, (m // 2,) * 3
        g, lay, clay = lib.Geom.make(n), lib.Layout.single(n), lib.Layout.single(nc)
        sig = lib.MultiFab(lay, lib.CELL, 1, 1)
        sig.set_from_global(1.0 + 0.3 * rng.random(tuple(v + 2 for v in n) + (1,)), (-1, -1, -1))
        x, r, out = lib.MultiFab(lay, lib.NODE, 1, 1), lib.MultiFab(lay, lib.NODE, 1, 1), lib.MultiFab(lay, lib.NODE, 1, 1)
        x.set_from_global(rng.standard_normal(tuple(v + 3 for v in n) + (1,)), (-1, -1, -1))
        r.set_from_global(rng.standard_normal(tuple(v + 3 for v in n) + (1,)), (-1, -1, -1))
        c = lib.MultiFab(clay, lib.NODE, 1, 1)
        L = lib.lib()
        forms = {"residual ghost reads": lambda: lib.check(L.iamrx_nodal_residual(C.byref(g), out.h, x.h, sig.h, r.h)),
                 "residual image reads": lambda: lib.check(L.iamrx_nodal_residual_images(C.byref(g), out.h, x.h, sig.h, r.h, z, z, None)),
                 "restrict ghost reads": lambda: lib.check(L.iamrx_nodal_restrict(c.h, x.h)),
                 "restrict image reads": lambda: lib.check(L.iamrx_nodal_restrict_images(C.byref(g), c.h, x.h, z, z))}
        line = []
        for rep in range(2):                         # ghost / image / ghost / image: the order does not decide
            for name, call in forms.items():
                best = 1e30
                for _ in range(6):
                    lib.sync(); t0 = time.perf_counter()
                    for _ in range(calls): call()
                    lib.sync(); best = min(best, (time.perf_counter() - t0) / calls * 1e6)
                line.append("%s %6.1f us" % (name, best))
        print("%3d^3 nodes  " % (m + 1) + "  ".join(line), flush=True)


if len(sys.argv) > 1 and sys.argv[1] in ("kc", "images"):
    import ctypes as C
    (kc_scan if sys.argv[1] == "kc" else images_scan)(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    sys.exit(0)
n = (int(sys.argv[1]) if len(sys.argv) > 1 else 256,) * 3
nc = tuple(v // 2 for v in n)
g = lib.Geom.make(n)
lay, clay = lib.Layout.single(n), lib.Layout.single(nc)
rng = np.random.default_rng(5)
sig = lib.MultiFab(lay, lib.CELL, 1, 1)
sig.set_from_global(1.0 + 0.3 * rng.random(tuple(v + 2 for v in n) + (1,)), (-1, -1, -1))
x = lib.MultiFab(lay, lib.NODE, 1, 1); r = lib.MultiFab(lay, lib.NODE, 1, 0); out = lib.MultiFab(lay, lib.NODE, 1, 0)
x.set_from_global(rng.standard_normal(tuple(v + 3 for v in n) + (1,)), (-1, -1, -1))
r.set_from_global(rng.standard_normal(tuple(v + 1 for v in n) + (1,)), (0, 0, 0))
c = lib.MultiFab(clay, lib.NODE, 1, 0)
c.set_from_global(rng.standard_normal(tuple(v + 1 for v in nc) + (1,)), (0, 0, 0))
ref = None
for tile in (0, 1, 2, 3):
    lib.tuning_set("NODAL_RES_TILE", tile)
    for _ in range(10): N.nodal_residual(g, out, x, sig, r)
    lib.sync()
    got = out.gather_valid(tuple(v + 1 for v in n))
    if ref is None: ref = got
    print("residual tile", tile, "identical to tile 0:", bool(np.array_equal(got, ref)), flush=True)
f0 = None
for form in (0, 1):
    lib.tuning_set("NODAL_INTERP_LDS", form)
    f = lib.MultiFab(lay, lib.NODE, 1, 1); f.setval(0.0)
    for _ in range(10): N.nodal_interp_add(f, c, sig)
    lib.sync()
    got = f.gather_valid(tuple(v + 1 for v in n))
    if f0 is None: f0 = got
    print("interp form", form, "identical to form 0:", bool(np.array_equal(got, f0)), flush=True)
lib.tuning_set("NODAL_INTERP_LDS", 1)
c0 = None
lib.tuning_set("NODAL_RESTRICT_MIN", 16)
for form in (0, 1):
    lib.tuning_set("NODAL_RESTRICT_TILE", form)
    for _ in range(10): N.nodal_restrict(c, x)
    lib.sync()
    got = c.gather_valid(tuple(v + 1 for v in nc))
    if c0 is None: c0 = got
    print("restrict form", form, "identical to form 0:", bool(np.array_equal(got, c0)), flush=True)
vel = lib.MultiFab(lay, lib.CELL, 3, 1)
vel.set_from_global(rng.standard_normal(tuple(v + 2 for v in n) + (3,)), (-1, -1, -1))
d0 = None
for form in (0, 1):
    lib.tuning_set("NODAL_DIVU_ZM", form)
    for _ in range(10): N.nodal_divu(g, r, vel, 0)
    lib.sync()
    got = r.gather_valid(tuple(v + 1 for v in n))
    if d0 is None: d0 = got
    print("divu form", form, "identical to form 0:", bool(np.array_equal(got, d0)), flush=True)
