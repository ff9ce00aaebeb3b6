"""Plane-averaged profiles (csrc/k_profile.hip): what one costs, against the integrated-quantity reduction that reads the same data.
  python tools/bench_profile.py [n] [out.txt]
On one n^3 box (default 256) and on the two-level hierarchy of bench.py's secondary workload (n^3 base box + one n^3 refined box over
its centre) it times, in this one process:
  - the profile along each of the three axes (hierarchy: bin level 0 and 1),
  - iamrx_ns_sum_integrated / iamrx_amr_sum_integrated, the yardstick: one pass over the same five state components,
  - a time step followed by a profile (ns.profile_interval = 1) against a time step alone.
Every call ends in a read-back, so a call is timed from the host around a synchronised call and, for the device's share, with HIP events
on the library's stream; warm-up first, then the median of the repeats with their minimum and maximum.  Each axis is reported as a ratio
to the yardstick and as a fraction of the 8 TB/s HBM peak on the compulsory traffic: 5 x 8 B per cell, plus 8 B per cell of a level that
carries a coverage mask.  Writes the table (default profiles/profile_bench.txt)."""
import ctypes as C
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N
from iamr_amd.amr import Amr

HBM_PEAK = 8.0e12
WARM, REPS, STEPS = 5, 30, 6
lib.init(0)
nn = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "profile_bench.txt")
hip = C.CDLL("libamdhip64.so")
stream = C.c_void_p(lib.lib().iamrx_stream())
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def hipcheck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def timed(fn):
    """(host ms, device ms) per call: medians, minima, maxima of REPS calls after WARM"""
    e0, e1 = C.c_void_p(), C.c_void_p()
    hipcheck(hip.hipEventCreate(C.byref(e0))); hipcheck(hip.hipEventCreate(C.byref(e1)))
    host, dev = [], []
    for r in range(WARM + REPS):
        lib.sync()
        t0 = time.perf_counter()
        hipcheck(hip.hipEventRecord(e0, stream))
        fn()
        hipcheck(hip.hipEventRecord(e1, stream))
        hipcheck(hip.hipEventSynchronize(e1))
        t1 = time.perf_counter()
        t = C.c_float()
        hipcheck(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        if r >= WARM:
            host.append((t1 - t0) * 1e3); dev.append(t.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return tuple((statistics.median(v), min(v), max(v)) for v in (host, dev))


def report(tag, fn, nbytes, yard=None):
    host, dev = timed(fn)
    frac = nbytes / (dev[0] * 1e-3) / HBM_PEAK
    ratio = "" if yard is None else f"  x{dev[0] / yard[0]:.2f} of the yardstick (device), x{host[0] / yard[1]:.2f} (host)"
    say(f"  {tag:34s} device {dev[0]:8.4f} ms (min {dev[1]:.4f}, max {dev[2]:.4f})  host {host[0]:8.4f} ms (min {host[1]:.4f}, max {host[2]:.4f})  "
        f"{nbytes / (dev[0] * 1e-3) / 1e12:5.2f} TB/s = {100 * frac:4.1f} % of peak{ratio}")
    return dev[0], host[0], frac


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
    return (statistics.median(a), min(a), max(a)), (statistics.median(b), min(b), max(b))


say(f"plane-averaged profiles, {nn}^3: {WARM} warm-up calls, median of {REPS}; compulsory traffic = 40 B per cell (+ 8 B per cell of a masked level)")
n = (nn,) * 3
cells = float(nn) ** 3

say(f"one {nn}^3 box")
g = lib.Geom.make(n)
ns = N.NavierStokes(g, lib.Layout.single(n), N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2))
ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
yard = report("sum_integrated (yardstick)", ns.sum_integrated, 40.0 * cells)
worst = min(report(f"plane_profile dir {d}", lambda d=d: ns.plane_profile(d), 40.0 * cells, yard)[2] for d in range(3))
say(f"  slowest axis reaches {100 * worst:.1f} % of peak, the yardstick {100 * yard[2]:.1f} %: " + ("FINDING: less than half of the yardstick's share" if worst < 0.5 * yard[2] else "at least half of the yardstick's share"))
ns.post_init()
for _ in range(2):
    ns.step()
alone, with_p = steps(ns.step, lambda: ns.plane_profile(2))
say(f"  step alone {alone[0]:.3f} ms (min {alone[1]:.3f}, max {alone[2]:.3f}); step + profile {with_p[0]:.3f} ms (min {with_p[1]:.3f}, max {with_p[2]:.3f}): "
    f"{100 * (with_p[0] / alone[0] - 1):+.2f} %")
del ns

say(f"two levels: {nn}^3 base box + one {nn}^3 refined box over its centre")
h = nn // 2
lays = [lib.Layout([((0, 0, 0), (nn - 1,) * 3)]), lib.Layout([((h,) * 3, (h + nn - 1,) * 3)])]
amr = Amr(g, lays, N.ns_params(cfl=0.7, visc_coef=1e-4, init_iter=2, init_shrink=1.0), lib.mg_opts())
for l in range(2):
    amr.levels[l].init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
nbytes = 40.0 * 2 * cells + 8.0 * cells
yard = report("sum_integrated (yardstick)", amr.sum_integrated, nbytes)
fr = [report(f"plane_profile dir {d} bin level {B}", lambda d=d, B=B: amr.plane_profile(d, B), nbytes, yard)[2] for d in range(3) for B in (0, 1)]
say(f"  slowest case reaches {100 * min(fr):.1f} % of peak, the yardstick {100 * yard[2]:.1f} %: " + ("FINDING: less than half of the yardstick's share" if min(fr) < 0.5 * yard[2] else "at least half of the yardstick's share"))
amr.post_init()
amr.coarse_step()
alone, with_p = steps(amr.coarse_step, lambda: amr.plane_profile(2, 1))
say(f"  coarse step alone {alone[0]:.3f} ms (min {alone[1]:.3f}, max {alone[2]:.3f}); coarse step + profile {with_p[0]:.3f} ms (min {with_p[1]:.3f}, max {with_p[2]:.3f}): "
    f"{100 * (with_p[0] / alone[0] - 1):+.2f} %")
del amr
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
