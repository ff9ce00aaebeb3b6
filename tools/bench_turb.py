"""Turbulent forcing: time of the force kernel and its share of the level step.
  python tools/bench_turb.py [out.json]
1. iamrx_turb_force (k_turb_factors + k_turb_force, the tutorial's table: nmodes 4, 54 modes, divergence-free form) on one box of 128^3 and
   of 256^3 with one ghost layer: HIP events on the library's launch stream around each call, median of the repeats, against the
   compulsory traffic (24 B per cell written).
2. the TaylorGreen-size 256^3 viscous step with the forcing on and off, interleaved: host clock around a synchronised step, median.
The direct per-cell form is timed by tools/turb_direct.hip.  Writes one JSON document (default profiles/turb_force.json)."""
import ctypes as C
import json
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N

lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "turb_force.json")
hip = C.CDLL("libamdhip64.so")
stream = C.c_void_p(lib.lib().iamrx_stream())
CUBE = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def hipcheck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def event_ms(fn, reps):
    e0, e1 = C.c_void_p(), C.c_void_p()
    hipcheck(hip.hipEventCreate(C.byref(e0))); hipcheck(hip.hipEventCreate(C.byref(e1)))
    ms = []
    for _ in range(reps):
        hipcheck(hip.hipEventRecord(e0, stream))
        fn()
        hipcheck(hip.hipEventRecord(e1, stream))
        hipcheck(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hipcheck(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(t.value)
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return ms


res = {"kernel": {}, "step": {}}
k, d = lib.host_turb_modes(CUBE[0], CUBE[1], 4, 0, 1)
for nn in (128, 256):
    n = (nn,) * 3
    g = lib.Geom.make(n, prob_lo=CUBE[0], prob_hi=CUBE[1])
    out = lib.MultiFab(lib.Layout.single(n), lib.CELL, 3, 1)
    event_ms(lambda: lib.turb_force(g, k, d, 1, 0.37, out), 5)
    ms = event_ms(lambda: lib.turb_force(g, k, d, 1, 0.37, out), 30)
    med = statistics.median(ms)
    gb = 24.0 * (nn + 2) ** 3 / 1e9
    res["kernel"][str(nn)] = {"modes": int(len(k)), "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "written_GB": gb, "GB_per_s": gb / (med * 1e-3)}
    print("turb_force", nn, res["kernel"][str(nn)], flush=True)
    del out

n = (256,) * 3
g = lib.Geom.make(n)
runs = {}
for name, on in (("unforced", 0), ("forced", 1)):
    ns = N.NavierStokes(g, lib.Layout.single(n), N.ns_params(cfl=0.7, visc_coef=1.0e-4, turb_forcing=on))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 0.0, 1.0)
    ns.post_init(-1.0)
    for _ in range(2):
        ns.step()
    lib.sync()
    runs[name] = (ns, [])
for _ in range(6):                             # interleaved: unforced, forced, unforced, ...
    for name in ("unforced", "forced"):
        ns, ts = runs[name]
        lib.sync()
        t0 = time.perf_counter()
        ns.step()
        lib.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
for name, (ns, ts) in runs.items():
    res["step"][name] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "ms": ts}
    print("step", name, res["step"][name], flush=True)
res["step"]["forced_minus_unforced_ms"] = res["step"]["forced"]["ms_median"] - res["step"]["unforced"]["ms_median"]
res["step"]["two_evaluations_share"] = 2.0 * res["kernel"]["256"]["ms_median"] / res["step"]["forced"]["ms_median"]
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
