"""LES: time of the eddy-viscosity kernel and of the level step it feeds.
  python tools/bench_les.py [n] [out.json]
1. k_les_mut at n^3 (default 256), both models, through iamrx_les_mut: HIP events on the library's launch stream around each launch,
   median of the repeats, against the compulsory traffic (24 B/cell read + 24 B/cell written).
2. the viscous TaylorGreen n^3 step in four modes: do_LES = 0 (uniform-viscosity kernels), do_LES = 1 with Cs = 0 (the same flow through
   the array-coefficient kernels), Smagorinsky, Sigma -- host clock around a synchronised step, median.
Writes one JSON document (default profiles/les_<n>.json)."""
import ctypes as C
import json
import os
import statistics
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N

lib.init(0)
nn = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", f"les_{nn}.json")
n = (nn,) * 3
hip = C.CDLL("libamdhip64.so")
stream = C.c_void_p(lib.lib().iamrx_stream())


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


res = {"n": nn, "kernel": {}, "step": {}}
g = lib.Geom.make(n)
lay = lib.Layout.single(n)
rng = np.random.default_rng(1)
vel = lib.MultiFab(lay, lib.CELL, 3, 1)
vel.from_numpy(np.asfortranarray(rng.standard_normal(tuple(v + 2 for v in n) + (3,))))
mu = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
gb = 48.0 * nn ** 3 / 1e9
for name, model, Cs in (("smagorinsky", N.SMAGORINSKY, 0.18), ("sigma", N.SIGMA, 1.5)):
    for zm in (1, 0):
        lib.tuning_set("LES_ZM", zm)
        event_ms(lambda: N.les_mut(g, vel, mu, model, Cs, base=0.001), 5)
        ms = event_ms(lambda: N.les_mut(g, vel, mu, model, Cs, base=0.001), 30)
        med = statistics.median(ms)
        res["kernel"][f"{name}_{'lds' if zm else 'plain'}"] = dict(ms_median=med, ms_min=min(ms), ms_max=max(ms), compulsory_GB=gb, GBps=gb / med * 1e3)
        print(f"k_les_mut {name:12s} {'LDS  ' if zm else 'plain'} {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})  {gb / med * 1e3:.0f} GB/s of compulsory traffic", flush=True)
lib.tuning_set("LES_ZM", 1)
del vel, mu

for name, kw in (("do_LES=0", {}), ("Cs=0", dict(do_LES=1, LES_model=N.SMAGORINSKY, smago_Cs_cst=0.0)),
                 ("smagorinsky", dict(do_LES=1, LES_model=N.SMAGORINSKY)), ("sigma", dict(do_LES=1, LES_model=N.SIGMA))):
    ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7, visc_coef=0.001, init_iter=2, **kw))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    for _ in range(2):
        ns.step()
    ms = []
    for _ in range(5):
        lib.sync(); t0 = time.perf_counter()
        ns.step()
        lib.sync(); ms.append((time.perf_counter() - t0) * 1e3)
    ns.profile(2)
    ns.step()
    lib.sync()
    sec = ns.profile(0)
    a, b, c = ns.stats()
    res["step"][name] = dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), visc_section_ms=sec[4], visc_iters=c.iters,
                             kinetic_energy=ns.sum_integrated()[2])
    print(f"step {name:12s} {statistics.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}); viscous section {sec[4]:.2f} ms, {c.iters} iterations", flush=True)
    del ns
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
