"""Tracer particles: time of the advect kernel, of the sample kernel, of a redistribution, and their share of the level step.
  python tools/bench_particles.py [out.json]
1. Particles.advect (k_part_advect, both passes) for 2^20 particles on one 128^3 periodic box with a smooth velocity: HIP events on the
   library's launch stream around each call, median of the repeats, once with the particles in random order and once grouped by cell
   (sorted by their cell index before they are added; redistribution keeps the order of arrival up to its atomics), alternating.
   Reported as particles per second and as effective gather bandwidth: per particle and pass 24 face values of 8 B are gathered, and
   pass 1 reads 3 + writes 6, pass 2 reads 6 + writes 6 doubles of particle data plus the id and box words (2 x 4 B per pass):
   bytes = 2 x 24 x 8 + (9 + 12) x 8 + 16 = 568 B per particle.
1b. Particles.sample (k_part_sample, launch only: nothing read back) of M = 1 and M = 5 components of a smooth 5-component cell array with
   one ghost layer, on the same two populations and in the same alternation, HIP events as in 1.  Per particle 8 M cell values are
   gathered and M written, and 3 position doubles, the id and the box word are read: bytes = 32 + 72 M.  Reported next to the advect
   kernel's time on the same population.
2. Particles.redistribute of the same two sets, host clock around a synchronised call, median.
3. a 128^3 TaylorGreen viscous step with one particle per 8 cells attached against the same step without particles, interleaved: host
   clock around a synchronised step, median.
Writes one JSON document (default profiles/particles.json)."""
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
from iamr_amd.particles import Particles

lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "particles.json")
hip = C.CDLL("libamdhip64.so")
stream = C.c_void_p(lib.lib().iamrx_stream())
BYTES_PER_PARTICLE = 2 * 24 * 8 + (9 + 12) * 8 + 16


def hipcheck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def event_ms(fn):
    e0, e1 = C.c_void_p(), C.c_void_p()
    hipcheck(hip.hipEventCreate(C.byref(e0))); hipcheck(hip.hipEventCreate(C.byref(e1)))
    hipcheck(hip.hipEventRecord(e0, stream))
    fn()
    hipcheck(hip.hipEventRecord(e1, stream))
    hipcheck(hip.hipEventSynchronize(e1))
    t = C.c_float()
    hipcheck(hip.hipEventElapsedTime(C.byref(t), e0, e1))
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return t.value


res = {"kernel": {}, "step": {}, "bytes_per_particle": BYTES_PER_PARTICLE}
nn, npart = 128, 1 << 20
n = (nn,) * 3
g = lib.Geom.make(n)
lay = lib.Layout.single(n)
rng = np.random.default_rng(0)
um = []
for d in range(3):
    idx = [np.mod(np.arange(-1, nn + (1 if e == d else 0) + 1) + (0.0 if e == d else 0.5), nn) * (2 * np.pi / nn) for e in range(3)]
    X, Y, Z = np.meshgrid(*idx, indexing="ij")
    f = 0.3 * np.cos(X + 2 * Y + d) * np.sin(Z - Y) + 0.2
    m = lib.MultiFab(lay, lib.face(d), 1, 1)
    m.from_numpy(f[..., None], 0)
    um.append(m)
x = rng.uniform(0, 1, (npart, 3))
cell = np.floor(x * nn).astype(np.int64)
order = np.argsort(cell[:, 0] + nn * (cell[:, 1] + nn * cell[:, 2]), kind="stable")
cases = {}
for name, pos in (("random", x), ("by_cell", x[order])):
    pc = Particles([g], [lay], 1)
    pc.add(pos)
    cases[name] = (pc, [])
dt = 0.2 / nn                                       # a fifth of a cell per call: the particles stay where their order put them
for name, (pc, ms) in cases.items():
    for _ in range(5):
        pc.advect(0, um, dt)
for _ in range(30):                                 # alternating: both sides see the same machine
    for name, (pc, ms) in cases.items():
        ms.append(event_ms(lambda: pc.advect(0, um, dt)))
for name, (pc, ms) in cases.items():
    med = statistics.median(ms)
    res["kernel"][name] = {"particles": npart, "box": nn, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                           "particles_per_s": npart / (med * 1e-3), "effective_GB_per_s": npart * BYTES_PER_PARTICLE / (med * 1e-3) / 1e9}
    print("advect", name, res["kernel"][name], flush=True)
# 1b. the sample kernel on the same sets
idx = [np.mod(np.arange(-1, nn + 1) + 0.5, nn) * (2 * np.pi / nn) for e in range(3)]
X, Y, Z = np.meshgrid(*idx, indexing="ij")
cell = lib.MultiFab(lay, lib.CELL, 5, 1)
cell.from_numpy(np.stack([0.3 * np.cos(X + 2 * Y + c) * np.sin(Z - Y) + 0.2 * c for c in range(5)], axis=-1), 0)
res["sample"] = {}
for M in (1, 5):
    comps = (C.c_int * M)(*range(M))
    launch = lambda pc: lib.check(lib.lib().iamrx_particles_sample(pc.h, 0, cell.h, M, comps, None, None, None))
    times = {name: [] for name in cases}
    for name, (pc, _) in cases.items():
        for _ in range(5):
            launch(pc)
    for _ in range(30):
        for name, (pc, _) in cases.items():
            times[name].append(event_ms(lambda: launch(pc)))
    for name, ms in times.items():
        med = statistics.median(ms)
        adv = res["kernel"][name]["ms_median"]
        res["sample"][f"{name}_M{M}"] = {"particles": npart, "box": nn, "components": M, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                                         "ns_per_particle": med * 1e6 / npart, "advect_ns_per_particle": adv * 1e6 / npart,
                                         "effective_GB_per_s": npart * (32 + 72 * M) / (med * 1e-3) / 1e9}
        print("sample", name, "M =", M, res["sample"][f"{name}_M{M}"], flush=True)
del cell
# 2. the redistribution of the same sets (nothing moves between boxes: placement, prefix, the one read-back, scatter), host clock around a
#    synchronised call
res["redistribute"] = {}
for _ in range(12):
    for name, (pc, ms) in cases.items():
        lib.sync()
        t0 = time.perf_counter()
        pc.redistribute()
        lib.sync()
        res["redistribute"].setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
for name, ts in list(res["redistribute"].items()):
    ts = ts[2:]
    res["redistribute"][name] = {"particles": npart, "ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
    print("redistribute", name, res["redistribute"][name], flush=True)
del cases, um

runs = {}
for name, on in (("without", 0), ("with_particles", 1)):
    ns = N.NavierStokes(g, lib.Layout.single(n), N.ns_params(cfl=0.7, visc_coef=1.0e-4))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 0.0, 1.0)
    ns.post_init(-1.0)
    if on:
        pc = Particles.for_level(ns)
        ns.set_particles(pc)
        pc.add(rng.uniform(0, 1, (nn ** 3 // 8, 3)))
    for _ in range(2):
        ns.step()
    lib.sync()
    runs[name] = (ns, [])
for _ in range(8):
    for name, (ns, ts) in runs.items():
        lib.sync()
        t0 = time.perf_counter()
        ns.step()
        lib.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
for name, (ns, ts) in runs.items():
    res["step"][name] = {"box": nn, "particles": nn ** 3 // 8 if name == "with_particles" else 0, "ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
    print("step", name, res["step"][name], flush=True)
res["step"]["added_ms"] = res["step"]["with_particles"]["ms_median"] - res["step"]["without"]["ms_median"]
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", out_path)
