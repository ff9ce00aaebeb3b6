"""The slab-decomposed transform of the spectra (csrc/k_spectrum.hip, SPECTRUM_DIST = 1): what ONE rank of R runs for one transform.
  python tools/bench_spectrum_slab.py [out.txt] [n]
One GPU cannot time the links, so this measures the kernels and counts the traffic.  For n^3 (default 256) and R = 2, 4, 8, in this one
process and this one run:
  - the passes of iamrx_spectrum_slab_bench -- scatter, x, y, pack, unpack, z, pack, unpack, shell sums on arena buffers of the
    per-rank shapes, the exchanges left out -- and k_spec_expand over N / R elements as the streaming yardstick (8 B read, 16 B
    written per element): HIP events between the passes on the library's stream; warm-up first, then the median of the repeats with
    their minimum and maximum;
  - the five one-rank passes of iamrx_spectrum_bench on one n^3 box, the yardstick the rank's summed time is set against (1 / R of it);
  - counted, not measured: the doubles a rank sends per plain transform and per packed pair against the N doubles the gather all-reduces.
Writes the table (default profiles/spectrum_slab_bench.txt)."""
import ctypes as C
import os
import statistics
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib
from iamr_amd.spectrum import SLAB_BENCH_PASSES

WARM, REPS = 5, 30
# bytes per element of N / R a pass moves at the least: the scatter reads 8 and writes 16, a transform pass and a full transpose kernel
# read and write 16 (the unpack moves (R - 1) / R of the slab: the own block went with the pack), the shell sums read 16, expand 8 + 16
BYTES = dict(scatter=24.0, x=32.0, y=32.0, pack_zy=32.0, unpack_zy=32.0, z=32.0, pack_yz=32.0, unpack_yz=32.0, shell_sums=16.0, expand=24.0)
lib.init(0)
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spectrum_slab_bench.txt")
nn = int(sys.argv[2]) if len(sys.argv) > 2 else 256
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return statistics.median(v), min(v), max(v)


n = (nn,) * 3
N = nn ** 3
g = lib.Geom.make(n)
say(f"slab-decomposed transform, {nn}^3: {WARM} warm-up repeats, median of {REPS}; one process, exchanges left out")
# the one-rank passes, same process
mf = lib.MultiFab(lib.Layout.single(n), lib.CELL, 1, 0)
mf.from_numpy(np.random.default_rng(1).standard_normal(n + (1,)) + 0.3, 0)
ms1 = (C.c_float * (5 * (WARM + REPS)))()
lib.check(lib.lib().iamrx_spectrum_bench(C.byref(g), mf.h, 0, WARM + REPS, ms1))
one = [med([ms1[5 * r + p] for r in range(WARM, WARM + REPS)]) for p in range(5)]
one_total = sum(m[0] for m in one)
for name, m in zip(("pack", "x", "y", "z", "shell sums"), one):
    say(f"  one rank      {name:12s} {m[0]:8.4f} ms (min {m[1]:.4f}, max {m[2]:.4f})")
say(f"  one rank      {'sum':12s} {one_total:8.4f} ms")
del mf
for R in (2, 4, 8):
    ms = lib.spectrum_slab_bench(g, R, WARM + REPS)[WARM:]
    share = N // R
    col = {name: med([float(v) for v in ms[:, p]]) for p, name in enumerate(SLAB_BENCH_PASSES)}
    rate = {name: BYTES[name] * share * ((R - 1) / R if name.startswith("unpack") else 1.0) / (col[name][0] * 1e-3) for name in col}
    say(f"R = {R}: N / R = {share} modes per rank")
    for name in SLAB_BENCH_PASSES:
        m = col[name]
        tail = f"  {100 * rate[name] / rate['expand']:5.1f} % of expand's rate" if "pack" in name else ""
        say(f"  rank of {R}     {name:12s} {m[0]:8.4f} ms (min {m[1]:.4f}, max {m[2]:.4f})  {rate[name] / 1e12:5.2f} TB/s{tail}")
    total = sum(col[name][0] for name in SLAB_BENCH_PASSES if name != "expand")
    say(f"  rank of {R}     {'sum':12s} {total:8.4f} ms against one rank / R = {one_total / R:.4f} ms: {total / (one_total / R):.2f} x")
    # counted: the doubles a rank sends.  Scatter: at most its N / R cells (boxes nowhere on their own slab), 0 for boxes that lie in
    # their owner's slab; transposes 2 * 2 (R - 1) N / R^2; mirror of a pair at most 2 N / R
    T = 2 * (R - 1) * N // R ** 2
    say(f"  counted: a rank sends per plain transform 2 T = {2 * T} doubles in the transposes (T = 2 (R - 1) N / R^2) and 0 .. N / R = {share} in the "
        f"scatter: {2 * T / N:.3f} .. {(2 * T + share) / N:.3f} N; per packed pair 2 T + mirror (<= 2 N / R) + two scatters: "
        f"{2 * T / N:.3f} .. {(2 * T + 4 * share) / N:.3f} N; the gather all-reduces N = {N} doubles per field ({2 * N} per pair) on every rank")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
