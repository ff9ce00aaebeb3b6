"""Host-level cost of the named-field diagnostics (csrc/diagnostics.hip): what a call costs from Python, read-back included.
  python tools/bench_diagnostics.py [label] [out.txt]
Workloads: a 128^3 single level (TaylorGreen data), and the benchmark's two-level hierarchy at 128^3 (bench.py amr_workload: the base box
and one refined box over its central half).  Calls: histogram (64 bins, fixed ranges) and integrate of x_velocity density enstrophy
dissipation, derive_fields of the ten velocity-gradient names (on the hierarchy: of every level).  Every call is timed on the host clock
between two device synchronisations; 3 warm-up calls, then ROUNDS medians of CALLS calls each: the median of those medians and their
interquartile range (the run-to-run spread inside one session).  Appends the table to the output file (default
profiles/diagnostics_refactor.txt) under `label`."""
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iamr_amd import lib, ns as N
from iamr_amd.amr import Amr
from iamr_amd.pdf import VELGRAD_NAMES

WARM, CALLS, ROUNDS = 3, 20, 7
NAMES = ["x_velocity", "density", "enstrophy", "dissipation"]
RANGES = [(-1.0, 1.0), (0.5, 1.5), (0.0, 40.0), (0.0, 0.1)]
label = sys.argv[1] if len(sys.argv) > 1 else "this tree"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "diagnostics_refactor.txt")
lib.init(0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    for _ in range(WARM):
        fn()
    meds = []
    for _ in range(ROUNDS):
        t = []
        for _ in range(CALLS):
            lib.sync(); t0 = time.perf_counter()
            fn()
            lib.sync(); t.append((time.perf_counter() - t0) * 1e3)
        meds.append(statistics.median(t))
    q = statistics.quantiles(meds, n=4)
    return statistics.median(meds), q[2] - q[0], min(meds), max(meds)


def report(tag, run):
    say(f"  {tag}")
    cases = [("histogram, 4 names", lambda: run.histogram(NAMES, 64, RANGES)), ("integrate, 4 names", lambda: run.integrate(NAMES)),
             ("derive_fields, 10 names", lambda: [lev.derive_fields(VELGRAD_NAMES) for lev in run.levels])]
    for name, fn in cases:
        m, iqr, lo, hi = timed(fn)
        say(f"    {name:26s} {m:8.4f} ms   IQR {iqr:.4f}   (medians {lo:.4f} .. {hi:.4f})")


say(f"[{label}] diagnostics from Python, host clock between synchronisations: {WARM} warm-up calls, median of {ROUNDS} medians of {CALLS} calls, IQR of those medians")
n = (128,) * 3
params = N.ns_params(cfl=0.7, visc_coef=1e-4, init_iter=2)
ns = N.NavierStokes(lib.Geom.make(n), lib.Layout.single(n), params)
ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
report("128^3 single level", ns)
del ns
fine = ((64,) * 3, (191,) * 3)
amr = Amr(lib.Geom.make(n), [lib.Layout.single(n), lib.Layout([fine], [0])], params, lib.mg_opts())
for lev in amr.levels:
    lev.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
report("two levels: 128^3 and a 128^3 refined box over the central half (bench.py's hierarchy)", amr)
del amr
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n\n")
print("appended to", out_path)
