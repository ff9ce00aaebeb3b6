"""python tools/record_diagnostics_golden.py [path]: write what integrate, histogram, plane_profile and sum_integrated give for the two
fixtures of tests/test_gpu_diagnostics.py, in both box modes of the suite (floats as hex strings), to
tests/golden/diagnostics_parent.json or to `path`.  Run on the commit whose results are to be kept;
tests/test_gpu_diagnostics.py::test_against_the_parent_commit compares with the file bit by bit."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from iamr_amd import lib                    # noqa: E402
import test_gpu_diagnostics as T            # noqa: E402

lib.init(0)
commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
gold = dict(recorded=f"commit {commit or 'unknown'}, python tools/record_diagnostics_golden.py", names=T.MIXED, nbins=16,
            ranges=[list(T.RANGES[nm]) for nm in T.MIXED])
for mode, value in (("merged", "1"), ("kept", "0")):
    os.environ["IAMRX_COALESCE"] = value
    lib.tuning_set("COALESCE", float(value))
    assert T.box_mode() == mode
    gold[mode] = T.record_all()
path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN_FILE
with open(path, "w") as f:
    json.dump(gold, f, sort_keys=True, separators=(",", ":"))
    f.write("\n")
print("wrote", path, os.path.getsize(path), "bytes")
