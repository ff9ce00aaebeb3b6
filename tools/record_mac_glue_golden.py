"""python tools/record_mac_glue_golden.py [path]: write what diffuse_tensor_velocity gives for the two fixtures of
tests/test_gpu_mac_glue.py (a sample of the solution, cycles, residual norm; one row per fixture) to
tests/golden/mac_glue_tensor_velocity.npy or to `path`.  Run on the commit whose results are to be kept;
tests/test_gpu_mac_glue.py::test_viscous_solve_keeps_its_numbers compares with the file bit by bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from iamr_amd import lib                    # noqa: E402
import test_gpu_mac_glue as T               # noqa: E402

lib.init(0)
lib.tuning_set("CHECK_UNIFORM", 1)          # as the suite's fixture sets it
rows = np.stack([T.tensor_velocity(lib, case) for case in T.TENSOR_CASES])
path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
np.save(path, rows)
print("wrote", path, rows.shape, os.path.getsize(path), "bytes; cycles", rows[:, -4], "levels", rows[:, -1])
