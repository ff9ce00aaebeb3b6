"""The text file of a run's volume integrals of named fields (ns.integrate_interval / ns.integrate_vars / ns.integrate_file, inputs.py; the
sums: NavierStokes.integrate / Amr.integrate): a header line `# step time name1 ... namen`, then one row `step time v1 ... vn` per
output, reals with 17 significant digits (they read back to the bit).  Host-only code."""
import os
import numpy as np


def header_line(names):
    return "# step time " + " ".join(names)


def start_file(path, names, append=False):
    """a fresh file with its header line; append (a restarted run): an existing file is kept and must carry the same names"""
    if append and os.path.exists(path):
        with open(path) as f:
            first = f.readline().rstrip("\n")
        if first != header_line(names):
            raise ValueError(f"integrals: {path} holds '{first}', this run writes '{header_line(names)}'")
        return
    with open(path, "w") as f:
        f.write(header_line(names) + "\n")


def append_row(path, names, step, time, values):
    values = [float(v) for v in values]
    if len(values) != len(names):
        raise ValueError(f"integrals: {len(values)} values for the {len(names)} names {' '.join(names)}")
    if not os.path.exists(path):
        start_file(path, names)
    with open(path, "a") as f:
        f.write(f"{int(step)} {float(time):.17g} " + " ".join(f"{v:.17g}" for v in values) + "\n")


def read_integrals(path):
    """the columns of the file: {"names" (tuple), "step" (int64), "time" (float64), and every name -> float64 array, one entry per row}"""
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if not lines or not lines[0].startswith("# step time"):
        raise ValueError(f"integrals: {path} does not start with the header line '# step time <names>'")
    names = tuple(lines[0].split()[3:])
    rows = [ln.split() for ln in lines[1:] if not ln.startswith("#")]
    for r in rows:
        if len(r) != 2 + len(names):
            raise ValueError(f"integrals: {path}: a row holds {len(r)} columns, the header names {2 + len(names)}")
    out = dict(names=names, step=np.array([int(r[0]) for r in rows], dtype=np.int64), time=np.array([float(r[1]) for r in rows], dtype=np.float64))
    for q, nm in enumerate(names):
        out[nm] = np.array([float(r[2 + q]) for r in rows], dtype=np.float64)
    return out
