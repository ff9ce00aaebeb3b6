"""Plane-averaged profiles of the state along one axis (include/iamrx.h: iamrx_ns_plane_profile / iamrx_amr_plane_profile; kernels in
csrc/k_profile.hip): the names of the quantities, the dict the Python layer hands out, the Reynolds stresses formed from one, and the
text file the driver writes (ns.profile_interval, inputs.py) with its reader.  Pure numpy: nothing here touches the library."""
import numpy as np

# the quantities in the library's order; "one" is the uncovered volume fraction of the slab (1 on a proper hierarchy)
NAMES = ("one", "u", "v", "w", "rho", "c", "uu", "vv", "ww", "uv", "uw", "vw", "rhorho", "cc")


def as_dict(out, nbins, prob_lo, prob_hi, dir, bin_level):
    """the library's out[q * nbins + b] -> {name: array of nbins, "coord": bin centres in physical units, "names": NAMES, "dir", "bin_level"}"""
    a = np.asarray(out, dtype=np.float64).reshape(len(NAMES), nbins)
    p = {n: a[q].copy() for q, n in enumerate(NAMES)}
    h = (float(prob_hi) - float(prob_lo)) / nbins
    p["coord"] = float(prob_lo) + (np.arange(nbins) + 0.5) * h
    p["names"] = NAMES
    p["dir"] = int(dir)
    p["bin_level"] = int(bin_level)
    return p


def reynolds_stresses(profile):
    """<u_i' u_j'> = <u_i u_j> - <u_i><u_j> per bin and the variances of rho and c -> dict with the keys uu vv ww uv uw vw rhorho cc"""
    m = {k: np.asarray(profile[k], dtype=np.float64) for k in NAMES}
    out = {a + b: m[a + b] - m[a] * m[b] for a, b in (("u", "u"), ("v", "v"), ("w", "w"), ("u", "v"), ("u", "w"), ("v", "w"))}
    out["rhorho"] = m["rhorho"] - m["rho"] * m["rho"]
    out["cc"] = m["cc"] - m["c"] * m["c"]
    return out


def write_profile(path, profile, step, time):
    """header lines beginning with '#' (step, time, dir, bin level, column names), then one line per bin: the coordinate and the 14
    means with 17 significant digits (a double survives the round trip)"""
    cols = ("coord",) + NAMES
    with open(path, "w") as f:
        f.write("# step = %d\n# time = %.17g\n# dir = %d\n# bin_level = %d\n" % (int(step), float(time), int(profile["dir"]), int(profile["bin_level"])))
        f.write("# columns = " + " ".join(cols) + "\n")
        for b in range(len(profile["coord"])):
            f.write(" ".join("%.17g" % float(profile[c][b]) for c in cols) + "\n")


def read_profile(path):
    """the dict write_profile was given (arrays of float64, "names", "dir", "bin_level") plus "step" and "time" """
    head, rows = {}, []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                k, _, v = line[1:].partition("=")
                head[k.strip()] = v.strip()
            elif line.strip():
                rows.append([float(x) for x in line.split()])
    cols = head["columns"].split()
    a = np.array(rows, dtype=np.float64).reshape(len(rows), len(cols))
    p = {c: a[:, q].copy() for q, c in enumerate(cols)}
    p["names"] = tuple(cols[1:])
    p["step"], p["time"] = int(head["step"]), float(head["time"])
    p["dir"], p["bin_level"] = int(head["dir"]), int(head["bin_level"])
    return p
