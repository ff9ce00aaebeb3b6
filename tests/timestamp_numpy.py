"""numpy restatement of the particle sample (iamr_amd/csrc/k_particles.hip: k_part_sample) and of a timestamp line (Particles::timestamp).
Same expressions in the same order as the kernel: (x - plo) / dx - 0.5, floor, the clamp to the array, a + w (b - a) in x, then y, then z.
Division and subtraction are correctly rounded on both sides, so indices and weights are the kernel's to the bit; the three nested stages
may differ by the device's contraction of a + w (b - a) into a fused multiply-add.  Like the container this is UNPINNED against AMReX, whose
source is not in the reference tree."""
import numpy as np


def sample(fab, lo, xyz, plo, dx, dlo, comps):
    """fab: (n0, n1, n2, ncomp) array of one box whose first cell has the index lo (ghost cells included); xyz: (n, 3) positions;
    plo, dx: the level's problem low corner and cell sizes; dlo: the domain's low index -> (n, len(comps))"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    i0, i1, w = [], [], []
    for e in range(3):
        l = (xyz[:, e] - plo[e]) / dx[e] - 0.5
        l = np.where(np.isnan(l), -1.0e9, np.minimum(np.maximum(l, -1.0e9), 1.0e9))
        fl = np.floor(l)
        w.append(l - fl)
        a = fl.astype(np.int64) + dlo[e]
        b = a + 1
        flo, fhi = lo[e], lo[e] + fab.shape[e] - 1
        i0.append(np.clip(a, flo, fhi) - lo[e])
        i1.append(np.clip(b, flo, fhi) - lo[e])
    wx, wy, wz = w
    out = np.zeros((len(xyz), len(comps)))
    for m, c in enumerate(comps):
        F = fab[..., c]
        f000, f100 = F[i0[0], i0[1], i0[2]], F[i1[0], i0[1], i0[2]]
        f010, f110 = F[i0[0], i1[1], i0[2]], F[i1[0], i1[1], i0[2]]
        f001, f101 = F[i0[0], i0[1], i1[2]], F[i1[0], i0[1], i1[2]]
        f011, f111 = F[i0[0], i1[1], i1[2]], F[i1[0], i1[1], i1[2]]
        a00, a10 = f000 + wx * (f100 - f000), f010 + wx * (f110 - f010)
        a01, a11 = f001 + wx * (f101 - f001), f011 + wx * (f111 - f011)
        b0, b1 = a00 + wy * (a10 - a00), a01 + wy * (a11 - a01)
        out[:, m] = b0 + wz * (b1 - b0)
    return out


def format_line(pid, cpu, xyz, time, r, values=(), fixed_dir=-1):
    """`id cpu x y z time r0 r1 r2 v_0 ..`: single blanks, reals as %.10e, a newline; with fixed_dir = d coordinate d and r_d are left out"""
    reals = [xyz[e] for e in range(3) if e != fixed_dir] + [time] + [r[e] for e in range(3) if e != fixed_dir] + list(values)
    return " ".join(["%d" % pid, "%d" % cpu] + ["%.10e" % float(v) for v in reals]) + "\n"


def parse_file(path):
    """-> (n_lines, n_fields) float array of a timestamp file"""
    with open(path) as f:
        rows = [[float(t) for t in line.split(" ")] for line in f.read().split("\n") if line]
    return np.array(rows, dtype=np.float64)
