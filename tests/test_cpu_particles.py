"""Tracer particles without a GPU: the numpy yardstick (tests/particles_numpy.py) on closed-form trajectories, the particles.* inputs keys on
the reference's two-dimensional particle regression test (tests/golden/run_2d_particles, copied byte for byte), the derive-name order, and
the particle files.  The container's arithmetic belongs to AMReX, which is not in the reference tree: unpinned."""
import os
import numpy as np
import pytest

import particles_numpy as pn
from iamr_amd.inputs import Inputs
from iamr_amd import particles as P
from iamr_amd.plotfile import plot_selection, state_names, DERIVE_NAMES, PARTICLE_DERIVE_NAMES

HERE = os.path.dirname(os.path.abspath(__file__))
RUN2D = os.path.join(HERE, "golden", "run_2d_particles")
INP = os.path.join(RUN2D, "regtest.inputs")
EPS = 2.0 ** -53

N = (12, 10, 8)
PLO, PHI = (-1.0, 0.0, 0.5), (2.0, 2.5, 2.5)
DX = tuple((PHI[e] - PLO[e]) / N[e] for e in range(3))


def _faces(fn):
    """face arrays over indices -2 .. n + type + 1 sampled from fn(d, x, y, z)"""
    out, lo = [], []
    for d in range(3):
        c = [PLO[e] + (np.arange(-2, N[e] + (1 if e == d else 0) + 2) + (0.0 if e == d else 0.5)) * DX[e] for e in range(3)]
        X, Y, Z = np.meshgrid(*c, indexing="ij")
        out.append(fn(d, X, Y, Z))
        lo.append((-2, -2, -2))
    return out, lo


def _positions(n=400):
    rng = np.random.default_rng(0)
    return np.array(PLO) + rng.uniform(0.05, 0.95, (n, 3)) * (np.array(PHI) - np.array(PLO))


def test_yardstick_uniform_field_moves_by_dt_u():
    U = (0.75, -0.5, 0.25)
    um, lo = _faces(lambda d, X, Y, Z: np.full(X.shape, U[d]))
    x = _positions()
    dt = 0.125
    xn, r, live = pn.advect(x, np.arange(1, len(x) + 1), um, lo, dt, PLO, DX, (0, 0, 0), tuple(n - 1 for n in N), (1, 1, 1))
    assert live.all()
    # a + w (b - a) of a constant is the constant, so v = U and x_new = x + dt U: exactly, one rounding of the sum
    assert np.array_equal(xn, x + dt * np.array(U)) and np.array_equal(r, np.broadcast_to(U, x.shape))
    U2 = (0.1, 1.0 / 3.0, -0.7)                               # nothing about U or dt has to be exact in binary
    um2, _ = _faces(lambda d, X, Y, Z: np.full(X.shape, U2[d]))
    xn2, r2, _ = pn.advect(x, np.ones(len(x), int), um2, lo, 0.3, PLO, DX, (0, 0, 0), tuple(n - 1 for n in N), (1, 1, 1))
    assert np.array_equal(xn2, x + 0.3 * np.array(U2)) and np.array_equal(r2, np.broadcast_to(U2, x.shape))


def test_yardstick_linear_field_is_reproduced():
    A = np.array([[0.3, -0.2, 0.1], [0.15, 0.25, -0.3], [-0.1, 0.2, 0.05]])
    b = np.array([0.4, -0.3, 0.2])
    um, lo = _faces(lambda d, X, Y, Z: A[d, 0] * X + A[d, 1] * Y + A[d, 2] * Z + b[d])
    x = _positions()
    dt = 0.2
    xn, r, _ = pn.advect(x, np.ones(len(x), int), um, lo, dt, PLO, DX, (0, 0, 0), tuple(n - 1 for n in N), (1, 1, 1))
    half = x + 0.5 * dt * (x @ A.T + b)
    exact = x + dt * (half @ A.T + b)
    # trilinear interpolation reproduces a linear field: the difference is rounding (~30 operations on numbers <= max|x| + max|u|)
    assert np.abs(xn - exact).max() <= 64 * EPS * (np.abs(x).max() + np.abs(um[0]).max())
    assert np.abs(r - (half @ A.T + b)).max() <= 64 * EPS * (np.abs(x).max() + np.abs(um[0]).max())


def test_yardstick_skips_invalid_and_clamps_at_walls():
    um, lo = _faces(lambda d, X, Y, Z: X + 0.0 * Y)
    for d in range(3):
        um[d][:2] = 1e30                                     # beyond the low x wall: never read
    x = np.array([[PLO[0] + 0.1 * DX[0], 1.0, 1.0], [0.5, 1.0, 1.0]])
    xn, r, live = pn.advect(x, np.array([1, 0]), um, lo, 0.01, PLO, DX, (0, 0, 0), tuple(n - 1 for n in N), (0, 1, 1))
    assert list(live) == [True, False] and np.array_equal(xn[1], x[1]) and np.all(np.abs(xn[0]) < 10)
    # the transverse components take the first cell's value inside the last half cell
    assert abs(r[0, 1] - (PLO[0] + 0.5 * DX[0])) <= 4 * EPS


def test_yardstick_redistribute_and_counts():
    levels = [dict(n=(8, 8, 8), dlo=(0, 0, 0), dx=(0.125,) * 3, boxes=[((0, 0, 0), (3, 7, 7)), ((4, 0, 0), (7, 7, 7))]),
              dict(n=(16, 16, 16), dlo=(0, 0, 0), dx=(0.0625,) * 3, boxes=[((4, 4, 4), (11, 11, 11))])]
    lo, hi, per = (0.0,) * 3, (1.0,) * 3, (1, 1, 0)
    x = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.5, 0.5, 0.5], [1.0, -0.25, 0.3], [0.3, 0.3, 1.0], [0.24, 0.5, 0.5], [0.5, 0.5, 0.5]])
    ids = np.array([1, 2, 3, 4, 5, 6, 0])
    xo, lev, box, st = pn.redistribute(x, ids, np.zeros(7, int), np.zeros(7, int), levels, lo, hi, per, 0, 1, 0)
    assert list(st) == [0, 0, 0, 0, 1, 0, 3]
    assert list(lev[:4]) == [0, 0, 1, 0] and list(box[:4]) == [0, 1, 0, 0] and lev[5] == 0
    assert np.array_equal(xo[3], [0.0, 0.75, 0.3])           # x = prob_hi wraps to prob_lo
    # one fine cell outside the patch: stays on level 1 with ngrow = 1, cannot be placed there with ngrow = 0
    keep = np.array([5])
    xo1, lev1, box1, st1 = pn.redistribute(x[keep], ids[keep], np.array([1]), np.array([0]), levels, lo, hi, per, 1, 1, 1)
    assert st1[0] == 0 and lev1[0] == 1 and box1[0] == 0 and np.array_equal(xo1, x[keep])
    assert pn.redistribute(x[keep], ids[keep], np.array([1]), np.array([0]), levels, lo, hi, per, 1, 1, 0)[3][0] == 2
    live = st == 0
    c0 = pn.particle_count(xo[live], lev[live], box[live], levels, lo, 0)
    c1 = pn.particle_count(xo[live], lev[live], box[live], levels, lo, 1)
    t0 = pn.total_particle_count(xo[live], lev[live], box[live], levels, lo, 0)
    assert c0.sum() == 4 and c1.sum() == 1 and c1[8, 8, 8] == 1 and t0.sum() == 5 and t0[4, 4, 4] == 1 and t0[0, 0, 0] == 1


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def test_golden_files_are_the_reference_regression_test():
    with open(os.path.join(RUN2D, "particle_file")) as f:
        lines = f.read().split("\n")
    assert lines[0] == "30" and len([l for l in lines[1:] if l.strip()]) == 30
    with open(INP) as f:
        txt = f.read()
    assert "particles.particle_init_file = particle_file" in txt and "particles.particles_in_plotfile = true" in txt


def test_particle_keys_of_the_regression_inputs():
    inp = Inputs([INP], ["amr.n_cell=32 32"])
    pr = inp.problem()
    pp = pr["particles"]
    assert pp is not None and pp["init_file"] == os.path.join(RUN2D, "particle_file") and pp["in_plotfile"] == 1
    assert pp["restart_file"] == "" and pp["output_file"] == "" and pp["restart_from_nonparticle_chkfile"] == 0 and pp["verbose"] == 0
    assert {"particles.timestamp_dir", "particles.timestamp_indices"} <= set(inp.ignored)
    assert pr["slab"] == 8 and pr["n"] == [32, 8, 32] and pr["prob_hi"][1] == 0.5
    # the 2-D lift of the 30 positions: (x, y) -> (x, mid-slab, y)
    x = P.read_particle_file(pp["init_file"], 0.5 * (pr["prob_lo"][1] + pr["prob_hi"][1]))
    assert x.shape == (30, 3) and np.all(x[:, 1] == 0.25)
    assert np.array_equal(x[:10, 0], [-0.8, -0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6, 0.8, 1.0]) and np.array_equal(x[10:20, 2], [-0.30] * 10)
    # x = 1.0 = prob_hi wraps to -1.0 (the yardstick's wrap is the kernel's)
    w = pn.wrap(x[:, 0], pr["prob_lo"][0], pr["prob_hi"][0])
    assert np.array_equal(w[x[:, 0] == 1.0], [-1.0, -1.0, -1.0]) and np.array_equal(w[x[:, 0] != 1.0], x[x[:, 0] != 1.0, 0])
    with pytest.raises(ValueError):
        P.read_particle_file(pp["init_file"])                # two-dimensional positions need the slab


def test_particle_key_handling():
    base = [INP], ["amr.n_cell=32 32"]
    assert Inputs(base[0], base[1] + ["particles.do_nspc_particles=0"]).problem()["particles"] is None     # off whatever else is named
    assert Inputs(base[0], base[1] + ["particles.particles_in_plotfile=0"]).problem()["particles"]["in_plotfile"] == 0
    ldc = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
    assert Inputs([ldc]).problem()["particles"] is None                                                    # no particles.* key: none
    pp = Inputs([ldc], ["particles.do_nspc_particles=1", "particles.verbose=1", "particles.particle_output_file=out.txt",
                        "particles.restart_from_nonparticle_chkfile=1"]).problem()["particles"]
    assert pp["init_file"] == "" and pp["verbose"] == 1 and pp["output_file"] == "out.txt" and pp["restart_from_nonparticle_chkfile"] == 1
    pp = Inputs([ldc], ["particles.particle_restart_file=/abs/more"]).problem()["particles"]
    assert pp["restart_file"] == "/abs/more"
    with pytest.raises(KeyError):
        Inputs([ldc], ["particles.nonsense=1"]).problem()
    with pytest.raises(ValueError):
        Inputs([ldc], ["particles.pverbose=1"]).problem()    # NavierStokesBase.cpp:3786-3788 aborts


def test_derive_name_order():
    st = state_names()
    assert PARTICLE_DERIVE_NAMES == ["particle_count", "total_particle_count"]
    assert plot_selection(st, "ALL", "ALL", particles=True)[1] == DERIVE_NAMES + PARTICLE_DERIVE_NAMES      # after avg_pressure
    assert plot_selection(st, "ALL", "ALL", averaging=True, particles=True)[1][-3:] == ["avg_pressure"] + PARTICLE_DERIVE_NAMES
    assert plot_selection(st, "ALL", ["total_particle_count", "energy"], particles=True)[1] == ["total_particle_count", "energy"]
    assert plot_selection(st, "ALL", "ALL")[1] == DERIVE_NAMES
    with pytest.raises(ValueError):
        plot_selection(st, "ALL", ["particle_count"])        # not known without particles


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _awkward(n=57):
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-1, 1, (n, 3)) * 10.0 ** rng.integers(-12, 3, (n, 3))
    xyz[0] = (np.nextafter(1.0, 0.0), -0.0, 5e-324)
    r = rng.standard_normal((n, 3))
    ids = rng.permutation(np.arange(1, n + 1)).astype(np.int32)
    cpu = rng.integers(0, 4, n).astype(np.int32)
    return xyz, r, ids, cpu


def test_particles_directory_round_trip(tmp_path):
    xyz, r, ids, cpu = _awkward()
    d = P.write_particles_dir(str(tmp_path), xyz, r, ids, cpu, 99)
    assert os.path.basename(d) == "Particles" and sorted(os.listdir(d)) == ["Header", "cpu.i32", "id.i32", "r.f64", "xyz.f64"]
    back = P.read_particles_dir(str(tmp_path))
    o = np.argsort(ids)
    assert back["next_id"] == 99 and np.array_equal(back["id"], ids[o]) and np.array_equal(back["cpu"], cpu[o])
    assert back["xyz"].tobytes() == xyz[o].tobytes() and back["r"].tobytes() == r[o].tobytes()            # bit for bit, -0.0 and denormals too
    assert open(os.path.join(d, "xyz.f64"), "rb").read() == xyz[o].astype("<f8").tobytes()                 # raw little-endian
    P.write_particles_dir(str(tmp_path / "empty"), np.zeros((0, 3)), np.zeros((0, 3)), [], [], 1)
    assert len(P.read_particles_dir(str(tmp_path / "empty"))["id"]) == 0
    with open(os.path.join(d, "Header"), "w") as f:
        f.write("something else\n")
    with pytest.raises(ValueError):
        P.read_particles_dir(str(tmp_path))


def test_ascii_output_round_trip(tmp_path):
    xyz, r, ids, cpu = _awkward()
    path = str(tmp_path / "particles.txt")
    P.write_ascii(path, xyz, ids, cpu)
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == str(len(ids)) and [int(l.split()[3]) for l in lines[1:-1]] == sorted(ids)            # sorted by id
    x2, i2, c2 = P.read_ascii(path)
    o = np.argsort(ids)
    assert x2.tobytes() == xyz[o].tobytes() and np.array_equal(i2, ids[o]) and np.array_equal(c2, cpu[o])  # %.17g round-trips doubles


def test_three_dimensional_particle_file(tmp_path):
    p = tmp_path / "pf"
    p.write_text("2\n0.1 0.2 0.3\n-1e-3 4 5.5 \n")
    assert np.array_equal(P.read_particle_file(str(p)), [[0.1, 0.2, 0.3], [-1e-3, 4.0, 5.5]])
    with pytest.raises(ValueError):
        P.read_particle_file(str(p), 0.25)
    p.write_text("3\n0.1 0.2 0.3\n")
    with pytest.raises(ValueError):
        P.read_particle_file(str(p))
