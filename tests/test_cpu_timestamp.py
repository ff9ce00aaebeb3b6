"""CPU: the yardstick of the particle sample (tests/timestamp_numpy.py), the line format of the timestamp files and the inputs keys
(particles.do_timestamps, particles.timestamp_dir, particles.timestamp_indices).  No device needed."""
import os
import numpy as np
import pytest

import timestamp_numpy as tn
from iamr_amd.inputs import Inputs

HERE = os.path.dirname(os.path.abspath(__file__))
INP = os.path.join(HERE, "golden", "run_2d_particles", "regtest.inputs")
EPS = 2.0 ** -53

N = (12, 10, 8)
PLO = (-1.0, 0.0, 0.5)
DX = (0.25, 0.125, 0.2)
LO = (-1, -1, -1)                                   # one ghost layer around the box 0 .. N - 1


def _positions(rng, n):
    """inside the box, some within 1e-12 of its faces and on cell centres"""
    hi = [PLO[e] + N[e] * DX[e] for e in range(3)]
    x = rng.uniform(0.0, 1.0, (n, 3)) * (np.array(hi) - np.array(PLO)) + np.array(PLO)
    x[:10, 0] = PLO[0] + 1e-12
    x[10:20, 1] = hi[1] - 1e-12
    x[20:30, 2] = PLO[2] + (np.arange(10) % N[2] + 0.5) * DX[2]
    return x


def test_yardstick_reproduces_a_uniform_field_to_the_bit():
    fab = np.full(tuple(n + 2 for n in N) + (2,), 0.1)
    fab[..., 1] = -3.7e5
    v = tn.sample(fab, LO, _positions(np.random.default_rng(0), 400), PLO, DX, (0, 0, 0), [1, 0])
    assert np.all(v[:, 0] == -3.7e5) and np.all(v[:, 1] == 0.1)


def test_yardstick_reproduces_a_linear_field():
    """f = a + b x at the cell centres (ghost cells included): the interpolant is f at the particle.  Bound 16 2^-53 max|f|: the centres,
    the weight and the three stages each commit a few roundings on operands no larger than 2 max|f|"""
    a, b = 0.3, (1.7, -0.9, 0.45)
    for e in range(3):
        c = [PLO[q] + (np.arange(LO[q], LO[q] + N[q] + 2) + 0.5) * DX[q] for q in range(3)]
        X = np.meshgrid(*c, indexing="ij")[e]
        fab = (a + b[e] * X)[..., None]
        x = _positions(np.random.default_rng(1 + e), 400)
        v = tn.sample(fab, LO, x, PLO, DX, (0, 0, 0), [0])[:, 0]
        err = np.abs(v - (a + b[e] * x[:, e])).max()
        assert err <= 16.0 * EPS * np.abs(fab).max(), (e, err)


def test_yardstick_never_reads_outside_the_array():
    fab = np.arange(4 * 4 * 4, dtype=np.float64).reshape(4, 4, 4, 1)
    x = np.array([[1e30, -1e30, np.nan], [np.inf, 0.0, -np.inf]])
    v = tn.sample(fab, (0, 0, 0), x, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0, 0, 0), [0])
    assert v.shape == (2, 1) and v[0, 0] == fab[3, 0, 0, 0]


def test_regression_inputs_as_they_are_keep_the_keys_ignored():
    inp = Inputs([INP], ["amr.n_cell=32 32"])
    pr = inp.problem()
    assert {"particles.timestamp_dir", "particles.timestamp_indices"} <= set(inp.ignored)
    assert pr["particles"]["timestamp"] is None
    inp = Inputs([INP], ["amr.n_cell=32 32", "particles.do_timestamps=0"])
    assert inp.problem()["particles"]["timestamp"] is None and "particles.timestamp_dir" in inp.ignored


def test_do_timestamps_uses_the_keys():
    inp = Inputs([INP], ["amr.n_cell=32 32", "particles.do_timestamps=1"])
    pr = inp.problem()
    assert not {"particles.timestamp_dir", "particles.timestamp_indices", "particles.do_timestamps"} & set(inp.ignored)
    ts = pr["particles"]["timestamp"]
    assert ts["dir"] == "particle_dir"
    assert ts["indices"] == [2]                     # the file's index 1 (the 2-D y-velocity) is the slab's component 2
    # the 2-D map 0 -> 0, i -> i + 1, any number of indices
    ts = Inputs([INP], ["amr.n_cell=32 32", "particles.do_timestamps=1", "particles.timestamp_indices=3 0 2"]).problem()["particles"]["timestamp"]
    assert ts["indices"] == [4, 0, 3]
    # three dimensions: as they are; the default directory is upstream's
    ldc = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
    ts = Inputs([ldc], ["particles.do_nspc_particles=1", "particles.do_timestamps=1", "particles.timestamp_indices=4 1"]).problem()["particles"]["timestamp"]
    assert ts == dict(dir="Timestamps", indices=[4, 1])
    ts = Inputs([ldc], ["particles.do_nspc_particles=1", "particles.do_timestamps=1"]).problem()["particles"]["timestamp"]
    assert ts == dict(dir="Timestamps", indices=[])


def test_an_index_outside_the_state_raises_at_parse_time():
    ldc = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
    with pytest.raises(ValueError, match="timestamp_indices"):
        Inputs([ldc], ["particles.do_nspc_particles=1", "particles.do_timestamps=1", "particles.timestamp_indices=5"]).problem()
    with pytest.raises(ValueError, match="timestamp_indices"):
        Inputs([ldc], ["particles.do_nspc_particles=1", "particles.do_timestamps=1", "particles.timestamp_indices=0 -1"]).problem()
    ts = Inputs([ldc], ["particles.do_nspc_particles=1", "particles.do_timestamps=1", "particles.timestamp_indices=5", "ns.do_trac2=1",
                        "ns.scal_diff_coefs=0.0 0.0"]).problem()
    assert ts["particles"]["timestamp"]["indices"] == [5]
    with pytest.raises(ValueError, match="timestamp_indices"):      # the 2-D state has four components
        Inputs([INP], ["amr.n_cell=32 32", "particles.do_timestamps=1", "particles.timestamp_indices=4"]).problem()


def test_line_format():
    line = tn.format_line(12, 3, (0.5, -1.25, 1.0e-3), 0.125, (1.0, 0.0, -2.0e10), (7.0, 1.0 / 3.0))
    assert line == ("12 3 5.0000000000e-01 -1.2500000000e+00 1.0000000000e-03 1.2500000000e-01 1.0000000000e+00 0.0000000000e+00 "
                    "-2.0000000000e+10 7.0000000000e+00 3.3333333333e-01\n")
    assert tn.format_line(1, 0, (0.5, 0.25, 1.0), 2.0, (1.0, 0.0, -2.0)) == ("1 0 5.0000000000e-01 2.5000000000e-01 1.0000000000e+00 2.0000000000e+00 "
                                                                             "1.0000000000e+00 0.0000000000e+00 -2.0000000000e+00\n")
    # the two-dimensional form: the slab coordinate (direction 1) and r_1 are left out -- id cpu x y time u v value
    line = tn.format_line(4, 0, (0.5, 0.25, 1.0), 2.0, (1.0, 0.0, -2.0), (9.0,), fixed_dir=1)
    assert line == "4 0 5.0000000000e-01 1.0000000000e+00 2.0000000000e+00 1.0000000000e+00 -2.0000000000e+00 9.0000000000e+00\n"
    assert len(line.split(" ")) == 8
