"""CPU: the host side of the on-the-fly velocity statistics and the integrated quantities -- inputs keys (ns.avg_interval,
ns.compute_fluctuations, ns.avg_in_checkpoint, ns.sum_interval; NavierStokesBase.cpp:452, 487-488, 539), the plotfile's derive list with
"velocity_average" (NS_setup.cpp:412-431), the TimeAverage file of a checkpoint (NavierStokesBase.cpp:863-888, 2505-2518) and the three
printed lines (NavierStokes.cpp:1075-1078).  No GPU."""
import os
import numpy as np
import pytest

from iamr_amd.inputs import Inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SIX = ["x_vel_average", "y_vel_average", "z_vel_average", "x_vel_rms", "y_vel_rms", "z_vel_rms"]      # NS_setup.cpp:417-427


def test_defaults_are_off():
    """upstream's defaults (NavierStokesBase.cpp:109, 151-152): no averages, no fluctuations, averages expected in a checkpoint, no sums"""
    p = Inputs([os.path.join(GOLD, "inputs.3d.taylorgreen")]).problem()["params"]
    assert (p["avg_interval"], p["compute_fluctuations"], p["avg_in_checkpoint"], p["sum_interval"]) == (0, 0, 1, -1)


def test_keys_map_into_params():
    inp = Inputs([os.path.join(GOLD, "inputs.3d.taylorgreen")],
                 ["ns.avg_interval=3", "ns.compute_fluctuations=1", "ns.avg_in_checkpoint=0", "ns.sum_interval=2"])
    p = inp.problem()["params"]
    assert (p["avg_interval"], p["compute_fluctuations"], p["avg_in_checkpoint"], p["sum_interval"]) == (3, 1, 0, 2)
    assert not [k for k in inp.ignored if k.startswith("ns.avg") or k in ("ns.sum_interval", "ns.compute_fluctuations")]


def test_sum_interval_is_no_longer_ignored():
    inp = Inputs([os.path.join(GOLD, "inputs.3d.lid_driven_cavity16")], ["ns.sum_interval=1"])
    pr = inp.problem()
    assert pr["params"]["sum_interval"] == 1 and "ns.sum_interval" not in inp.ignored


def test_fixture_file():
    inp = Inputs([os.path.join(GOLD, "inputs.3d.taylorgreen_stats16")])
    pr = inp.problem()
    p = pr["params"]
    assert pr["n"] == [16, 16, 16] and p["visc_coef"] > 0 and pr["prob"]["probtype"] == 11
    assert (p["avg_interval"], p["compute_fluctuations"], p["sum_interval"]) == (1, 1, 1)
    assert pr["derive_plot_vars"] == ["velocity_average", "energy"] and not inp.ignored


def test_negative_avg_interval_raises():
    with pytest.raises(ValueError):
        Inputs([os.path.join(GOLD, "inputs.3d.taylorgreen")], ["ns.avg_interval=-1"]).problem()


def test_two_dimensional_inputs_with_averages_raise():
    f = os.path.join(GOLD, "inputs.2d.doubleshearlayer_c3")
    Inputs([f]).problem()                                          # the file itself is fine
    Inputs([f], ["ns.sum_interval=1"]).problem()                   # sums on a slab are (plane integrals)
    with pytest.raises(NotImplementedError):
        Inputs([f], ["ns.avg_interval=1"]).problem()


def test_plot_selection_with_averages():
    from iamr_amd.plotfile import plot_selection, state_names, DERIVE_NAMES, VEL_AVG_NAMES
    st = state_names()
    assert VEL_AVG_NAMES == SIX
    assert plot_selection(st, "ALL", "ALL", averaging=True) == (list(range(5)), SIX + DERIVE_NAMES)          # declared before "energy"
    assert plot_selection(st, "ALL", ["velocity_average", "energy"], averaging=True)[1] == SIX + ["energy"]
    assert plot_selection(st, "ALL", ["mag_vort"], averaging=True)[1] == ["mag_vort"]
    assert plot_selection(st, "ALL", "NONE", averaging=True)[1] == []


def test_plot_selection_without_averages_is_unchanged():
    from iamr_amd.plotfile import plot_selection, state_names, DERIVE_NAMES
    st = state_names()
    assert DERIVE_NAMES == ["energy", "mag_vort", "avg_pressure"]
    assert plot_selection(st, "ALL", "ALL") == (list(range(5)), DERIVE_NAMES)
    assert plot_selection(st, ["density"], ["mag_vort", "energy"]) == ([3], ["mag_vort", "energy"])
    with pytest.raises(ValueError):
        plot_selection(st, "ALL", ["velocity_average"])
    with pytest.raises(ValueError):
        plot_selection(st, "ALL", ["velocity_average"], averaging=False)
    with pytest.raises(ValueError):
        plot_selection(st, "ALL", ["x_vel_average"], averaging=True)            # the components are not quantities of their own


def test_time_average_file_round_trip(tmp_path):
    from iamr_amd import checkpoint
    d = str(tmp_path)
    for ta, tf in ((0.1 + 0.2, 1.0 / 3.0), (0.0, 0.0), (1.2345678901234567e-5, 0.0), (np.nextafter(1.0, 2.0), 7.0e10 / 3.0)):
        checkpoint.write_time_average(d, ta, tf)
        lines = open(os.path.join(d, "TimeAverage")).read().split("\n")
        assert lines[0] == "Writing time_average to checkpoint" and len(lines) == 4 and lines[3] == ""
        assert checkpoint.read_time_average(d) == (ta, tf)                       # 17 significant digits carry a double exactly


def test_sum_lines_parse_back():
    from iamr_amd.run import sum_lines
    sums = (1.0 / 3.0, -2.0e-17 / 7.0, 12345.678901234567)
    L = sum_lines(0.1 + 0.2, sums)
    assert [l.split("= ")[0] for l in L] == ["TIME"] * 3
    for l, name, v in zip(L, ("MASS", "TRAC", "KINETIC ENERGY"), sums):
        t, rest = l[len("TIME= "):].split(" ", 1)
        assert rest.startswith(name + "= ")
        assert float(t) == float(f"{0.1 + 0.2:.12g}") and abs(float(rest[len(name) + 2:]) - v) <= 5e-12 * abs(v)      # 12 significant digits
    # a two-dimensional run on its slab: the plane integrals
    L2 = sum_lines(0.0, (8.0, 4.0, 2.0), dict(slab=8, prob_lo=[0.0, 0.0, 0.0], prob_hi=[1.0, 0.25, 1.0]))
    assert [float(l.rsplit("= ", 1)[1]) for l in L2] == [32.0, 16.0, 8.0]
