"""Host side of the velocity-gradient derived fields (diveru, vort_x/y/z, enstrophy, strain_rate, dissipation, q_criterion, r_invariant,
helicity): the names in plotfile.plot_selection, pdf.DERIVED_NAMES and the inputs parser, the ns.integrate_* keys, the text file of the
integrals and the declarations of the C-ABI.  No GPU."""
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FORCED = os.path.join(GOLD, "inputs.3d.forced")
LES = os.path.join(GOLD, "inputs.3d.LES_hotspot")
TG = os.path.join(GOLD, "inputs.3d.taylorgreen")
DSL2D = os.path.join(GOLD, "inputs.2d.doubleshearlayer_c3")
TEN = ["diveru", "vort_x", "vort_y", "vort_z", "enstrophy", "strain_rate", "dissipation", "q_criterion", "r_invariant", "helicity"]
STATE = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer"]


def test_tutorial_inputs_need_no_override():
    """the file's own amr.derive_plot_vars = mag_vort diveru avg_pressure goes through"""
    from iamr_amd.inputs import Inputs
    from iamr_amd import run as R
    pr = Inputs([FORCED]).problem()
    names, der, kept = R.plot_names_and_filter(pr)
    assert der == ["mag_vort", "diveru", "avg_pressure"]
    assert names == STATE + der and set(der) <= kept
    # the second tutorial file sets the same key (its ns.do_LES stays refused: only the key is looked at)
    text = open(LES).read()
    assert re.search(r"^\s*amr\.derive_plot_vars\s*=\s*mag_vort\s+diveru\s+avg_pressure", text, re.M)


def test_plot_selection_names():
    from iamr_amd import plotfile as P
    from iamr_amd import pdf
    assert P.VELGRAD_NAMES == TEN and list(pdf.VELGRAD_NAMES) == TEN
    assert "vorticity" not in P.VELGRAD_NAMES
    for nm in TEN:
        assert P.plot_selection(STATE, "ALL", [nm]) == ([0, 1, 2, 3, 4], [nm])
    assert P.plot_selection(STATE, "NONE", ["q_criterion", "energy", "r_invariant"]) == ([], ["q_criterion", "energy", "r_invariant"])
    # ALL is upstream's derive list: unchanged
    assert P.DERIVE_NAMES == ["energy", "mag_vort", "avg_pressure"]
    assert P.plot_selection(STATE, "ALL", "ALL") == ([0, 1, 2, 3, 4], ["energy", "mag_vort", "avg_pressure"])
    with pytest.raises(ValueError, match="diveru"):                          # the message lists the new names too
        P.plot_selection(STATE, "ALL", ["vorticity"])
    assert pdf.DERIVED_NAMES == ("energy", "mag_vort", "avg_pressure") + tuple(TEN)
    assert pdf.known_names()[-10:] == tuple(TEN)


def test_integrate_keys_parse():
    from iamr_amd.inputs import Inputs
    pr = Inputs([TG]).problem()
    assert pr["integrate"] == dict(interval=0, vars=[], file="integ")
    pr = Inputs([TG], ["ns.integrate_interval=5", "ns.integrate_vars=energy enstrophy dissipation", "ns.integrate_file=sums.txt"]).problem()
    assert pr["integrate"] == dict(interval=5, vars=["energy", "enstrophy", "dissipation"], file="sums.txt")
    pr = Inputs([TG], ["ns.integrate_interval=1", 'ns.integrate_vars="density q_criterion"']).problem()
    assert pr["integrate"]["vars"] == ["density", "q_criterion"] and pr["integrate"]["file"] == "integ"
    pr = Inputs([TG], ["ns.pdf_interval=1", "ns.pdf_vars=q_criterion r_invariant"]).problem()
    assert pr["pdf"]["vars"] == ["q_criterion", "r_invariant"]


def test_integrate_key_errors():
    from iamr_amd.inputs import Inputs
    with pytest.raises(ValueError, match="q_criterion"):                     # an interval without names: the known names are listed
        Inputs([TG], ["ns.integrate_interval=1"]).problem()
    with pytest.raises(ValueError, match="enstrophy") as e:
        Inputs([TG], ["ns.integrate_interval=1", "ns.integrate_vars=energy vorticity"]).problem()
    assert "vorticity" in str(e.value) and "mag_vort" in str(e.value)
    with pytest.raises(ValueError, match="vorticity"):                       # names are checked also while the output is off
        Inputs([TG], ["ns.integrate_vars=vorticity"]).problem()
    with pytest.raises(ValueError):
        Inputs([TG], ["ns.integrate_interval=-1", "ns.integrate_vars=energy"]).problem()


@pytest.mark.parametrize("name", ["vort_x", "vort_y", "vort_z", "helicity", "r_invariant"])
def test_two_dimensional_refusals(name):
    from iamr_amd.inputs import Inputs
    for key in ("amr.derive_plot_vars", "ns.pdf_vars", "ns.integrate_vars"):
        with pytest.raises(NotImplementedError) as e:
            Inputs([DSL2D], [f"{key}={name}"]).problem()
        assert key in str(e.value) and name in str(e.value)


def test_two_dimensional_accepts():
    from iamr_amd.inputs import Inputs
    from iamr_amd import run as R
    ok = ["diveru", "enstrophy", "strain_rate", "dissipation", "q_criterion"]
    pr = Inputs([DSL2D], ["amr.derive_plot_vars=" + " ".join(ok), "ns.integrate_interval=1", "ns.integrate_vars=" + " ".join(ok),
                          "ns.pdf_vars=diveru"]).problem()
    assert pr["slab"] and pr["derive_plot_vars"] == ok and pr["integrate"]["vars"] == ok
    assert R.plot_names_and_filter(pr)[1] == ok


def test_integrals_file_round_trip(tmp_path):
    from iamr_amd.integrals import start_file, append_row, read_integrals, header_line
    names = ["energy", "enstrophy", "dissipation"]
    rng = np.random.default_rng(5)
    rows = [(s, float(t), rng.standard_normal(3) * 10.0 ** rng.integers(-300, 300, 3)) for s, t in zip((0, 1, 2), rng.uniform(0, 1, 3))]
    rows[1][2][0] = np.nextafter(1.0, 2.0)
    rows[2][2][1] = 5e-324
    path = str(tmp_path / "integ")
    with open(path, "w") as f:
        f.write("stale\n")
    start_file(path, names)                                                 # truncates
    for s, t, v in rows[:2]:
        append_row(path, names, s, t, v)
    assert open(path).readline() == header_line(names) + "\n" == "# step time energy enstrophy dissipation\n"
    start_file(path, names, append=True)                                    # a restarted run keeps what is there
    append_row(path, names, *rows[2])
    r = read_integrals(path)
    assert r["names"] == tuple(names) and r["step"].dtype == np.int64 and np.array_equal(r["step"], [0, 1, 2])
    assert r["time"].tobytes() == np.array([t for _, t, _ in rows]).tobytes()
    for q, nm in enumerate(names):
        assert r[nm].dtype == np.float64 and r[nm].tobytes() == np.array([v[q] for _, _, v in rows]).tobytes(), nm
    with pytest.raises(ValueError):
        start_file(path, ["energy"], append=True)                           # another set of names
    with pytest.raises(ValueError):
        append_row(path, names, 3, 0.5, [1.0])
    start_file(path, names)
    assert read_integrals(path)["step"].size == 0


def test_exports_declared():
    text = open(os.path.join(ROOT, "include", "iamrx.h")).read()
    for fn in ("iamrx_derive_velgrad", "iamrx_ns_derive_fields", "iamrx_ns_integrate", "iamrx_amr_integrate", "iamrx_velgrad_bench"):
        assert re.search(r"^int " + fn + r"\(", text, re.M), fn
    assert re.search(r"int iamrx_derive_velgrad\([^;]*int path\);", text)
    src = open(os.path.join(ROOT, "iamr_amd", "csrc", "cabi.hip")).read()
    for fn in ("iamrx_derive_velgrad", "iamrx_ns_derive_fields", "iamrx_ns_integrate", "iamrx_amr_integrate", "iamrx_velgrad_bench"):
        assert re.search(r"^int " + fn + r"\(", src, re.M), fn
    assert "k_velgrad.hip" in open(os.path.join(ROOT, "iamr_amd", "csrc", "Makefile")).read()
