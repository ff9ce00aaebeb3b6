"""CPU suite: the turbulent forcing's mode table (host-only entry iamrx_host_turb_modes) against the numpy yardstick tests/turb_numpy.py,
pins of the yardstick itself, and the inputs keys that switch the forcing on.  No GPU."""
import os
import numpy as np
import pytest

import turb_numpy as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED = os.path.join(ROOT, "tests", "golden", "inputs.3d.forced")
CUBE = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
LONG = ((0.0, 0.0, 0.0), (1.0, 1.0, 2.0))
A0, A1 = tn.IX["FAX"], tn.IX["FAZ"] + 1


# ---- pins of the yardstick ------------------------------------------------------------------------------------------------------------
def test_stream_is_mt19937():
    s = tn.Stream(5489)
    assert [int(v) for v in s.raw[:3]] == [3499211612, 581869302, 3890346734]


def test_entry_counts():
    k, d = tn.modes(*CUBE, nmodes=4)
    assert len(k) == 54 and int(np.count_nonzero(np.abs(d[:, A0:A1]).max(axis=1))) == 53
    assert tuple(k[0]) == (0, 0, 0) and np.all(d[0, A0:A1] == 0.0) and d[0, tn.IX["FTX"]] != 0.0      # the zero mode keeps its draws
    k, d = tn.modes(*LONG, nmodes=2)
    main = int(np.sum(k[:, 2] % 2 == 0))
    assert (main, len(k) - main) == (11, 4) and int(np.count_nonzero(np.abs(d[:, A0:A1]).max(axis=1))) == 14
    assert np.all(k[main:, 2] == 1)                     # the symmetry-breaking set comes last


def _field16(div_free):
    k, d = tn.modes(*CUBE, nmodes=4, div_free=div_free)
    x, y, z = tn.centres(*CUBE, (16, 16, 16), (0, 0, 0), (15, 15, 15))
    return tn.field(k, d, div_free, *CUBE, x, y, z, 0.37)


def test_divergence_free_form_is_solenoidal():
    f = _field16(1)
    kk = 2.0 * np.pi * np.fft.fftfreq(16, d=1.0 / 16)
    div = (1j * kk[:, None, None] * np.fft.fftn(f[..., 0]) + 1j * kk[None, :, None] * np.fft.fftn(f[..., 1])
           + 1j * kk[None, None, :] * np.fft.fftn(f[..., 2]))
    div = np.abs(np.fft.ifftn(div)).max()
    print("spectral divergence", div, "field", np.abs(f).max())
    assert div <= 1e-12


def test_forms_differ():
    a, b = _field16(1), _field16(0)
    assert np.abs(a - b).max() > 1e-3 * np.abs(a).max()


# ---- the product's table ----------------------------------------------------------------------------------------------------------------
def _ulp_diff(a, b):
    return np.abs(a - b) / np.maximum(np.spacing(np.abs(b)), np.finfo(float).tiny)


@pytest.mark.parametrize("box,nmodes,mode_start,div_free", [(CUBE, 4, 0, 1), (CUBE, 4, 0, 0), (LONG, 2, 0, 1), (LONG, 2, 0, 0), (CUBE, 2, 1, 1), (CUBE, 2, 1, 0)])
def test_host_table_equals_yardstick(box, nmodes, mode_start, div_free):
    from iamr_amd import lib
    k, d = lib.host_turb_modes(box[0], box[1], nmodes, mode_start, div_free)
    kr, dr = tn.modes(box[0], box[1], nmodes, mode_start, div_free)
    assert k.shape == kr.shape and np.array_equal(k, kr)                   # integer wavevectors and their order
    phases = [q for q in range(17) if not A0 <= q < A1]
    assert np.array_equal(d[:, phases], dr[:, phases])                     # frequencies and phases: plain fp64 arithmetic on the draws
    u = _ulp_diff(d[:, A0:A1], dr[:, A0:A1])
    print("modes", len(k), "amplitude max ulp", u.max())
    assert u.max() <= 4.0                                                  # amplitudes go through sin / cos of libm and of numpy
    if not div_free:
        assert np.all(d[:, tn.IX["FPXX"]:] == 0.0)
    if mode_start:
        assert k.min() >= mode_start


@pytest.mark.parametrize("lo,hi,nmodes,rule", [((0, 0, 0), (1, 2, 2), 2, "Lx == Ly"), ((0, 0, 0), (1, 1, 0.5), 2, "Lz >= Lx"), ((0, 0, 0), (1, 1, 3), 11, "<= 32")])
def test_refusals(lo, hi, nmodes, rule):
    from iamr_amd import lib
    with pytest.raises(lib.IamrxError, match=rule):
        lib.host_turb_modes(lo, hi, nmodes)


def test_default_params_leave_forcing_off():
    from iamr_amd import ns
    p = ns.ns_params()
    assert (p.turb_forcing, p.turb_nmodes, p.turb_mode_start, p.turb_div_free) == (0, 4, 0, 1)
    q = ns.ns_params(turb_forcing=1, turb_nmodes=2, turb_mode_start=1, turb_div_free=0)
    assert (q.turb_forcing, q.turb_nmodes, q.turb_mode_start, q.turb_div_free) == (1, 2, 1, 0)
    # they travel beside the library's struct, whose layout stays what it was (the forcing is set on a level after its creation)
    assert not [f[0] for f in ns.NsParams._fields_ if f[0].startswith("turb")]


def test_header_declares_and_library_exports_the_entries():
    import re
    from iamr_amd import lib
    txt = open(os.path.join(ROOT, "include", "iamrx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in ("iamrx_host_turb_modes", "iamrx_turb_force", "iamrx_ns_set_turb_forcing", "iamrx_amr_set_turb_forcing", "iamrx_ns_set_turb_modes",
              "iamrx_amr_set_turb_modes"):
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert hasattr(lib.lib(), s), s


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
OVERRIDES = ["amr.n_cell=16 16 16", "max_step=4", "amr.plot_int=-1", "amr.check_int=-1", "amr.derive_plot_vars=NONE"]


def test_inputs_switch_forcing_on():
    from iamr_amd.inputs import Inputs
    inp = Inputs([FORCED], OVERRIDES)
    pr = inp.problem()
    p = pr["params"]
    assert (p["turb_forcing"], p["turb_nmodes"], p["turb_mode_start"], p["turb_div_free"]) == (1, 4, 0, 1)
    assert pr["prob"]["probtype"] == 100 and pr["prob"]["turb_scale"] == 1.0 and pr["prob"]["density_ic"] == 1.0
    assert "turb.force_file" in inp.ignored
    assert p["proj_tol"] == 1.0e-10                     # nodal_proj.proj_tol of the file
    pr = Inputs([FORCED], OVERRIDES + ["turb.div_free_force=0", "turb.mode_start=1", "turb.ff_factor=4", "turb.verbose=1"]).problem()
    assert (pr["params"]["turb_div_free"], pr["params"]["turb_mode_start"]) == (0, 1)


def test_inputs_without_turb_keys_leave_forcing_off():
    from iamr_amd.inputs import Inputs
    pr = Inputs([os.path.join(ROOT, "tests", "golden", "inputs.3d.taylorgreen")], ["amr.derive_plot_vars=NONE"]).problem()
    assert pr["params"]["turb_forcing"] == 0


def test_inputs_refuse_unknown_turb_key_and_slab():
    from iamr_amd.inputs import Inputs
    with pytest.raises(KeyError, match="turb.spectrum"):
        Inputs([FORCED], OVERRIDES + ["turb.spectrum=3"]).problem()
    slab = os.path.join(ROOT, "tests", "golden", "inputs.2d.doubleshearlayer_c3")
    with pytest.raises(NotImplementedError, match="two-dimensional"):
        Inputs([slab], ["turb.nmodes=4"]).problem()


def test_probtype_100_initial_state():
    from iamr_amd import probinit
    prob = dict(probtype=100, turb_scale=0.5, density_ic=2.0, prob_lo=[0.0, 0.0, 0.0], prob_hi=[1.0, 1.0, 2.0])
    X, Y, Z = probinit.cell_centres((8, 8, 16), prob["prob_lo"], prob["prob_hi"])
    S = probinit.initial_state(prob, X, Y, Z, 6)
    c = lambda a, L: np.cos(2.0 * np.pi * a / L)
    assert np.allclose(S[..., 0], 0.5 * c(Y, 1.0) * c(Z, 2.0), rtol=0, atol=1e-15)
    assert np.allclose(S[..., 1], 0.5 * c(X, 1.0) * c(Z, 2.0), rtol=0, atol=1e-15)
    assert np.allclose(S[..., 2], 0.5 * c(X, 1.0) * c(Y, 1.0), rtol=0, atol=1e-15)
    assert np.all(S[..., 3] == 2.0) and np.all(S[..., 4:] == 1.0)
