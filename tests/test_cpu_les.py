"""CPU suite: the LES closure (reference Source/NS_LES.cpp).  Pins of the numpy yardstick the GPU tests compare the kernel with
(tests/les_numpy.py), the new parameters and their defaults, the C-ABI entries, and the inputs keys."""
import os
import re
import numpy as np
import pytest
import les_numpy as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOTSPOT = os.path.join(GOLD, "inputs.3d.LES_hotspot")
LDC = os.path.join(GOLD, "inputs.3d.lid_driven_cavity16")


def test_sigma_of_a_diagonal_gradient():
    """singular values 3, 2, 1: sigma3 (sigma1 - sigma2)(sigma2 - sigma3) / sigma1^2 = 1/9"""
    g = np.zeros((1, 9)); g[0, 0], g[0, 4], g[0, 8] = 3.0, 2.0, 1.0
    fac = (1.5 * 0.1) ** 2
    assert abs(LN.sigma(g, fac)[0] - fac / 9) <= 1e-13 * fac


def test_smagorinsky_of_a_pure_shear():
    """one component gamma: 0.5 (2 gamma)^2 = 2 gamma^2"""
    for gamma in (0.7, -2.5):
        g = np.zeros((1, 9)); g[0, 1] = gamma
        fac = (0.18 * 0.05) ** 2
        assert abs(LN.smagorinsky(g, fac)[0] - fac * np.sqrt(2.0) * abs(gamma)) <= 4e-16 * fac * abs(gamma)


def test_zero_gradient_gives_exactly_zero():
    g = np.zeros((3, 9))
    assert np.all(LN.smagorinsky(g, 1.0) == 0.0) and np.all(LN.sigma(g, 1.0) == 0.0)


def test_models_are_invariant_under_transposing_the_gradient():
    rng = np.random.default_rng(3)
    g = rng.standard_normal((500, 9))
    gt = g.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    s, st = LN.smagorinsky(g, 1.0), LN.smagorinsky(gt, 1.0)
    assert np.abs(s - st).max() <= 4e-16 * np.abs(s).max()
    (m, s1), mt = LN.sigma(g, 1.0, with_s1=True), LN.sigma(gt, 1.0)
    assert np.abs(m - mt).max() <= 5e-12 * s1.max()


def periodic_fields():
    rng = np.random.default_rng(7)
    noise16 = np.moveaxis(rng.standard_normal((3, 16, 16, 16)), 0, -1)
    noise24 = np.moveaxis(rng.standard_normal((3, 24, 24, 24)), 0, -1)
    tp = 2 * np.pi

    def grid(n):
        x = (np.arange(n) + 0.5) / n
        return np.meshgrid(x, x, x, indexing="ij")
    # two modes per component, wave vectors, amplitudes and phases drawn from rng: no symmetry (a field such as sin x cos y cos z has
    # whole surfaces on which two singular values coincide, where the closed form loses half its digits)
    rm = np.random.default_rng(7)
    rm.standard_normal((3, 16, 16, 16))          # (the modes continue the stream behind the first noise field)
    X, Y, Z = grid(16)
    S16 = np.zeros((16, 16, 16, 3))
    for c in range(3):
        for _ in range(2):
            k = rm.integers(1, 4, 3)
            amp, ph = rm.standard_normal(), rm.uniform(0, tp)
            S16[..., c] += amp * np.sin(tp * (k[0] * X + k[1] * Y + k[2] * Z) + ph)
    X, Y, Z = grid(24)
    S24 = np.stack([np.sin(tp * X) + 0.5 * np.sin(2 * tp * Y) + 0.25 * np.sin(3 * tp * Z),
                    np.cos(tp * X) + 0.5 * np.cos(2 * tp * Y) + 0.25 * np.cos(3 * tp * Z), np.sin(tp * (X + Y + Z))], axis=-1)
    return [("noise16", noise16), ("sines16", S16), ("sines24+noise", S24 + 0.1 * noise24)]


def test_sigma_equals_the_singular_values_of_numpy():
    """the closed form of NS_LES.cpp:153-209 against numpy.linalg.svd on every face of three periodic fields; error as a fraction of
    (Cs Delta)^2 sigma_1.  Measured maxima when the issue was written: 8.9e-13, 1.5e-13, 7.8e-13; bound 5e-12, five times the
    largest.  The error is the conditioning of acos next to +-1 (two nearly equal singular values), so it depends on the draw (other seeds of the
    same fields reach 1e-10, a field with exactly coinciding singular values 1e-9): the fields are fixed -- default_rng(7), components
    drawn first, unit cube; the white noise is the issue's (8.9e-13 again), the two others measure 2.5e-12 and 5.5e-13 here."""
    for name, V in periodic_fields():
        n = V.shape[0]
        dx = (1.0 / n,) * 3
        P = np.pad(V, ((1, 1), (1, 1), (1, 1), (0, 0)), mode="wrap")
        G = LN.grads(P, dx)
        for D in range(3):
            mu = LN.sigma(G[D], 1.0)
            sv = np.linalg.svd(G[D].reshape(G[D].shape[:-1] + (3, 3)), compute_uv=False)
            s1, s2, s3 = sv[..., 0], sv[..., 1], sv[..., 2]
            ref = s3 * (s1 - s2) * (s2 - s3) / (s1 * s1)
            err = np.abs(mu - ref) / s1
            print(name, D, float(err.max()))
            assert err.max() <= 5e-12, (name, D, float(err.max()))


def test_gradients_of_a_linear_field_are_exact():
    n = (6, 5, 4)
    dx = (0.1, 0.2, 0.3)
    x = [(np.arange(-1, n[d] + 1) + 0.5) * dx[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*x, indexing="ij")
    A = np.array([[1.0, 2.0, 3.0], [-4.0, 5.0, 6.0], [7.0, -8.0, 9.0]])
    P = np.stack([A[c, 0] * X + A[c, 1] * Y + A[c, 2] * Z for c in range(3)], axis=-1)
    for D, g in enumerate(LN.grads(P, dx)):
        assert g.shape == tuple(n[d] + (d == D) for d in range(3)) + (9,)
        assert np.abs(g - A.reshape(9)).max() <= 1e-12


def test_parameter_defaults():
    from iamr_amd import ns as N
    p = N.ns_params()
    assert (p.do_LES, p.LES_model, p.smago_Cs_cst, p.sigma_Cs_cst) == (0, 0, 0.18, 1.5)
    q = N.ns_params(do_LES=1, LES_model=N.SIGMA, sigma_Cs_cst=1.35)
    assert (q.do_LES, q.LES_model, q.sigma_Cs_cst) == (1, 1, 1.35)


def test_header_declares_and_library_exports_the_les_entries():
    from iamr_amd import lib
    txt = open(os.path.join(ROOT, "include", "iamrx.h")).read()
    struct = txt[txt.index("typedef struct iamrx_ns_params"):txt.index("} iamrx_ns_params;")]
    fields = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    tail = [f.strip() for f in fields.split(";") if f.strip()][-4:]
    assert tail == ["int do_LES", "int LES_model", "double smago_Cs_cst", "double sigma_Cs_cst"], tail      # appended at the end
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = lib.lib()
    for s in ("iamrx_les_mut", "iamrx_calc_mut_les", "iamrx_calc_mut_les_cf"):
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert hasattr(L, s), s


def test_tutorial_fixture_parses_with_the_sigma_model():
    from iamr_amd.inputs import Inputs
    inp = Inputs([HOTSPOT], ["ns.do_LES=0", "amr.derive_plot_vars=mag_vort avg_pressure"])
    p = inp.problem()["params"]
    assert (p["do_LES"], p["LES_model"], p["smago_Cs_cst"], p["sigma_Cs_cst"]) == (0, 1, 0.18, 1.5)
    assert not [k for k in inp.ignored if "LES" in k or "Cs_cst" in k]
    # the keys are read in every run (NavierStokesBase.cpp:481-485), LES or not
    p = Inputs([LDC], ["ns.LES_model=Smagorinsky", "ns.smago_Cs_cst=0.1", "ns.sigma_Cs_cst=1.2", "ns.getLESVerbose=1"]).problem()["params"]
    assert (p["do_LES"], p["LES_model"], p["smago_Cs_cst"], p["sigma_Cs_cst"]) == (0, 0, 0.1, 1.2)


def test_a_bad_les_model_raises():
    from iamr_amd.inputs import Inputs
    with pytest.raises(ValueError):
        Inputs([LDC], ["ns.LES_model=WALE"]).problem()


def test_the_inputs_switch_stays_off_and_says_where_les_lives():
    from iamr_amd.inputs import Inputs
    with pytest.raises(NotImplementedError, match="iamrx_ns_params.do_LES"):
        Inputs([HOTSPOT], ["amr.derive_plot_vars=mag_vort avg_pressure"]).problem()
