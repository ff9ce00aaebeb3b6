"""CPU suite: co-spectra and the spectral energy budget (iamr_amd/budget.py, the ns.budget_* keys of iamr_amd/inputs.py, the entries of
include/iamrx.h) -- everything about them that needs no device.  The numpy yardstick the GPU tests compare with
(tests/cospectrum_numpy.py) is itself checked here: the packed identity the library uses through an independent radix-2 transform
within the derived bound, the energy identity of the skew-symmetric nonlinear term, and a cosine pair whose answer is written out."""
import math
import os
import re
import numpy as np
import pytest
import spectrum_numpy as SN
import cospectrum_numpy as CN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TG16 = os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")
UNIT = (1.0, 1.0, 1.0)


def pair(n, seed=3):
    """noise a and b = 0.6 roll(a) + 0.8 noise + 0.5: correlated, with means of their own"""
    f = SN.noise(n, seed, 2)
    a = np.ascontiguousarray(f[..., 0])
    return a, 0.6 * np.roll(a, (1, 2, 3), (0, 1, 2)) + 0.8 * f[..., 1] + 0.5


# ------------------------------------------------------------------------------------------------------------------ 1. the yardstick
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), (1.0, 1.0, 2.0)), ((128, 4, 4), UNIT), ((4, 4, 4), UNIT), ((4, 64, 4), UNIT)])
def test_packed_identity_within_the_bound(n, L):
    """ONE radix-2 transform of a + i b, every mode read with its mirror mode (rows 0 and n / 2 mirror themselves), gives C_ab, P_a and
    P_b of two numpy transforms within the derived bounds; Parseval: the shells of C sum to mean(a b)"""
    a, b = pair(n)
    N = a.size
    C, Pa, Pb, count = CN.cospectrum_reference(a, b, L)
    Cp, Pap, Pbp, countp = CN.cospectrum_packed(a, b, L)
    bd = CN.cospectrum_bound(Pa, Pb, count, N)
    Pt = math.fsum(Pa) + math.fsum(Pb)
    print(f"{n}: packed C error / bound = {float(np.max(np.abs(Cp - C) / bd)):.2e}, smallest |C| / bound = {float(np.min(np.abs(C) / bd)):.2e}")
    assert np.array_equal(count, countp) and int(count.sum()) == N
    assert np.all(np.abs(Cp - C) <= bd)
    assert np.all(np.abs(Pap - Pa) <= CN.power_bound_packed(Pa, Pt, count, N)) and np.all(np.abs(Pbp - Pb) <= CN.power_bound_packed(Pb, Pt, count, N))
    assert abs(math.fsum(C) - float(np.mean(a * b))) <= float(np.sum(bd))
    Caa, Paa, _, _ = CN.cospectrum_reference(a, a, L)
    assert np.all(np.abs(Caa - Paa) <= 4.0 * CN.U * Paa)                             # C_aa = P_a (the complex product may round differently)


@pytest.mark.parametrize("phi", [0.0, 1.0, math.pi / 2])
def test_cosine_pair(phi):
    """a = cos(theta), b = cos(theta + phi) with mode (3, 4, 0) at 16^3: C(5) = cos(phi) / 2, nothing anywhere else"""
    n = (16, 16, 16)
    i, j, k = np.meshgrid(*(np.arange(v) for v in n), indexing="ij")
    th = 2.0 * np.pi * (3 * i + 4 * j) / 16.0
    a, b = np.cos(th), np.cos(th + phi)
    for form in (CN.cospectrum_reference, CN.cospectrum_packed):
        C, Pa, Pb, count = form(a, b, UNIT)
        bd = CN.cospectrum_bound(Pa, Pb, count, a.size)
        eps = SN.eps_of(a.size)
        assert abs(C[5] - 0.5 * math.cos(phi)) <= bd[5]
        assert float(np.abs(np.delete(C, 5)).max()) <= eps * eps * 1.0              # Pt_a + Pt_b = 1


def test_k2_yardstick_on_a_cosine_mode():
    """cos(2 pi (3 i + 4 j) / 16), L = 1: W(5) = k^2 / 2 with k^2 = 25 (2 pi)^2"""
    f = SN.cosine_mode((16, 16, 16))
    W, P, count, k2max = CN.k2_reference(f, UNIT)
    k2 = 25.0 * (2.0 * math.pi) ** 2
    assert abs(W[5] - 0.5 * k2) <= CN.k2_bound(W, P, count, k2max, f.size)[5]
    assert k2max[5] >= k2 * (1.0 - 1e-15) and float(np.delete(W, 5).max()) <= k2max.max() * SN.eps_of(f.size) ** 2


def test_energy_identity_of_the_nonlinear_term():
    """sum_x u_i N_i = 0 up to rounding for noise on (16, 16, 32), L = (1, 1, 2); the ghost-filled form gives the bits of np.roll; a
    uniform flow and a shear flow give exactly zero"""
    n, L = (16, 16, 32), (1.0, 1.0, 2.0)
    dx = [L[d] / n[d] for d in range(3)]
    V = SN.noise(n, 11, 3)
    N, M = CN.convective_reference(V, dx)
    tot, bd = CN.energy_identity(V, N, M)
    scale = math.fsum(np.abs(V * N).ravel())
    print(f"sum u.N = {tot:.3e}, bound {bd:.3e}, sum |u.N| = {scale:.3e}")
    assert abs(tot) <= bd and bd < 1e-12 * scale
    G = np.pad(V, ((1, 1), (1, 1), (1, 1), (0, 0)), mode="wrap")
    Ng, Mg = CN.convective_reference(G, dx, ghost=True)
    assert Ng.tobytes() == N.tobytes() and Mg.tobytes() == M.tobytes()
    Uf = np.broadcast_to(np.array([1.0, 2.0, 3.0]), n + (3,)).copy()
    assert not CN.convective_reference(Uf, dx)[0].any()
    Sh = np.zeros(n + (3,))
    Sh[..., 0] = np.sin(2.0 * np.pi * np.arange(n[1]) / n[1])[None, :, None]
    assert not CN.convective_reference(Sh, dx)[0].any()


# ------------------------------------------------------------------------------------------------------------------ 2. inputs
def test_budget_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([TG16]).problem()
    assert off["budget"] == dict(interval=-1, file="sbud")
    on = Inputs([TG16], ["ns.budget_interval=5", "ns.budget_file=out/bud"]).problem()
    assert on["budget"] == dict(interval=5, file="out/bud")
    assert on["params"] == off["params"] and not any("budget" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "budget"} == {k: v for k, v in off.items() if k != "budget"}
    assert Inputs([LDC], ["ns.budget_interval=-1", "ns.budget_file=x"]).problem()["budget"] == dict(interval=-1, file="x")
    with pytest.raises(KeyError, match="ns.budget_intervall"):                       # an unknown neighbour key still raises
        Inputs([TG16], ["ns.budget_intervall=5"]).problem()


def test_budget_refusals_name_the_reason():
    from iamr_amd.inputs import Inputs
    with pytest.raises(ValueError, match=r"ns.budget_interval > 0 needs a fully periodic domain"):
        Inputs([LDC], ["ns.budget_interval=1"]).problem()
    with pytest.raises(ValueError, match=r"ns.budget_interval > 0 needs extents that are powers of two in 4 .. 1024, amr.n_cell has n_y = 24"):
        Inputs([TG16], ["ns.budget_interval=1", "amr.n_cell=16 24 16", "amr.max_level=0"]).problem()
    with pytest.raises(NotImplementedError, match=r"ns.budget_interval > 0 in a two-dimensional run"):
        Inputs([POIS2D], ["ns.budget_interval=1"]).problem()


# ------------------------------------------------------------------------------------------------------------------ 3. files
def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import budget as B
    from iamr_amd import spectrum as S
    rng = np.random.default_rng(5)
    n, L = (16, 16, 32), (1.0, 1.0, 2.0)
    nb = S.nbins_of(n, L)
    cols = rng.standard_normal((4, nb)) * 10.0 ** rng.integers(-30, 3, size=(4, nb))
    count = rng.integers(1, 5000, size=nb)
    s = B.as_dict(cols, count, n, L, 0.1 / 3.0)
    assert np.array_equal(s["Pi"], -np.cumsum(cols[1])) and np.array_equal(s["F"], cols[3])
    path = str(tmp_path / "sbud00007")
    B.write_budget(path, s, 7, 0.1 + 0.2)
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head == lines[:len(head)] and len(lines) == len(head) + nb
    assert head[0] == "# step = 7" and head[2] == "# n = 16 16 32" and head[-1] == "# columns = s k count E T Pi D F"
    assert all(len(l.split()) == 8 for l in lines[len(head):])
    r = B.read_budget(path)
    assert (r["step"], r["time"], r["n"], r["L"], r["visc_coef"]) == (7, 0.1 + 0.2, n, L, 0.1 / 3.0)
    assert (r["sum_T"], r["sum_D"], r["sum_F"]) == (math.fsum(s["T"]), math.fsum(s["D"]), math.fsum(s["F"]))
    assert r["count"].dtype == np.int64 and np.array_equal(r["count"], count)
    for k in ("k", "E", "T", "Pi", "D", "F"):
        assert r[k].tobytes() == s[k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------------ 4. the header
def test_the_entries_are_declared_and_exported():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    tail = r"int\s+nbins_cap,\s*double\s*\*\s*out,\s*long\s*\*\s*count,\s*int\s*\*\s*nbins"
    L = lib.lib()
    for name, args in (("iamrx_budget_nq", r"void"),
                       ("iamrx_mf_cospectrum", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+a,\s*int\s+acomp,\s*iamrx_mf\s+b,\s*int\s+bcomp,\s*" + tail),
                       ("iamrx_mf_spectrum_k2", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+ncomp,\s*int\s+nbins_cap,\s*double\s*\*\s*out,\s*int\s*\*\s*nbins"),
                       ("iamrx_convective_term", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+out,\s*int\s+ocomp,\s*iamrx_mf\s+vel,\s*int\s+vcomp"),
                       ("iamrx_ns_spectral_budget", r"iamrx_ns\s+ns,\s*" + tail),
                       ("iamrx_amr_spectral_budget", r"iamrx_amr\s+a,\s*" + tail)):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", txt), name
        assert hasattr(L, name), name
    assert L.iamrx_budget_nq() == 4 and L.iamrx_spectrum_nq() == 4
    from iamr_amd.ns import NavierStokes
    from iamr_amd.amr import Amr
    assert callable(NavierStokes.spectral_budget) and callable(NavierStokes.cospectrum) and callable(Amr.spectral_budget)
    assert callable(lib.mf_cospectrum) and callable(lib.mf_spectrum_k2) and callable(lib.convective_term)
