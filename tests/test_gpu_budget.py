"""GPU: co-spectra, the k^2-weighted power, the skew-symmetric nonlinear term and the spectral energy budget (include/iamrx.h:
iamrx_mf_cospectrum / iamrx_mf_spectrum_k2 / iamrx_convective_term / iamrx_ns_spectral_budget / iamrx_amr_spectral_budget; kernels in
iamr_amd/csrc/k_spectrum.hip and k_convect.hip) through the C-ABI against the numpy yardstick of tests/cospectrum_numpy.py on the same
data, every tolerance the bound derived in its docstring.

The data are white noise of order one with non-zero means, b correlated with a; every ghost cell holds NaN unless the call needs it.
The shapes are the smallest at which each path can go wrong: unequal extents (an axis mix-up in the mirror index shows), a non-cubic
domain, the longest mirror on each axis, a chunk of a full wavefront, 4^3 where every row is its own mirror or a Nyquist row, one box
against eight.  C_ab and C_ba agree within the bound, not to the bit: the library transforms a + i b, and b + i a is another field."""
import ctypes as C
import functools
import math
import os
import numpy as np
import pytest
import spectrum_numpy as SN
import cospectrum_numpy as CN
from test_gpu_spectrum import make_mf, geom_of, UNIT, AMR16, FORCED, QUIET

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def pair(n, L, seed=3):
    """(f (n, 2) = (a, b), the yardstick's (C, P_a, P_b, count)): computed once per shape and shared, never written to"""
    f = SN.noise(n, seed, 2)
    f[..., 1] = 0.6 * np.roll(f[..., 0], (1, 2, 3), (0, 1, 2)) + 0.8 * f[..., 1] + 0.5
    f.setflags(write=False)
    return f, CN.cospectrum_reference(np.ascontiguousarray(f[..., 0]), np.ascontiguousarray(f[..., 1]), L)


def within(got, ref, bd, tag):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = np.abs(got - ref)
    worst = float(np.max(err[bd > 0.0] / bd[bd > 0.0])) if np.any(bd > 0.0) else 0.0          # (a bound of zero -- W(0), F without forcing -- asks for equality)
    print(f"{tag}: {len(ref)} shells, max |got - yardstick| = {float(err.max()):.3e}, worst error / bound = {worst:.4f}")
    assert np.all(err <= bd), (tag, worst)


# ------------------------------------------------------------------------------------------------------------------ 1. co-spectrum
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), (1.0, 1.0, 2.0)), ((1024, 4, 4), UNIT), ((4, 1024, 4), UNIT),
                                 ((4, 4, 1024), UNIT), ((128, 4, 4), UNIT), ((4, 4, 4), UNIT)])
def test_cospectrum_one_box(gpu, n, L):
    f, (Cr, Pa, Pb, count) = pair(n, L)
    N = f[..., 0].size
    mf, lay = make_mf(n, f)
    g = geom_of(n, L)
    Cg, Pag, Pbg, cg = gpu.mf_cospectrum(g, mf, mf, 0, 1)
    bd = CN.cospectrum_bound(Pa, Pb, count, N)
    within(Cg, Cr, bd, f"{n} L {L} C_ab")
    within(Pag, Pa, SN.bound(Pa, count, N), f"{n} L {L} P_a")
    within(Pbg, Pb, SN.bound(Pb, count, N), f"{n} L {L} P_b")
    assert cg.dtype == np.int64 and np.array_equal(cg, count) and int(cg.sum()) == N
    again = gpu.mf_cospectrum(g, mf, mf, 0, 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (Cg, Pag, Pbg, cg)))
    assert abs(math.fsum(Cg) - float(np.mean(f[..., 0] * f[..., 1]))) <= float(np.sum(bd))          # Parseval
    Cba = gpu.mf_cospectrum(g, mf, mf, 1, 0)[0]                                                        # C_ba: within the bound of C_ab
    within(Cba, Cr, bd, f"{n} L {L} C_ba")


def test_cospectrum_one_box_against_eight(gpu):
    """32^3 as one box and as eight 16^3 boxes: equal to the bit (only the pack differs), and again with a in one layout and b in the
    other; count may be NULL"""
    n = (32, 32, 32)
    f, (Cr, Pa, Pb, count) = pair(n, UNIT, 7)
    g = geom_of(n)
    one, _ = make_mf(n, f)
    eight, lay8 = make_mf(n, f, 16)
    assert len(lay8.boxes) == 8
    r1 = gpu.mf_cospectrum(g, one, one, 0, 1)
    within(r1[0], Cr, CN.cospectrum_bound(Pa, Pb, count, f[..., 0].size), "32^3 one box")
    for a, b, tag in ((eight, eight, "eight"), (one, eight, "one / eight"), (eight, one, "eight / one")):
        r = gpu.mf_cospectrum(g, a, b, 0, 1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(r, r1)), tag
    out, nb = np.zeros(3 * 29), C.c_int()
    assert gpu.lib().iamrx_mf_cospectrum(C.byref(g), one.h, 0, eight.h, 1, 29, out.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(nb)) == 0
    assert nb.value == 29 and out.tobytes() == np.concatenate(r1[:3]).tobytes()


@pytest.mark.parametrize("phi", [0.0, 1.0, math.pi / 2])
def test_cosine_pair(gpu, phi):
    """a = cos(theta), b = cos(theta + phi), mode (3, 4, 0) at 16^3: C(5) = cos(phi) / 2 within the bound, every other shell <= eps^2 Pt"""
    n = (16, 16, 16)
    i, j, k = np.meshgrid(*(np.arange(v) for v in n), indexing="ij")
    th = 2.0 * np.pi * (3 * i + 4 * j) / 16.0
    f = np.stack([np.cos(th), np.cos(th + phi)], axis=-1)
    _, Pa, Pb, count = CN.cospectrum_reference(f[..., 0].copy(), f[..., 1].copy(), UNIT)
    mf, _ = make_mf(n, f)
    Cg = gpu.mf_cospectrum(geom_of(n), mf, mf, 0, 1)[0]
    eps, Pt = SN.eps_of(16 ** 3), math.fsum(Pa) + math.fsum(Pb)
    others = float(np.abs(np.delete(Cg, 5)).max())
    print(f"phi = {phi}: |C(5) - cos(phi)/2| = {abs(Cg[5] - 0.5 * math.cos(phi)):.3e}, largest other shell {others:.3e} (bound {eps * eps * Pt:.3e})")
    assert abs(Cg[5] - 0.5 * math.cos(phi)) <= CN.cospectrum_bound(Pa, Pb, count, 16 ** 3)[5]
    assert others <= eps * eps * Pt


def test_nyquist_plane(gpu):
    """a = (-1)^i, b = 0.5 (-1)^i + cos(2 pi 3 i / n_x) at (16, 8, 8): the Nyquist plane is its own mirror; C(8) = 0.5, C(3) = 0"""
    n = (16, 8, 8)
    i = np.arange(16)[:, None, None] * np.ones(n)
    a = (-1.0) ** i
    f = np.stack([a, 0.5 * a + np.cos(2.0 * np.pi * 3.0 * i / 16.0)], axis=-1)
    _, Pa, Pb, count = CN.cospectrum_reference(f[..., 0].copy(), f[..., 1].copy(), UNIT)
    bd = CN.cospectrum_bound(Pa, Pb, count, a.size)
    mf, _ = make_mf(n, f)
    Cg = gpu.mf_cospectrum(geom_of(n), mf, mf, 0, 1)[0]
    print(f"C(8) - 0.5 = {Cg[8] - 0.5:.3e} (bound {bd[8]:.3e}), C(3) = {Cg[3]:.3e} (bound {bd[3]:.3e})")
    assert abs(Cg[8] - 0.5) <= bd[8] and abs(Cg[3]) <= bd[3]


# ------------------------------------------------------------------------------------------------------------------ 2. k^2 weighting
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), (1.0, 1.0, 2.0))])
def test_spectrum_k2(gpu, n, L):
    f, _ = pair(n, L)
    mf, _ = make_mf(n, f)
    Wg = gpu.mf_spectrum_k2(geom_of(n, L), mf, 0, 2)
    assert Wg.shape[0] == 2
    for q in range(2):
        W, P, count, k2max = CN.k2_reference(np.ascontiguousarray(f[..., q]), L)
        within(Wg[q], W, CN.k2_bound(W, P, count, k2max, f[..., q].size), f"{n} L {L} W component {q}")


def test_spectrum_k2_cosine_mode(gpu):
    """cos(2 pi (3 i + 4 j) / 16), L = 1: W(5) = k^2 / 2 with k^2 = 25 (2 pi)^2"""
    n = (16, 16, 16)
    f = SN.cosine_mode(n)[..., None]
    mf, _ = make_mf(n, f)
    Wg = gpu.mf_spectrum_k2(geom_of(n), mf, 0, 1)[0]
    W, P, count, k2max = CN.k2_reference(f[..., 0].copy(), UNIT)
    k2 = 25.0 * (2.0 * math.pi) ** 2
    assert abs(Wg[5] - 0.5 * k2) <= CN.k2_bound(W, P, count, k2max, 16 ** 3)[5]


# ------------------------------------------------------------------------------------------------------------------ 3. nonlinear term
def convect(gpu, n, L, V, max_grid_size=None):
    """the library's N of the periodic field V (n, 3): ghost cells by the library's periodic fill"""
    vel, lay = make_mf(n, V, max_grid_size)
    g = geom_of(n, L)
    vel.fill_boundary(g)
    out = gpu.MultiFab(lay, gpu.CELL, 3, 0)
    gpu.convective_term(g, out, vel)
    return out.gather_valid(n)


@pytest.mark.parametrize("n,L,mgs", [((8, 16, 32), UNIT, None), ((32, 32, 32), UNIT, None), ((32, 32, 32), UNIT, 16), ((16, 16, 32), (1.0, 1.0, 2.0), 8)])
def test_convective_term(gpu, n, L, mgs):
    V = SN.noise(n, 11, 3)
    Ng = convect(gpu, n, L, V, mgs)
    Nr, M = CN.convective_reference(V, [L[d] / n[d] for d in range(3)])
    err = np.abs(Ng - Nr)
    print(f"{n} boxes of {mgs}: worst error / bound = {float(np.max(err / (CN.GAMMA * M))):.3f}")
    assert np.all(err <= CN.GAMMA * M)
    tot, bd = CN.energy_identity(V, Ng, M)
    print(f"sum u.N = {tot:.3e} (bound {bd:.3e})")
    assert abs(tot) <= bd
    if mgs == 16:
        assert Ng.tobytes() == convect(gpu, n, L, V).tobytes()                     # eight boxes against one: the same bits


def test_convective_term_exact_zeros(gpu):
    n = (8, 16, 8)
    Uf = np.broadcast_to(np.array([1.0, 2.0, 3.0]), n + (3,)).copy()
    assert not convect(gpu, n, UNIT, Uf).any()
    Sh = np.zeros(n + (3,))
    Sh[..., 0] = np.sin(2.0 * np.pi * np.arange(n[1]) / n[1])[None, :, None]
    assert not convect(gpu, n, UNIT, Sh).any()


def test_convective_term_nan_reach(gpu):
    """a NaN in one ghost cell reaches only that cell's face neighbour"""
    n = (8, 8, 8)
    V = SN.noise(n, 5, 3)
    vel, lay = make_mf(n, V)
    g = geom_of(n)
    vel.fill_boundary(g)
    a, glo = vel.to_numpy(0)
    a[-1 - glo[0], 3 - glo[1], 4 - glo[2], :] = np.nan                             # the ghost cell (-1, 3, 4)
    vel.from_numpy(np.asfortranarray(a), 0)
    out = gpu.MultiFab(lay, gpu.CELL, 3, 0)
    gpu.convective_term(g, out, vel)
    bad = np.isnan(out.gather_valid(n))
    want = np.zeros(n + (3,), dtype=bool)
    want[0, 3, 4, :] = True
    assert np.array_equal(bad, want)


# ------------------------------------------------------------------------------------------------------------------ 4. level, hierarchy
def budget_check(s, ref, tag, cols=("E", "T", "D", "F")):
    for c in cols:
        within(s[c], ref[c], ref["b" + c], f"{tag} {c}")
    assert np.array_equal(s["count"], ref["count"])
    assert s["Pi"].tobytes() == (-np.cumsum(s["T"])).tobytes()
    assert abs(s["Pi"][-1]) <= float(np.sum(ref["bT"]))                             # the transfer sums to zero over the shells


def test_level(gpu):
    """a 16^3 level in eight boxes whose new-time state was set from outside, viscous, no forcing"""
    from iamr_amd import ns as N
    from test_gpu_profile import random_state, put_state
    n = (16, 16, 16)
    S = random_state(n, 12)
    lay = gpu.Layout.decompose(n, 8)
    ns = N.NavierStokes(gpu.Geom.make(list(n), periodic=(1, 1, 1)), lay, N.ns_params(visc_coef=0.01))
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    s = ns.spectral_budget()
    ref = CN.budget_reference(S, UNIT, 0.01)
    budget_check(s, ref, "level 16^3")
    assert not s["F"].any() and s["visc_coef"] == 0.01 and s["n"] == n and s["L"] == UNIT
    sp = ns.spectrum()
    N3 = float(S[..., 0].size)
    bsp = 0.5 * sum(SN.bound(*SN.spectrum_reference(np.ascontiguousarray(S[..., q]), UNIT), N3) for q in range(3))
    assert np.all(np.abs(s["E"] - sp["E"]) <= ref["bE"] + bsp) and np.array_equal(s["k"], sp["k"]) and np.array_equal(s["count"], sp["count"])
    again = ns.spectral_budget()
    assert all(again[c].tobytes() == s[c].tobytes() for c in ("E", "T", "Pi", "D", "F"))
    co = ns.cospectrum("x_velocity", "y_velocity")                                 # the Reynolds-stress co-spectrum by field name
    Cr, Pa, Pb, count = CN.cospectrum_reference(np.ascontiguousarray(S[..., 0]), np.ascontiguousarray(S[..., 1]), UNIT)
    within(co["C"], Cr, CN.cospectrum_bound(Pa, Pb, count, N3), "E_uv by name")


def forced_level(gpu, n=16):
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([FORCED], [f"amr.n_cell={n} {n} {n}", "amr.derive_plot_vars=NONE"] + QUIET).problem()
    ns, lay, g, pr = R.build(None, gpu, N, pr=pr)
    ns.post_init(pr["stop_time"])
    return ns, lay, g, pr


def test_forced_level(gpu):
    """inputs.3d.forced at 16^3 after post_init: F against the yardstick on u and lib.turb_force at the level's time"""
    ns, lay, g, pr = forced_level(gpu)
    n = tuple(g.n)
    Lside = tuple(g.prob_hi[d] - g.prob_lo[d] for d in range(3))
    s = ns.spectral_budget()
    S = ns.data(ns.S_NEW).gather_valid(n)
    k, d = gpu.host_turb_modes(g.prob_lo, g.prob_hi, ns.params.turb_nmodes, ns.params.turb_mode_start, ns.params.turb_div_free)
    fm = gpu.MultiFab(lay, gpu.CELL, 3, 0)
    gpu.turb_force(g, k, d, ns.params.turb_div_free, ns.time, fm)
    f = fm.gather_valid(n)
    ref = CN.budget_reference(S, Lside, ns.params.visc_coef, f)
    budget_check(s, ref, "forced 16^3")
    uf = float(np.mean(np.sum(S[..., :3] * f, axis=-1)))
    print(f"sum F = {math.fsum(s['F']):.6e}, mean(u.f) = {uf:.6e}")
    assert s["F"].any() and abs(math.fsum(s["F"]) - uf) <= float(np.sum(ref["bF"])) + 4.0 * CN.U * float(np.mean(np.sum(np.abs(S[..., :3] * f), axis=-1)))


def test_taylor_green(gpu):
    """TaylorGreen initial data at 32^3, one level, visc_coef = 0.01: E in shell 2 only, no transfer (products of modes with |m_d| = 1 have m_d in {0, +-2}
    and do not project back), D(2) = 2 visc 3 (2 pi / L)^2 E(2)"""
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([AMR16], ["amr.n_cell=32 32 32", "amr.max_level=0", "ns.vel_visc_coef=0.01", "amr.derive_plot_vars=NONE"] + QUIET).problem()
    ns, lay, g, pr = R.build(None, gpu, N, pr=pr)
    n = tuple(g.n)
    Lside = tuple(g.prob_hi[d] - g.prob_lo[d] for d in range(3))
    visc = ns.params.visc_coef
    assert n == (32, 32, 32) and visc > 0.0 and len(set(Lside)) == 1
    s = ns.spectral_budget()
    ref = CN.budget_reference(ns.data(ns.S_NEW).gather_valid(n), Lside, visc)
    budget_check(s, ref, "TaylorGreen 32^3")
    eps = SN.eps_of(32 ** 3)
    assert ref["E"][2] > 0.0 and float(np.delete(ref["E"], 2).max()) <= eps * eps * ref["E"][2]
    print(f"largest |T| / bound = {float(np.max(np.abs(s['T']) / ref['bT'])):.3e}")
    assert np.all(np.abs(s["T"]) <= ref["bT"])
    k2 = 3.0 * (2.0 * math.pi / Lside[0]) ** 2
    assert abs(s["D"][2] - 2.0 * visc * k2 * s["E"][2]) <= ref["bD"][2] + 2.0 * visc * k2 * ref["bE"][2] + 8.0 * CN.U * s["D"][2]


def test_hierarchy(gpu):
    """inputs.3d.taylorgreen_amr16 after one coarse step: Amr.spectral_budget against the yardstick on level 0's read-back"""
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([AMR16]).problem()
    amr, lays, g0 = R.build_amr(pr, gpu, N)
    amr.post_init(pr["stop_time"])
    amr.coarse_step()
    n = tuple(amr.geom0.n)
    assert n == (16, 16, 16) and amr.nlev > 1
    s = amr.spectral_budget()
    S = amr.levels[0].data(amr.levels[0].S_NEW).gather_valid(n)
    Lside = tuple(amr.geom0.prob_hi[d] - amr.geom0.prob_lo[d] for d in range(3))
    budget_check(s, CN.budget_reference(S, Lside, amr.params.visc_coef), "hierarchy level 0")
    assert not s["F"].any()


# ------------------------------------------------------------------------------------------------------------------ 5. driver
def test_driver_writes_the_files(gpu, tmp_path, monkeypatch):
    """inputs.3d.forced at 16^3, two steps with ns.budget_interval = 1: sbud00000 .. sbud00002 hold NavierStokes.spectral_budget of that
    moment bit for bit; without the key no file appears; ns.spectrum_interval alone writes its spec files and nothing else"""
    from iamr_amd import run as R
    from iamr_amd.budget import read_budget
    over = ["amr.n_cell=16 16 16", "max_step=2", "amr.derive_plot_vars=NONE"] + QUIET
    seen = {}

    def observe(ns, step, dt):
        seen[step] = (ns.time, ns.spectral_budget())

    d1 = tmp_path / "on"; d1.mkdir()
    monkeypatch.chdir(d1)
    assert R.main([FORCED, "ns.budget_interval=1"] + over, observe) == 0
    assert sorted(os.listdir(d1)) == ["sbud00000", "sbud00001", "sbud00002"]
    for step in range(3):
        time, s = seen[step]
        r = read_budget(str(d1 / f"sbud{step:05d}"))
        assert (r["step"], r["time"], r["n"], r["visc_coef"]) == (step, time, (16, 16, 16), s["visc_coef"])
        assert (r["sum_T"], r["sum_D"], r["sum_F"]) == (math.fsum(s["T"]), math.fsum(s["D"]), math.fsum(s["F"])) and r["sum_D"] > 0.0
        for k in ("k", "count", "E", "T", "Pi", "D", "F"):
            assert r[k].tobytes() == s[k].tobytes(), (step, k)
    d2 = tmp_path / "off"; d2.mkdir()
    monkeypatch.chdir(d2)
    assert R.main([FORCED] + over) == 0
    assert os.listdir(d2) == []
    d3 = tmp_path / "spec"; d3.mkdir()
    monkeypatch.chdir(d3)
    assert R.main([FORCED, "ns.spectrum_interval=1"] + over) == 0
    assert sorted(os.listdir(d3)) == ["spec00000", "spec00001", "spec00002"]


# ------------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors(gpu):
    from iamr_amd.lib import IamrxError
    f = SN.noise((24, 16, 16), 1, 2)
    mf, _ = make_mf((24, 16, 16), f)
    with pytest.raises(IamrxError, match=r"n_x = 24"):
        gpu.mf_cospectrum(geom_of((24, 16, 16)), mf, mf, 0, 1)
    with pytest.raises(IamrxError, match=r"n_x = 24"):
        gpu.mf_spectrum_k2(geom_of((24, 16, 16)), mf, 0, 1)
    n = (8, 16, 32)
    f, (Cr, _, _, _) = pair(n, UNIT)
    mf, lay = make_mf(n, f)
    with pytest.raises(IamrxError, match="periodic"):
        gpu.mf_cospectrum(geom_of(n, periodic=(1, 0, 1)), mf, mf, 0, 1)
    with pytest.raises(IamrxError, match="component"):
        gpu.mf_cospectrum(geom_of(n), mf, mf, 0, 2)
    with pytest.raises(IamrxError, match="component"):
        gpu.mf_spectrum_k2(geom_of(n), mf, 1, 2)
    with pytest.raises(IamrxError, match="cover"):                                  # the array's one box is half of this domain
        gpu.mf_cospectrum(geom_of((8, 16, 64)), mf, mf, 0, 1)
    nbins = len(Cr)
    out, nb = np.zeros(3 * nbins), C.c_int()
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    g = geom_of(n)
    assert gpu.lib().iamrx_mf_cospectrum(C.byref(g), mf.h, 0, mf.h, 1, nbins - 1, ptr, None, C.byref(nb)) != 0       # capacity too small ...
    assert nb.value == nbins and not out.any()                                                                        # ... *nbins all the same
    nb = C.c_int()
    assert gpu.lib().iamrx_mf_spectrum_k2(C.byref(g), mf.h, 0, 1, nbins - 1, ptr, C.byref(nb)) != 0 and nb.value == nbins and not out.any()
    vel0 = gpu.MultiFab(lay, gpu.CELL, 3, 0)                                        # no ghost layer
    out3 = gpu.MultiFab(lay, gpu.CELL, 3, 0)
    with pytest.raises(IamrxError, match="ghost layer"):
        gpu.convective_term(g, out3, vel0)
    vel1 = gpu.MultiFab(lay, gpu.CELL, 3, 1)
    with pytest.raises(IamrxError, match="components"):
        gpu.convective_term(g, out3, vel1, ocomp=1)
