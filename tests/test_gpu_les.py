"""GPU: the LES closure (reference Source/NS_LES.cpp; NavierStokes::getViscosity, Source/NavierStokes.cpp:2119-2153).  The kernel k_les_mut
against the numpy yardstick (tests/les_numpy.py, pinned by tests/test_cpu_les.py), known answers, the operator entry
iamrx_calc_mut_les(_cf) against model(ghost cells of iamrx_tensor_apply(_cf)), the level step with a varying face viscosity, the
array-coefficient tensor paths against the oracle, the tutorial fixture and a two-level run.

Tolerances.  Smagorinsky: 4 ulp (same expression order as the yardstick, no contraction, a sum of squares).  Sigma:
|gpu - numpy| <= 1e-11 (Cs Delta)^2 sigma_1 -- only acos, cos and sqrt differ (device library against numpy), on identical arguments."""
import ctypes as C
import os
import numpy as np
import pytest
import les_numpy as LN

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DIR, NEU, PER = 101, 102, 0            # LinOpBC codes (include/iamrx.h)
CS = {LN.SMAGORINSKY: 0.18, LN.SIGMA: 1.5}


def nan_corners(a):
    """the eight corner ghost cells of a fab with one ghost layer: outside every stencil"""
    for i in (0, -1):
        for j in (0, -1):
            for k in (0, -1):
                a[i, j, k, :] = np.nan


def check_faces(model, got, P, dx, Cs, base, tag):
    """every face of the box (hi + 1 included) against the yardstick on the fab's own padded velocity P; returns the largest error seen
    (ulp for Smagorinsky, fraction of (Cs Delta)^2 sigma_1 for Sigma)"""
    ref = LN.mu_faces(model, P, dx, Cs, base)
    worst = 0.0
    for D in range(3):
        g, r = got[D][..., 0], ref[D]
        assert g.shape == r.shape, (tag, D, g.shape, r.shape)
        assert np.isfinite(g).all(), (tag, D)
        if model == LN.SMAGORINSKY:
            u = int(LN.ulp_diff(g, r).max())
            worst = max(worst, u)
            assert u <= 4, (tag, D, u)
        else:
            scale = LN.sigma_scale(P, dx, Cs)[D]
            err = np.abs(g - r)
            assert np.all(err <= 1e-11 * scale), (tag, D, float((err / np.maximum(scale, 1e-300)).max()))
            worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0)
    return worst


LAYOUTS = {
    "plain_16x12x8": ((16, 12, 8), [((0, 0, 0), (15, 11, 7))]),                       # shorter than a tile: the plain variant
    "lds_40x24x12": ((40, 24, 12), [((0, 0, 0), (39, 23, 11))]),                      # partial tiles in x and y, a partial z-chunk
    "two_boxes_40x16x8": ((40, 16, 8), [((0, 0, 0), (31, 15, 7)), ((32, 0, 0), (39, 15, 7))]),      # seam at x = 32, unequal boxes
}


@pytest.mark.parametrize("model", [LN.SMAGORINSKY, LN.SIGMA])
@pytest.mark.parametrize("case", list(LAYOUTS))
def test_kernel_against_numpy(gpu, case, model):
    lib = gpu
    from iamr_amd import ns as N
    n, boxes = LAYOUTS[case]
    g = lib.Geom.make(n, prob_hi=(n[0] * 0.011, n[1] * 0.017, n[2] * 0.007))
    dx = g.dx
    assert len({dx[0], dx[1], dx[2]}) == 3
    lay = lib.Layout(boxes)
    rng = np.random.default_rng(11)
    G = rng.standard_normal((n[0] + 2, n[1] + 2, n[2] + 2, 4))               # one array for all boxes: the two sides of a seam agree
    vel = lib.MultiFab(lay, lib.CELL, 4, 1)
    pads = []
    for li in range(vel.nlocal()):
        lo, hi = vel.fab_box(li)
        a = G[tuple(slice(lo[d] + 1, hi[d] + 2) for d in range(3))].copy()
        nan_corners(a)
        vel.from_numpy(a, li)
        pads.append(a[..., 1:4])
    mu = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
    worst = 0.0
    for base in (0.0, 0.01):
        for m in mu:
            m.setval(np.nan)
        N.les_mut(g, vel, mu, model, CS[model], base=base, vcomp=1)
        for li in range(vel.nlocal()):
            got = [mu[d].to_numpy(li)[0] for d in range(3)]
            worst = max(worst, check_faces(model, got, pads[li], dx, CS[model], base, (case, base, li)))
    print(f"k_les_mut {case} model {model}: largest error {worst:.3g} ({'ulp' if model == 0 else 'of (Cs D)^2 sigma_1'})")
    if len(boxes) == 2:        # the seam faces are written by both boxes: the same doubles
        a0, a1 = mu[0].to_numpy(0)[0], mu[0].to_numpy(1)[0]
        assert np.array_equal(a0[-1], a1[0])


def linear_velocity(n, dx, A):
    x = [(np.arange(-1, n[d] + 1) + 0.5) * dx[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*x, indexing="ij")
    return np.stack([A[c][0] * X + A[c][1] * Y + A[c][2] * Z for c in range(3)], axis=-1)


@pytest.mark.parametrize("n", [(16, 12, 8), (40, 24, 12)])
def test_known_answers(gpu, n):
    lib = gpu
    from iamr_amd import ns as N
    g = lib.Geom.make(n, prob_hi=(n[0] * 0.011, n[1] * 0.017, n[2] * 0.007))
    dx = g.dx
    lay = lib.Layout.single(n)
    vel = lib.MultiFab(lay, lib.CELL, 3, 1)
    mu = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]

    def run(P, model, Cs):
        vel.from_numpy(np.asfortranarray(P))
        N.les_mut(g, vel, mu, model, Cs)
        return [m.to_numpy(0)[0][..., 0] for m in mu]
    # u = (3x, 2y, z): singular values 3, 2, 1 -> Sigma = (Cs dx_d)^2 / 9 on every d-face
    out = run(linear_velocity(n, dx, [[3, 0, 0], [0, 2, 0], [0, 0, 1]]), LN.SIGMA, 1.5)
    for d in range(3):
        fac = (1.5 * dx[d]) ** 2
        assert np.abs(out[d] - fac / 9).max() <= 1e-11 * fac * 3.0, (d, float(np.abs(out[d] - fac / 9).max() / fac))
    # u = (gamma y, 0, 0): Smagorinsky = (Cs dx_d)^2 sqrt(2) |gamma|
    gamma = -2.5
    out = run(linear_velocity(n, dx, [[0, gamma, 0], [0, 0, 0], [0, 0, 0]]), LN.SMAGORINSKY, 0.18)
    for d in range(3):
        ref = (0.18 * dx[d]) ** 2 * np.sqrt(2.0) * abs(gamma)
        assert np.abs(out[d] - ref).max() <= 1e-12 * ref, d
    # fluid at rest: exactly zero
    for model in (LN.SMAGORINSKY, LN.SIGMA):
        out = run(np.zeros(tuple(q + 2 for q in n) + (3,)), model, CS[model])
        assert all(np.all(o == 0.0) for o in out), model
    # Sigma where the exact answer is zero (shear, rigid rotation, a z-independent field): rounding noise of the closed form, finite and >= 0
    x = [(np.arange(-1, n[d] + 1) + 0.5) * dx[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*x, indexing="ij")
    twod = np.stack([np.sin(20 * X) * np.cos(15 * Y), -np.cos(20 * X) * np.sin(15 * Y) + 0.3 * X, 0 * X], axis=-1)
    for P in (linear_velocity(n, dx, [[0, gamma, 0], [0, 0, 0], [0, 0, 0]]), linear_velocity(n, dx, [[0, -1.5, 0], [1.5, 0, 0], [0, 0, 0]]), twod):
        out = run(P, LN.SIGMA, 1.5)
        assert all(np.isfinite(o).all() and (o >= 0.0).all() for o in out)


def ghost_nan(a):
    a = a.copy()
    inner = a[1:-1, 1:-1, 1:-1].copy()
    a[...] = np.nan
    a[1:-1, 1:-1, 1:-1] = inner
    return a


def assert_face_and_edge_ghosts_finite(a, tag):
    """every ghost cell outside the box in one or two directions (corners are outside the stencil)"""
    b = a.copy()
    nan_corners(b)
    bad = ~np.isfinite(b)
    for i in (0, -1):
        for j in (0, -1):
            for k in (0, -1):
                bad[i, j, k, :] = False
    assert not bad.any(), (tag, np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("model", [LN.SMAGORINSKY, LN.SIGMA])
def test_operator_entry_periodic(gpu, model):
    lib = gpu
    from iamr_amd import ns as N
    n = (16, 16, 16)
    g = lib.Geom.make(n, prob_hi=(1.0, 1.2, 0.9))
    lay = lib.Layout.single(n)
    rng = np.random.default_rng(5)
    V = rng.standard_normal(n + (3,))
    vel = lib.MultiFab(lay, lib.CELL, 3, 1)
    vel.from_numpy(np.asfortranarray(ghost_nan(np.pad(V, ((1, 1),) * 3 + ((0, 0),), mode="wrap"))))
    mu = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
    N.calc_mut_les(g, vel, mu, model, CS[model])
    P = np.pad(V, ((1, 1),) * 3 + ((0, 0),), mode="wrap")
    check_faces(model, [m.to_numpy(0)[0] for m in mu], P, g.dx, CS[model], 0.0, "periodic")


@pytest.mark.parametrize("model", [LN.SMAGORINSKY, LN.SIGMA])
def test_operator_entry_cavity_walls(gpu, model):
    """x: no-slip walls, y: slip walls, z: no-slip wall below, the moving lid (u = 1) above.  Ghost cells = NaN except the boundary data the
    operator reads (the wall values of the Dirichlet components); iamrx_tensor_apply must leave every face and edge ghost cell finite, and
    iamrx_calc_mut_les must equal the yardstick on exactly those ghost cells."""
    lib = gpu
    from iamr_amd import ns as N
    n = (16, 16, 16)
    g = lib.Geom.make(n, prob_hi=(1.0, 1.2, 0.9), periodic=(0, 0, 0))
    lay = lib.Layout.single(n)
    # [component][direction]
    lobc = [[DIR, NEU, DIR], [DIR, DIR, DIR], [DIR, NEU, DIR]]
    hibc = [[DIR, NEU, DIR], [DIR, DIR, DIR], [DIR, NEU, DIR]]
    rng = np.random.default_rng(6)
    a = ghost_nan(rng.standard_normal(tuple(q + 2 for q in n) + (3,)))
    for c in range(3):
        for d in range(3):
            if lobc[c][d] != DIR:
                continue
            sl = [slice(None)] * 3
            sl[d] = 0; a[tuple(sl) + (c,)] = 0.0
            sl[d] = -1; a[tuple(sl) + (c,)] = 0.0
    a[:, :, -1, 0] = 1.0                                           # the lid
    a = np.asfortranarray(a)
    vel = lib.MultiFab(lay, lib.CELL, 3, 1); vel.from_numpy(a)
    vel2 = lib.MultiFab(lay, lib.CELL, 3, 1); vel2.from_numpy(a)
    eta = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
    for e in eta:
        e.setval(1.0)
    out = lib.MultiFab(lay, lib.CELL, 3, 0)
    N.tensor_apply(g, out, vel, 0.0, -1.0, None, eta, lobc=lobc, hibc=hibc, maxorder=3)
    P = vel.to_numpy(0)[0]
    assert_face_and_edge_ghosts_finite(P, "tensor_apply, cavity walls")
    assert np.array_equal(P[1:-1, 1:-1, 1:-1], a[1:-1, 1:-1, 1:-1])
    mu = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
    N.calc_mut_les(g, vel2, mu, model, CS[model], lobc=lobc, hibc=hibc, maxorder=3)
    check_faces(model, [m.to_numpy(0)[0] for m in mu], P, g.dx, CS[model], 0.0, "cavity")


@pytest.mark.parametrize("model", [LN.SMAGORINSKY, LN.SIGMA])
def test_operator_entry_refined_patch(gpu, model):
    """a 16^3 patch over 8^3 coarse cells inside a 16^3 coarse level: coarse/fine ghost cells on every side"""
    lib = gpu
    from iamr_amd import ns as N
    nf, nc = (32,) * 3, (16,) * 3
    gf, gc = lib.Geom.make(nf), lib.Geom.make(nc)
    lay, clay = lib.Layout([((8, 8, 8), (23, 23, 23))]), lib.Layout.single(nc)
    rng = np.random.default_rng(8)
    xc = (np.arange(-1, 17) + 0.5) / 16
    Xc, Yc, Zc = np.meshgrid(xc, xc, xc, indexing="ij")
    tp = 2 * np.pi
    Vc = np.stack([np.sin(tp * Xc) * np.cos(tp * Yc), np.cos(tp * (Yc + Zc)), 0.5 * np.sin(tp * (Xc - Zc))], axis=-1)
    cv = lib.MultiFab(clay, lib.CELL, 3, 1); cv.from_numpy(np.asfortranarray(Vc))
    a = np.asfortranarray(ghost_nan(rng.standard_normal((18, 18, 18, 3))))
    vel = lib.MultiFab(lay, lib.CELL, 3, 1); vel.from_numpy(a)
    vel2 = lib.MultiFab(lay, lib.CELL, 3, 1); vel2.from_numpy(a)
    eta = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
    for e in eta:
        e.setval(1.0)
    out = lib.MultiFab(lay, lib.CELL, 3, 0)
    N.tensor_apply_cf(gf, out, vel, 0.0, -1.0, None, eta, cv, gc, 2, maxorder=3)
    P = vel.to_numpy(0)[0]
    assert_face_and_edge_ghosts_finite(P, "tensor_apply_cf")
    mu = [lib.MultiFab(lay, lib.face(d), 1, 0) for d in range(3)]
    N.calc_mut_les(gf, vel2, mu, model, CS[model], maxorder=3, crse_vel=cv, cgeom=gc, ratio=2)
    check_faces(model, [m.to_numpy(0)[0] for m in mu], P, gf.dx, CS[model], 0.0, "refined patch")


VISC = 0.01


def tg_run(lib, N, nsteps, **kw):
    n = (16, 16, 16)
    g = lib.Geom.make(n)
    lay = lib.Layout.single(n)
    ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7, visc_coef=VISC, init_iter=2, **kw))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init()
    for _ in range(nsteps):
        ns.step()
        a, b, c = ns.stats()
        assert a.converged == 1 and b.converged == 1 and c.converged == 1
    return ns, n, g


@pytest.fixture(scope="module")
def tg_plain(gpu):
    from iamr_amd import ns as N
    ns, n, g = tg_run(gpu, N, 3)
    return ns.data(N.NavierStokes.S_NEW).gather_valid(n), ns.sum_integrated()[2]


def test_level_step_with_zero_constant_equals_the_uniform_path(gpu, tg_plain):
    """do_LES = 1 with Cs = 0: eta = visc_coef + 0 on arrays that are not marked uniform -- every viscous apply and solve takes the
    array-coefficient kernels; the project's full-step parity bar between two paths is 1e-8"""
    lib = gpu
    from iamr_amd import ns as N
    ns, n, g = tg_run(lib, N, 3, do_LES=1, LES_model=N.SMAGORINSKY, smago_Cs_cst=0.0)
    S = ns.data(N.NavierStokes.S_NEW).gather_valid(n)
    err = float(np.abs(S - tg_plain[0]).max())
    print("Cs = 0 against do_LES = 0:", err)
    assert err <= 1e-8
    for d in range(3):
        assert np.all(ns.data(N.NavierStokes.ETA_N + d).gather_valid(n) == VISC) and np.all(ns.data(N.NavierStokes.ETA_NP1 + d).gather_valid(n) == VISC)


def test_level_step_smagorinsky(gpu, tg_plain):
    lib = gpu
    from iamr_amd import ns as N
    ns, n, g = tg_run(lib, N, 3, do_LES=1, LES_model=N.SMAGORINSKY, smago_Cs_cst=0.18)
    So = ns.data(N.NavierStokes.S_OLD).gather_valid(n)[..., 0:3]
    P = np.pad(So, ((1, 1),) * 3 + ((0, 0),), mode="wrap")
    ref = LN.mu_faces(LN.SMAGORINSKY, P, g.dx, 0.18, VISC)
    for d in range(3):
        e_n = ns.data(N.NavierStokes.ETA_N + d).gather_valid(n)[..., 0]
        assert int(LN.ulp_diff(e_n, ref[d]).max()) <= 4, d
        e_p = ns.data(N.NavierStokes.ETA_NP1 + d).gather_valid(n)[..., 0]
        assert (e_n >= VISC).all() and (e_p >= VISC).all() and e_n.max() > 1.01 * VISC
    ke = ns.sum_integrated()[2]
    print("kinetic energy:", ke, "without LES:", tg_plain[1])
    assert np.isfinite(ke) and ke < tg_plain[1]


def test_eta_selectors_need_les(gpu):
    lib = gpu
    from iamr_amd import ns as N
    ns, n, g = tg_run(lib, N, 1)
    with pytest.raises(lib.IamrxError):
        ns.data(N.NavierStokes.ETA_N)


def smooth_eta(orc, lib, lay, n):
    eta_o, eta_d = [], []
    for d in range(3):
        t = orc.face(d)
        ax = [(np.arange(0, n[q] + t[q]) + (0.0 if t[q] else 0.5)) / n[q] for q in range(3)]
        Xf, Yf, Zf = np.meshgrid(*ax, indexing="ij")
        e = orc.Fab(n, t, 0, 1)
        e.a[..., 0] = 0.02 * (1.0 + (2.0 / 3.0) * np.sin(2 * np.pi * Xf) * np.cos(2 * np.pi * Yf) * np.cos(2 * np.pi * Zf))     # 5 : 1
        eta_o.append(e)
        m = lib.MultiFab(lay, t, 1, 0); m.set_from_global(e.a, e.lo); eta_d.append(m)
    return eta_o, eta_d


@pytest.mark.parametrize("case", ["one_box_40x24x16", "eight_boxes_16"])
def test_variable_viscosity_against_the_oracle(orc, gpu, case):
    """the array-coefficient tensor paths LES relies on (k_tensor_cross_zm<true>, k_tensor_cross<true>, the colour smoother on face arrays):
    apply to 1e-12, solve to 1e-9 of the oracle (the bars of tests/test_gpu_kernel_forms.py and DESIGN.md section 2)"""
    lib = gpu
    from iamr_amd import ns as N
    L = orc.lib()
    n = (40, 24, 16) if case.startswith("one") else (16, 16, 16)
    lay = lib.Layout.single(n) if case.startswith("one") else lib.Layout.decompose(n, 8)
    g_o, g_d = orc.geom(n), lib.Geom.make(n)
    x = [(np.arange(-1, n[d] + 1) + 0.5) / n[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*x, indexing="ij")
    tp = 2 * np.pi
    u = orc.Fab(n, orc.CELL, 1, 3)
    u.a[..., 0] = np.sin(tp * X) * np.cos(tp * Y) * np.cos(tp * Z)
    u.a[..., 1] = np.cos(2 * tp * X) * np.sin(tp * Y) + 0.3 * np.sin(tp * Z)
    u.a[..., 2] = 0.5 * np.sin(tp * (X + Y + Z))
    eta_o, eta_d = smooth_eta(orc, lib, lay, n)
    assert max(e.a.max() for e in eta_o) / min(e.a.min() for e in eta_o) > 4.5
    acoef = orc.Fab(n, orc.CELL, 0, 1)
    acoef.a[..., 0] = 1.0 + 0.2 * np.cos(tp * X[1:-1, 1:-1, 1:-1])
    y = orc.Fab(n, orc.CELL, 0, 3)
    L.orc_tensor_apply(C.byref(g_o), y.ref(), u.ref(), C.c_double(0.0), C.c_double(-1.0), None, orc.fabptrs(eta_o))
    u_d = lib.MultiFab(lay, lib.CELL, 3, 1); u_d.set_from_global(u.a, u.lo)
    out_d = lib.MultiFab(lay, lib.CELL, 3, 0)
    N.tensor_apply(g_d, out_d, u_d, 0.0, -1.0, None, eta_d)
    err = float(np.abs(out_d.gather_valid(n) - y.a).max() / np.abs(y.a).max())
    print(case, "apply:", err)
    assert err <= 1e-12
    rhs = orc.Fab(n, orc.CELL, 0, 3)
    rhs.a[...] = u.valid(n) * acoef.a
    z3 = orc.i3([0, 0, 0])
    s_o = u.copy()
    st_o = orc.CMgStats()
    oo = orc.mg_opts(maxorder=2)
    bval = 0.5                     # b eta / h^2 ~ 2.5 ... 15: the multigrid hierarchy runs (no diagonal shortcut)
    L.orc_tensor_solve(C.byref(g_o), s_o.ref(), rhs.ref(), C.c_double(1.0), C.c_double(bval), acoef.ref(), orc.fabptrs(eta_o), z3, z3,
                       C.c_double(1e-11), C.c_double(0.0), C.byref(oo), C.byref(st_o))
    assert st_o.converged == 1
    a_d = lib.MultiFab(lay, lib.CELL, 1, 0); a_d.set_from_global(acoef.a, acoef.lo)
    r_d = lib.MultiFab(lay, lib.CELL, 3, 0); r_d.set_from_global(rhs.a, rhs.lo)
    s_d = lib.MultiFab(lay, lib.CELL, 3, 1); s_d.set_from_global(u.a, u.lo)
    st = N.tensor_solve(g_d, s_d, r_d, 1.0, bval, a_d, eta_d, tol_rel=1e-11, tol_abs=0.0)
    assert st.converged == 1
    err = float(np.abs(s_d.gather_valid(n) - s_o.valid(n)).max() / np.abs(s_o.valid(n)).max())
    print(case, "solve:", err, "levels", st.nlevels, "iters", st.iters, st_o.iters)
    assert err <= 1e-9


def hotspot_run(lib, N, do_les):
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    inp = Inputs([os.path.join(HERE, "golden", "inputs.3d.LES_hotspot")], ["ns.do_LES=0", "amr.derive_plot_vars=mag_vort avg_pressure"])
    pr = inp.problem()
    assert pr["params"]["LES_model"] == N.SIGMA and tuple(pr["n"]) == (32, 32, 32)
    pr["params"]["do_LES"] = do_les
    ns, lay, g, pr = R.build(inp, lib, N, pr=pr)
    ns.post_init(pr["stop_time"])
    for _ in range(2):
        ns.step()
        for st in ns.stats():
            assert st.converged == 1
    return ns, pr


def test_tutorial_fixture_with_the_sigma_model(gpu):
    lib = gpu
    from iamr_amd import ns as N
    ns, pr = hotspot_run(lib, N, 1)
    n = tuple(pr["n"])
    S = ns.data(N.NavierStokes.S_NEW).gather_valid(n)
    assert np.isfinite(S).all()
    visc = pr["params"]["visc_coef"]
    for w in range(13, 19):
        e = ns.data(w).gather_valid(n)
        assert np.isfinite(e).all() and (e >= visc).all(), w
    assert max(ns.data(13 + d).gather_valid(n).max() for d in range(3)) > visc
    ns0, _ = hotspot_run(lib, N, 0)
    S0 = ns0.data(N.NavierStokes.S_NEW).gather_valid(n)
    diff = float(np.abs(S[..., 0:3] - S0[..., 0:3]).max())
    print("hot spot, 2 steps: largest velocity difference LES - no LES:", diff)
    assert diff > 0.0


def test_two_levels_with_smagorinsky(gpu):
    """inputs.3d.taylorgreen_amr16 with nu = 0.01, two levels, one coarse step: the viscous flux registers carry the varying eta, so the
    composite momentum drifts no more than without LES (x 10, floor 1e-12); mass is conserved to round-off"""
    lib = gpu
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs

    def run(do_les):
        inp = Inputs([os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")], ["ns.vel_visc_coef=0.01", "amr.max_level=1"])
        pr = inp.problem()
        pr["params"].update(do_LES=do_les, LES_model=N.SMAGORINSKY)
        amr, lays, g0 = R.build_amr(pr, lib, N)
        assert amr.nlev == 2
        amr.post_init(-1.0)
        fb = pr["fine_boxes"][0]
        cov = np.zeros((16, 16, 16), dtype=bool)
        for lo, hi in fb:
            cov[lo[0] // 2:hi[0] // 2 + 1, lo[1] // 2:hi[1] // 2 + 1, lo[2] // 2:hi[2] // 2 + 1] = True
        fmask = np.zeros((32, 32, 32), dtype=bool)
        for lo, hi in fb:
            fmask[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True

        def sums():
            Sc = amr.levels[0].data(0).gather_valid((16,) * 3)
            Sf = amr.levels[1].data(0).gather_valid((32,) * 3)
            assert np.isfinite(Sc).all() and np.isfinite(Sf[fmask]).all()
            hc, hf = (1.0 / 16) ** 3, (1.0 / 32) ** 3
            mass = Sc[..., 3][~cov].sum() * hc + Sf[..., 3][fmask].sum() * hf
            mom = [(Sc[..., 3] * Sc[..., c])[~cov].sum() * hc + (Sf[..., 3] * Sf[..., c])[fmask].sum() * hf for c in range(3)]
            return mass, np.array(mom)
        m0, p0 = sums()
        amr.coarse_step()
        for lev in amr.levels:
            for st in lev.stats():
                assert st.converged == 1
        a, b = amr.sync_stats()
        assert a.converged == 1 and b.converged == 1
        m1, p1 = sums()
        return abs(m1 - m0), float(np.abs(p1 - p0).max()), amr
    dm0, dp0, _ = run(0)
    dm1, dp1, amr = run(1)
    print("two levels: mass drift", dm1, "momentum drift with LES", dp1, "without", dp0)
    assert dm1 <= 1e-13
    assert dp1 <= 10 * max(dp0, 1e-12)
    for l in range(2):
        e = amr.levels[l].data(N.NavierStokes.ETA_N)
        for li in range(e.nlocal()):
            a = e.to_numpy(li)[0]
            assert np.isfinite(a).all() and (a >= 0.01).all() and a.max() > 0.01
