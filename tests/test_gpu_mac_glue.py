"""The passes around the V-cycles of the MAC projection (IAMRX_MAC_GLUE).  With the switch on, mlmg_mac_solve hands the
solver the density alone: no finest-level face arrays (CellMG::prepare makes them only for a kernel that reads them), the level-1
coefficients averaged straight from the density, the face velocities updated by one launch that forms b in place.  Every expression is the
one it replaces, so a solve is the same solve bit for bit -- potential, face velocities, cycles, residual norm -- on every path the finest
level can take.  The switch-less part of the change (the right-hand side chain of CellMG::solve, the norms of the viscous solve) is pinned
by values recorded with the build before it (tests/golden/mac_glue_tensor_velocity.npy)."""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PERIODIC, DIRICHLET, NEUMANN = 0, 101, 102
COUNTERS = ("MAC_GLUE_NO_ARRAYS", "MAC_GLUE_MATERIALISED", "MAC_GLUE_LEVEL1", "MAC_GLUE_FLUX")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mac_glue_tensor_velocity.npy")


def with_keys(lib, keys, fn):
    old = {k: lib.tuning_get(k, 1) for k in keys}
    try:
        for k, v in keys.items():
            lib.tuning_set(k, v)
        return fn()
    finally:
        for k, v in old.items():
            lib.tuning_set(k, v)


def wrap(a, n, per):
    """periodic images in the ghost layer of a (n + 2)^3 array along the periodic directions"""
    for d in range(3):
        if per[d]:
            lo = [slice(None)] * 3; hi = [slice(None)] * 3; s0 = [slice(None)] * 3; s1 = [slice(None)] * 3
            lo[d] = 0; s0[d] = n[d]; hi[d] = n[d] + 1; s1[d] = 1
            a[tuple(lo)] = a[tuple(s0)]; a[tuple(hi)] = a[tuple(s1)]
    return a


def inputs(n, per, lobc, hibc, seed):
    """a random density in [0.5, 2] with its ghost layer (periodic images; beyond a wall whatever a fill left there), random face
    velocities (zero through Neumann walls, one value on a periodic face and its image), a random divergence source"""
    rng = np.random.default_rng(seed)
    rho = wrap(0.5 + 1.5 * rng.random(tuple(v + 2 for v in n)), n, per)
    um = []
    for d in range(3):
        u = rng.standard_normal(tuple(n[e] + (1 if e == d else 0) for e in range(3)))
        s0 = [slice(None)] * 3; s1 = [slice(None)] * 3; s0[d] = 0; s1[d] = n[d]
        if per[d]:
            u[tuple(s1)] = u[tuple(s0)]
        else:
            if lobc[d] == NEUMANN: u[tuple(s0)] = 0.0
            if hibc[d] == NEUMANN: u[tuple(s1)] = 0.0
        um.append(u)
    S = 0.1 * rng.standard_normal(n)
    return rho, um, S - S.mean()


def counters(lib):
    return [lib.tuning_get(k, 0) for k in COUNTERS]


def fab_bytes(m):
    return [m.to_numpy(li)[0].copy() for li in range(m.nlocal())]


def mac_solve(lib, n, lay, per, lobc, hibc, rho, um, S, rho_ng=1):
    g = lib.Geom.make(n, prob_hi=tuple(v / n[0] for v in n), periodic=per)
    rho_d = lib.MultiFab(lay, lib.CELL, 1, rho_ng)
    if rho_ng:
        rho_d.set_from_global(rho[..., None], (-1, -1, -1))
    else:
        rho_d.set_from_global(rho[1:-1, 1:-1, 1:-1, None], (0, 0, 0))
    um_d = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 0)
        m.set_from_global(um[d][..., None], (0, 0, 0))
        um_d.append(m)
    S_d = None
    if S is not None:
        S_d = lib.MultiFab(lay, lib.CELL, 1, 0); S_d.set_from_global(S[..., None], (0, 0, 0))
    phi_d = lib.MultiFab(lay, lib.CELL, 1, 1); phi_d.setval(0.0)
    c0 = counters(lib)
    st = lib.mlmg_mac_solve(g, um_d, rho_d, 0, S_d, phi_d, 200.0, lobc=lobc, hibc=hibc, mac_tol=1e-9, opts=lib.mg_opts(maxorder=3))
    moved = [int(b - a) for a, b in zip(c0, counters(lib))]
    return dict(iters=st.iters, converged=st.converged, resnorm=st.resnorm, nlevels=st.nlevels, phi=fab_bytes(phi_d), um=[fab_bytes(m) for m in um_d]), moved


def same_solve(on, off):
    assert on["converged"] >= 1 and off["converged"] >= 1
    assert (on["iters"], on["converged"], on["nlevels"]) == (off["iters"], off["converged"], off["nlevels"])
    assert on["resnorm"] == off["resnorm"], (on["resnorm"], off["resnorm"])
    for a, b in zip(on["phi"], off["phi"]):
        assert np.array_equal(a, b), float(np.abs(a - b).max())
    for d in range(3):
        for a, b in zip(on["um"][d], off["um"][d]):
            assert np.array_equal(a, b), (d, float(np.abs(a - b).max()))
    assert max(float(np.abs(a).max()) for a in on["phi"]) > 0.0


# name: domain, box size (None: one box), periodic flags, low / high conditions, boxes kept as boxes
CASES = {
    # the flagship's path in miniature: the one-launch sweep in the density form, fused residual + restriction, the device bottom
    "128x16x16 periodic": ((128, 16, 16), None, (1, 1, 1), (PERIODIC,) * 3, (PERIODIC,) * 3, False),
    # the finest level takes the colour passes, in their density form: still no reader of the face arrays
    "32^3 periodic, colour passes": ((32, 32, 32), None, (1, 1, 1), (PERIODIC,) * 3, (PERIODIC,) * 3, False),
    "128x16x16 walls in y and z": ((128, 16, 16), None, (1, 0, 0), (PERIODIC, NEUMANN, NEUMANN), (PERIODIC, NEUMANN, NEUMANN), False),
    # a Dirichlet face: a non-singular solve, no mean removed, the separate max norm of the right-hand side
    "128x16x16 walls, outflow on z high": ((128, 16, 16), None, (1, 0, 0), (PERIODIC, NEUMANN, NEUMANN), (PERIODIC, NEUMANN, DIRICHLET), False),
    # the sweep on several boxes, which keeps its own copy of the density
    "two boxes of 128x16x16 in z": ((128, 16, 32), (128, 16, 16), (1, 1, 1), (PERIODIC,) * 3, (PERIODIC,) * 3, True),
}


@pytest.mark.parametrize("source", [False, True], ids=["no S", "S"])
@pytest.mark.parametrize("case", list(CASES))
def test_mac_solve_is_the_same_without_the_face_arrays(gpu, case, source):
    lib = gpu
    n, box, per, lobc, hibc, kept = CASES[case]
    rho, um, S = inputs(n, per, lobc, hibc, 11)

    def run():
        lay = lib.Layout.single(n) if box is None else lib.Layout.decompose(n, box)
        assert lay.nlocal() == (1 if box is None else 2)
        return mac_solve(lib, n, lay, per, lobc, hibc, rho, um, S if source else None)

    keys = {"COALESCE": 0} if kept else {}
    off, moved_off = with_keys(lib, dict(keys, MAC_GLUE=0), run)
    on, moved_on = with_keys(lib, dict(keys, MAC_GLUE=1), run)
    assert moved_off == [0, 0, 0, 0]
    # the new path really ran: no arrays, none made on the way, level 1 from the density, one flux launch
    assert moved_on == [1, 0, 1, 1], moved_on
    assert on["nlevels"] >= 2
    same_solve(on, off)


def test_a_density_without_ghost_cells_is_refused(gpu):
    """the face average of the density reads one cell beyond every box face (include/iamrx.h: "rho needs 1 filled ghost"): without a
    ghost layer there is no density form and no face array either, and mlmg_mac_solve says so under both settings instead of reading
    outside the array"""
    lib = gpu
    n, per, bc = (128, 16, 16), (1, 1, 1), (PERIODIC,) * 3
    rho, um, S = inputs(n, per, bc, bc, 14)
    for glue in (0, 1):
        with pytest.raises(Exception, match="one filled ghost layer"):
            with_keys(lib, {"MAC_GLUE": glue}, lambda: mac_solve(lib, n, lib.Layout.single(n), per, bc, bc, rho, um, None, rho_ng=0))


@pytest.mark.parametrize("why", ["IAMRX_ABEC_SIG = 0", "one level: the device bottom solver"])
def test_prepare_makes_the_arrays_for_a_kernel_that_reads_them(gpu, why):
    """the decision of CellMG::prepare: the stored-coefficient kernels (ABEC_SIG = 0) and the device bottom solver on a hierarchy of one
    level read face arrays -- the solver makes them itself and the solve is the one of MAC_GLUE = 0"""
    lib = gpu
    n = (32, 32, 32) if why.startswith("IAMRX") else (8, 8, 8)
    per, bc = (1, 1, 1), (PERIODIC,) * 3
    rho, um, S = inputs(n, per, bc, bc, 12)
    keys = {"ABEC_SIG": 0} if why.startswith("IAMRX") else {}
    run = lambda: mac_solve(lib, n, lib.Layout.single(n), per, bc, bc, rho, um, None)
    off, moved_off = with_keys(lib, dict(keys, MAC_GLUE=0), run)
    on, moved_on = with_keys(lib, dict(keys, MAC_GLUE=1), run)
    assert moved_off == [0, 0, 0, 0]
    assert moved_on == [0, 1, 0, 1], moved_on          # arrays made, level 1 (if any) averaged from them, the one flux launch
    assert (on["nlevels"] == 1) == (n[0] == 8)
    same_solve(on, off)


@pytest.mark.parametrize("source", [False, True], ids=["no S", "S"])
def test_mac_solve_on_a_refined_box_is_the_same(gpu, source):
    """mlmg_mac_solve_cf: a refined box of 128 x 16 x 16 strictly inside a 128 x 32 x 32 coarse domain (the sweep with in-kernel coarse/fine values)"""
    lib = gpu
    nc = (128, 32, 32)
    n = tuple(2 * v for v in nc)
    box = ((64, 24, 24), (191, 39, 39))
    g_d, gc_d = lib.Geom.make(n, prob_hi=(4.0, 1.0, 1.0)), lib.Geom.make(nc, prob_hi=(4.0, 1.0, 1.0))
    rng = np.random.default_rng(13)
    rho = 0.5 + 1.5 * rng.random(tuple(v + 2 for v in n))
    um = [rng.standard_normal(tuple(n[e] + (1 if e == d else 0) + 2 for e in range(3))) for d in range(3)]
    S = 0.1 * rng.standard_normal(n)
    cphi = rng.standard_normal(tuple(v + 2 for v in nc))

    def run():
        lay, clay = lib.Layout([box]), lib.Layout.single(nc)
        um_d = []
        for d in range(3):
            m = lib.MultiFab(lay, lib.face(d), 1, 1)
            m.set_from_global(um[d][..., None], (-1, -1, -1))
            um_d.append(m)
        rho_d = lib.MultiFab(lay, lib.CELL, 1, 1); rho_d.set_from_global(rho[..., None], (-1, -1, -1))
        S_d = None
        if source:
            S_d = lib.MultiFab(lay, lib.CELL, 1, 0); S_d.set_from_global(S[..., None], (0, 0, 0))
        phi_d = lib.MultiFab(lay, lib.CELL, 1, 1); phi_d.setval(0.0)
        cphi_d = lib.MultiFab(clay, lib.CELL, 1, 1); cphi_d.set_from_global(cphi[..., None], (-1, -1, -1))
        c0 = counters(lib)
        st = lib.mlmg_mac_solve_cf(g_d, um_d, rho_d, 0, S_d, phi_d, 200.0, cphi_d, gc_d, 2, mac_tol=1e-9)
        moved = [int(b - a) for a, b in zip(c0, counters(lib))]
        return dict(iters=st.iters, converged=st.converged, resnorm=st.resnorm, nlevels=st.nlevels, phi=fab_bytes(phi_d), um=[fab_bytes(m) for m in um_d]), moved

    off, moved_off = with_keys(lib, {"MAC_GLUE": 0}, run)
    on, moved_on = with_keys(lib, {"MAC_GLUE": 1}, run)
    assert moved_off == [0, 0, 0, 0] and moved_on == [1, 0, 1, 1], (moved_off, moved_on)
    same_solve(on, off)


@pytest.mark.parametrize("boxes", ["one box", "eight boxes kept"])
def test_mac_sync_solve_and_its_fluxes_are_the_same(gpu, boxes):
    """mac_sync_solve goes through mlmg_mac_solve with a source, no velocity and the FLUX outputs (Ucorr): with the switch on it takes the
    density path too, and the one flux launch fills flux[d] -- the same bytes as the three launches on the face arrays"""
    lib = gpu
    nc, n = (32, 32, 32), (64, 64, 64)
    gc = lib.Geom.make(nc)
    fbox = [((16, 16, 16), (47, 47, 47))]
    rng = np.random.default_rng(15)
    rho = wrap(0.5 + 1.5 * rng.random(tuple(v + 2 for v in nc)), nc, (1, 1, 1))
    uc = [rng.standard_normal(tuple(nc[e] + (1 if e == d else 0) for e in range(3))) for d in range(3)]
    uf = [rng.standard_normal(tuple(n[e] + (1 if e == d else 0) for e in range(3))) for d in range(3)]
    dt, dc = 0.01, 1.0 / nc[0]

    def run():
        clay = lib.Layout.single(nc) if boxes == "one box" else lib.Layout.decompose(nc, 16)
        assert clay.nlocal() == (1 if boxes == "one box" else 8)
        flay = lib.Layout(fbox)
        mr = lib.FluxRegister(flay, clay, gc, 2, 1)
        mr.setVal(0.0)
        for d in range(3):
            c = lib.MultiFab(clay, lib.face(d), 1, 0); c.set_from_global(uc[d][..., None], (0, 0, 0))
            f = lib.MultiFab(flay, lib.face(d), 1, 0); f.set_from_global(uf[d][..., None], (0, 0, 0))
            mr.CrseInit(c, d, 0, 0, 1, -dc * dc)
            mr.FineAdd(f, d, 0, 0, 1, 0.25 * dc * dc)
        rho_d = lib.MultiFab(clay, lib.CELL, 1, 1); rho_d.set_from_global(rho[..., None], (-1, -1, -1))
        ucorr = [lib.MultiFab(clay, lib.face(d), 1, 0) for d in range(3)]
        for m in ucorr:
            m.setval(0.0)
        sync_phi = lib.MultiFab(clay, lib.CELL, 1, 1)
        c0 = counters(lib)
        st = lib.mac_sync_solve(gc, mr, rho_d, dt, flay, ucorr, sync_phi, tol=1e-9)
        moved = [int(b - a) for a, b in zip(c0, counters(lib))]
        return dict(iters=st.iters, converged=st.converged, resnorm=st.resnorm, nlevels=st.nlevels, phi=fab_bytes(sync_phi), um=[fab_bytes(m) for m in ucorr]), moved

    keys = {} if boxes == "one box" else {"COALESCE": 0}
    off, moved_off = with_keys(lib, dict(keys, MAC_GLUE=0), run)
    on, moved_on = with_keys(lib, dict(keys, MAC_GLUE=1), run)
    assert moved_off == [0, 0, 0, 0] and moved_on == [1, 0, 1, 1], (moved_off, moved_on)
    same_solve(on, off)
    assert max(float(np.abs(a).max()) for a in on["um"][0]) > 0.0


# ---- the viscous solve: no switch, so against the values of the build before the change -------------------------------------------
TENSOR_CASES = ["periodic", "walls in z"]


def tensor_velocity(lib, case, nan_at=None):
    """Diffusion::diffuse_tensor_velocity at 32^3 through its C-ABI entry.  periodic: the multigrid hierarchy; walls in z (no slip), a small
    viscosity: the diagonally dominant shortcut, whose sweep count comes from the reduction of 1 / a"""
    N = 32
    n = (N, N, N)
    walls = case == "walls in z"
    per = (1, 1, 0) if walls else (1, 1, 1)
    g = lib.Geom.make(n, periodic=per)
    lay = lib.Layout.single(n)
    rng = np.random.default_rng(21)
    x = (np.arange(N + 2) - 0.5) / N
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    tp = 2 * np.pi
    rho_o = 1.0 + 0.3 * np.sin(tp * X) * np.cos(tp * Y)
    rho_n = 1.0 + 0.3 * np.sin(tp * (X - 0.05)) * np.cos(tp * Y)

    def vel(sh):
        v = np.stack([np.sin(tp * (X - sh)) * np.cos(tp * Y) * np.sin(tp * Z), -np.cos(tp * (X - sh)) * np.sin(tp * Y) * np.sin(tp * Z),
                      0.3 * np.sin(tp * Z) * np.cos(2 * tp * Y)], axis=-1)
        v = v + 0.05 * wrap(rng.standard_normal(X.shape), n, (1, 1, 1))[..., None]
        if walls:
            v[:, :, 0] = 0.0; v[:, :, -1] = 0.0
        return v

    Uo = np.concatenate([vel(0.0), rho_o[..., None]], axis=-1)
    Us = np.concatenate([vel(0.02), rho_n[..., None]], axis=-1)
    if nan_at is not None:
        Us[nan_at + (1,)] = np.nan
    rh = 0.5 * (rho_o + rho_n)[..., None]
    mu, dt, theta = (0.001 if walls else 0.02), 0.02, 0.5

    def mf(arr, ng):
        m = lib.MultiFab(lay, lib.CELL, arr.shape[-1], ng)
        m.set_from_global(arr, (-ng, -ng, -ng) if ng else (0, 0, 0))
        return m

    U_old, U_new, rho_half = mf(Uo, 1), mf(Us, 1), mf(rh, 1)
    eta = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 0)
        m.setval(mu)
        eta.append(m)
    bc = (PERIODIC, PERIODIC, DIRICHLET if walls else PERIODIC) * 3
    st = lib.diffuse_tensor_velocity(g, U_old, U_new, 3, dt, theta, rho_half, 1, eta, eta_n=eta, lobc=bc, hibc=bc, visc_tol=1e-11,
                                     fill_new=lambda: U_new.fill_boundary(g))
    out = U_new.gather_valid(n)[..., :3]
    # the record: a sample of the solution (every second cell in y, every fourth in x and z), the cycle count and the residual norm
    return np.concatenate([out[1::4, ::2, 2::4].ravel(), [float(st.iters), float(st.converged), st.resnorm, float(st.nlevels)]])


@pytest.mark.parametrize("case", TENSOR_CASES)
def test_viscous_solve_keeps_its_numbers(gpu, case):
    want = np.load(GOLDEN)[TENSOR_CASES.index(case)]
    got = tensor_velocity(gpu, case)
    assert got[-3] >= 1.0
    assert np.array_equal(got[-4:], want[-4:]), (got[-4:], want[-4:])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), float(np.abs(got - want).max())


def test_a_nan_in_the_viscous_right_hand_side_is_still_an_error(gpu):
    with pytest.raises(Exception, match="not finite"):
        tensor_velocity(gpu, "periodic", nan_at=(7, 9, 11))
