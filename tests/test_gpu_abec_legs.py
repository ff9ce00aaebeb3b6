"""The coarse levels of the cell-centred V-cycle as two launches per level (k_abec_legs.hip, IAMRX_MG_LEGS) against the ten launches they
replace.  The leg kernels keep the expressions and the order of the colour passes, the residual, the restriction and the prolongation, so
a solve is the same solve bit for bit: solution, cycles and final residual norm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STORED, UNIFORM = 0, 2


def leg_levels(lib, n, levels, nu1, nu2, coef, has_a):
    """the host query's answer for the levels n / 2^l, l in levels"""
    out = []
    for l in levels:
        m = tuple(v >> l for v in n)
        out.append(lib.host_abec_leg_plan(lib.Geom.make(m), [((0, 0, 0), tuple(v - 1 for v in m))], l, nu1=nu1, nu2=nu2, coef=coef, has_a=has_a)["legs"])
    return out


def with_keys(lib, keys, fn):
    old = {k: lib.tuning_get(k, 1) for k in keys}
    try:
        for k, v in keys.items():
            lib.tuning_set(k, v)
        return fn()
    finally:
        for k, v in old.items():
            lib.tuning_set(k, v)


def fields(n, const_b=None):
    """smooth positive face coefficients, different on every face and in every direction, a positive a-term and a right-hand side"""
    rng = np.random.default_rng(7)
    X = [(np.arange(n[d] + 1)) / n[d] for d in range(3)]          # faces
    Xc = [(np.arange(n[d]) + 0.5) / n[d] for d in range(3)]       # centres
    b = []
    for d in range(3):
        x = [X[e] if e == d else Xc[e] for e in range(3)]
        f = (1.0 + 0.1 * d + 0.3 * np.sin(2 * np.pi * (x[0][:, None, None] + 0.1 * d)) * np.cos(2 * np.pi * (x[1][None, :, None] - 0.07))
             + 0.2 * np.sin(2 * np.pi * (2 * x[2][None, None, :] + 0.3 * d)) + 0.15 * np.cos(2 * np.pi * (x[0][:, None, None] + x[1][None, :, None] + x[2][None, None, :])))
        b.append(np.full_like(f, const_b) if const_b is not None else f)
    a = 1.0 + 0.4 * np.sin(2 * np.pi * Xc[0])[:, None, None] * np.sin(2 * np.pi * (Xc[1][None, :, None] + Xc[2][None, None, :]))
    r = rng.standard_normal(n)
    return b, a, r - r.mean()


def solve(lib, n, b, a, r, alpha, nu1, nu2):
    g = lib.Geom.make(n, prob_hi=tuple(v / n[0] for v in n))
    lay = lib.Layout.single(n)
    b_d = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 0); m.set_from_global(b[d][..., None], (0, 0, 0))
        b_d.append(m)
    a_d = None
    if alpha:
        a_d = lib.MultiFab(lay, lib.CELL, 1, 0); a_d.set_from_global(a[..., None], (0, 0, 0))
    rhs = lib.MultiFab(lay, lib.CELL, 1, 0); rhs.set_from_global(r[..., None], (0, 0, 0))
    phi = lib.MultiFab(lay, lib.CELL, 1, 1); phi.setval(0.0)
    st = lib.abec_solve(g, alpha, 1.0, a_d, b_d, phi, rhs, rtol=1e-10, atol=1e-16, opts=lib.mg_opts(nu1=nu1, nu2=nu2))
    assert st.converged >= 1
    return st.iters, st.resnorm, st.nlevels, phi.gather_valid(n)[..., 0]


# shape, (nu1, nu2), the levels that must take legs
CASES = [
    ((64, 64, 64), (2, 2), (1, 2)),         # 32^3 and 16^3 (the region is the whole level) above the 8^3 device bottom
    ((48, 48, 48), (2, 2), (1, 2)),         # 24^3 and 12^3: partial tiles, a level shorter than the region
    ((96, 48, 32), (2, 2), (1, 2, 3)),      # (48,24,16), (24,12,8), (12,6,4): anisotropic, directions held two and four times in the region
    ((72, 72, 72), (2, 2), (1, 2)),         # 36^3 and 18^3 above a 9^3 bottom that the device bottom solver does not take: host Krylov bottom
    ((64, 64, 64), (1, 1), (1, 2)),
    ((64, 64, 64), (2, 1), (1, 2)),
    ((64, 64, 64), (3, 3), (1, 2)),         # tiles of 4^3 in a halo of 6
]


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("n, nu, levels", CASES)
def test_solve_is_the_same_with_legs(gpu, n, nu, levels, alpha):
    lib = gpu
    assert leg_levels(lib, n, levels, nu[0], nu[1], STORED, alpha != 0.0) == [True] * len(levels)
    b, a, r = fields(n)
    off = with_keys(lib, {"MG_LEGS": 0}, lambda: solve(lib, n, b, a, r, alpha, *nu))
    on = with_keys(lib, {"MG_LEGS": 1}, lambda: solve(lib, n, b, a, r, alpha, *nu))
    assert on[2] == off[2] == len(levels) + 2
    assert on[0] == off[0] and on[1] == off[1], (on[:2], off[:2])
    assert np.array_equal(on[3], off[3]), float(np.abs(on[3] - off[3]).max())


def test_a_cycle_shape_the_tile_cannot_hold_keeps_its_launches(gpu):
    lib = gpu
    n = (64, 64, 64)
    assert leg_levels(lib, n, (1, 2), 4, 4, STORED, False) == [False, False]
    b, a, r = fields(n)
    off = with_keys(lib, {"MG_LEGS": 0}, lambda: solve(lib, n, b, a, r, 0.0, 4, 4))
    on = with_keys(lib, {"MG_LEGS": 1}, lambda: solve(lib, n, b, a, r, 0.0, 4, 4))
    assert on[:2] == off[:2] and np.array_equal(on[3], off[3])


def test_uniform_coefficients_on_the_coarse_levels(gpu):
    """the scalar-diffusion operator: constant b and an a-term.  The coarse levels take the constants (IAMRX_MG_COARSE_UNIFORM = 1) or
    their arrays, with legs or without: four forms of one solve"""
    lib = gpu
    n = (64, 64, 64)
    assert leg_levels(lib, n, (1, 2), 2, 2, UNIFORM, True) == [True, True] and leg_levels(lib, n, (1, 2), 2, 2, STORED, True) == [True, True]
    b, a, r = fields(n, const_b=0.7)
    runs = {}
    for uni in (1, 0):
        for legs in (0, 1):
            runs[uni, legs] = with_keys(lib, {"MG_COARSE_UNIFORM": uni, "MG_LEGS": legs}, lambda: solve(lib, n, b, a, r, 1.0, 2, 2))
    ref = runs[1, 0]
    for key, got in runs.items():
        assert got[:3] == ref[:3], (key, got[:3], ref[:3])
        assert np.array_equal(got[3], ref[3]), (key, float(np.abs(got[3] - ref[3]).max()))


def test_whole_step_is_the_same_with_legs(gpu):
    """two steps of a variable-density, viscous, diffusive run on one periodic box of 128 x 32 x 32: the MAC solve's coarse levels
    (64,16,16) and (32,8,8) hold stored coefficients, those of the tracer's diffusion solve constants and an a-term"""
    lib = gpu
    from iamr_amd import ns as N
    n = (128, 32, 32)
    assert leg_levels(lib, n, (1, 2), 2, 2, STORED, False) == [True, True]

    def run():
        g = lib.Geom.make(n, prob_hi=(n[0] / 32.0, 1.0, 1.0))
        lay = lib.Layout.single(n)
        ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.5, visc_coef=2e-2, tracer_diff_coef=1e-2, init_iter=1))
        ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
        m = ns.data(N.NavierStokes.S_NEW)
        G = np.zeros(tuple(v + 2 for v in n) + (5,), order="F")
        G[1:-1, 1:-1, 1:-1] = m.gather_valid(n)
        x = (np.arange(n[0]) + 0.5) / n[0]
        G[1:-1, 1:-1, 1:-1, 3] = 1.0 + 0.3 * np.sin(2 * np.pi * x)[:, None, None]
        m.set_from_global(G, (-1, -1, -1))
        ns.set_data(N.NavierStokes.S_NEW, m)
        ns.post_init(-1.0)
        dts = [ns.step() for _ in range(2)]
        return dts, ns.data(N.NavierStokes.S_NEW).gather_valid(n), ns.data(N.NavierStokes.P_NEW).gather_valid(n)[..., 0]

    dts0, S0, P0 = with_keys(lib, {"MG_LEGS": 0}, run)
    dts, S, P = with_keys(lib, {"MG_LEGS": 1}, run)
    assert dts == dts0
    assert np.array_equal(S, S0), float(np.abs(S - S0).max())
    assert np.array_equal(P, P0), float(np.abs(P - P0).max())
