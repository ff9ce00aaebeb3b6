"""Two switches of the cell-centred multigrid's smoother path inside a whole solve: the one-launch red + black sweep on a box spanning its
domain (IAMRX_GSRB_RB) against the two colour passes, and the colour passes that apply the domain walls themselves
(IAMRX_GSRB_WALLS_INKERNEL) against a ghost fill in front of each pass.  Either way a sweep forms the same doubles, so the solve is the same
solve bit for bit: cycles and solution -- the bound of the on / off tests of the other paths (tests/test_gpu_rb_nbr.py, tests/test_gpu_cf_abec.py).
CellMG::prepare() chooses the path once per level per solve: a key flipped between two solves of one process shows in the second."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEUMANN, DIRICHLET = 102, 101


def on_and_off(lib, key, solve):
    out = {}
    for v in (1, 0):
        old = lib.tuning_get(key, 1)
        lib.tuning_set(key, v)
        try:
            out[v] = solve()
        finally:
            lib.tuning_set(key, old)
    assert out[1][0] == out[0][0], (key, out[1][0], out[0][0])
    for a, b in zip(out[1][1], out[0][1]):
        assert np.array_equal(a, b), (key, float(np.abs(a - b).max()))


@pytest.mark.parametrize("walls", [False, True])
def test_mac_solve_does_not_depend_on_the_sweep_kernel_of_a_box(gpu, walls):
    """MAC projection (density form) on one box of 128 x 16 x 16, periodic (16 wavefronts, index wrap) and with Neumann walls (12 wavefronts,
    wall formulas in the kernel)"""
    lib = gpu
    n = (128, 16, 16)
    per = (0, 0, 0) if walls else (1, 1, 1)
    bc = tuple(0 if p else NEUMANN for p in per)
    g = lib.Geom.make(n, prob_hi=tuple(v / n[0] for v in n), periodic=per)
    lay = lib.Layout.single(n)
    rng = np.random.default_rng(41)
    rho = 1.0 + 0.5 * rng.random(tuple(v + 2 for v in n))
    if not walls:
        rho = np.pad(rho[1:-1, 1:-1, 1:-1], 1, mode="wrap")
    um = []
    for d in range(3):
        u = rng.standard_normal(tuple(n[e] + (1 if e == d else 0) for e in range(3)))
        lo = [slice(None)] * 3; hi = [slice(None)] * 3; lo[d] = 0; hi[d] = n[d]
        if walls:
            u[tuple(lo)] = 0.0; u[tuple(hi)] = 0.0
        else:
            u[tuple(hi)] = u[tuple(lo)]
        um.append(u)

    def solve():
        rho_d = lib.MultiFab(lay, lib.CELL, 1, 1); rho_d.set_from_global(rho[..., None], (-1,) * 3)
        um_d = []
        for d in range(3):
            m = lib.MultiFab(lay, lib.face(d), 1, 0); m.set_from_global(um[d][..., None], (0, 0, 0))
            um_d.append(m)
        phi_d = lib.MultiFab(lay, lib.CELL, 1, 1); phi_d.setval(0.0)
        st = lib.mlmg_mac_solve(g, um_d, rho_d, 0, None, phi_d, 200.0, lobc=bc, hibc=bc, mac_tol=1e-10, opts=lib.mg_opts(maxorder=3))
        assert st.converged >= 1
        return st.iters, [phi_d.gather_valid(n)] + [m.gather_valid(n) for m in um_d]
    on_and_off(lib, "GSRB_RB", solve)


def test_abec_solve_does_not_depend_on_where_the_walls_are_applied(gpu):
    """stored face coefficients on one box of 32 x 16 x 16 with Dirichlet walls: the plane-pipelined colour pass with the wall table
    against the same pass behind a ghost fill"""
    lib = gpu
    n = (32, 16, 16)
    bc = (DIRICHLET,) * 3
    g = lib.Geom.make(n, prob_hi=tuple(v / n[0] for v in n), periodic=(0, 0, 0))
    lay = lib.Layout.single(n)
    rng = np.random.default_rng(43)
    b = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 0)
        m.set_from_global(1.0 + 0.5 * rng.random(tuple(n[e] + (1 if e == d else 0) for e in range(3)) + (1,)), (0, 0, 0))
        b.append(m)
    r = rng.standard_normal(tuple(n) + (1,))

    def solve():
        rhs = lib.MultiFab(lay, lib.CELL, 1, 0); rhs.set_from_global(r, (0, 0, 0))
        phi = lib.MultiFab(lay, lib.CELL, 1, 1); phi.setval(0.0)
        st = lib.abec_solve(g, 0.0, 1.0, None, b, phi, rhs, lobc=bc, hibc=bc, rtol=1e-10, atol=1e-16)
        assert st.converged >= 1
        return st.iters, [phi.gather_valid(n)]
    on_and_off(lib, "GSRB_WALLS_INKERNEL", solve)
