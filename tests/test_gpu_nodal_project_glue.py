"""GPU: the passes around the nodal solve of the level projection behind their run-time switches -- the divergence kernel
(IAMRX_NODAL_DIVU_ZM), the velocity scaling folded into nodal_mknewu (IAMRX_PROJ_SCALE_FUSED), the solve on the caller's right-hand side
(IAMRX_NODAL_RHS_INPLACE), the zero fills of the solver's work arrays (IAMRX_NODAL_SKIP_FILLS) and the tiled restriction
(IAMRX_NODAL_RESTRICT_TILE, from 16 coarse cells in x here so that these small levels take it): three NavierStokes steps with all of them
on against all of them off give the same S_new, P_new and Gp_new, ghost cells included, and the same iteration counts -- also when the
device allocator hands out blocks filled with NaNs (IAMRX_POISON_ALLOC = 1) or zeros (2).

TaylorGreen (periodic) and a lid-driven cavity (walls) at 32^3, and at 64 x 48 x 48: the smallest boxes the register-resident smoother
takes, hence the smallest on which the fills are skipped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = {"NODAL_DIVU_ZM": (0, 1), "PROJ_SCALE_FUSED": (0, 1), "NODAL_RHS_INPLACE": (0, 1), "NODAL_SKIP_FILLS": (0, 1),
            "NODAL_RESTRICT_TILE": (0, 1), "NODAL_RESTRICT_MIN": (48, 16)}
LID = [0.0] * 9
LID[2 * 3 + 0] = 1.0
_REF = {}


def _run(lib, flow, n, on, poison):
    from iamr_amd import ns as N
    for key, (off_v, on_v) in SWITCHES.items():
        lib.tuning_set(key, on_v if on else off_v)
    lib.tuning_set("POISON_ALLOC", poison)
    try:
        lay = lib.Layout.single(n)
        if flow == "taylorgreen":
            ns = N.NavierStokes(lib.Geom.make(n), lay, N.ns_params(cfl=0.5, visc_coef=0.01, init_iter=2))
            ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
        else:
            g = lib.Geom.make(n, periodic=(0, 0, 0))
            ns = N.NavierStokes(g, lay, N.ns_params(phys_lo=[4, 4, 5], phys_hi=[5, 5, 5], wall_vel_hi=LID, cfl=0.3, visc_coef=0.01, init_dt=0.0140625,
                                                    init_shrink=0.3, init_iter=2, tracer_diff_coef=0.001))
            ns.init_rest(1.0)
        ns.post_init(-1.0)
        iters = []
        for _ in range(3):
            ns.step()
            iters.append(tuple(s.iters for s in ns.stats()))
        arrays = [ns.data(w).to_numpy(0)[0].copy() for w in (N.NavierStokes.S_NEW, N.NavierStokes.P_NEW, N.NavierStokes.GP_NEW)]
    finally:
        lib.tuning_set("POISON_ALLOC", 0)
        for key, (off_v, on_v) in SWITCHES.items():
            lib.tuning_set(key, off_v if key == "NODAL_RESTRICT_MIN" else on_v)        # the library's defaults
    return arrays, iters


def _reference(lib, flow, n):
    """all switches off, plain allocator: computed once per case"""
    if (flow, n) not in _REF:
        _REF[(flow, n)] = _run(lib, flow, n, False, 0)
    return _REF[(flow, n)]


CASES = [("taylorgreen", (32, 32, 32)), ("cavity", (32, 32, 32)), ("taylorgreen", (64, 48, 48)), ("cavity", (64, 48, 48))]


@pytest.mark.parametrize("flow,n", CASES, ids=[f"{f}-{n[0]}x{n[1]}x{n[2]}" for f, n in CASES])
@pytest.mark.parametrize("poison", [0, 1, 2])
def test_steps_with_all_switches_on_equal_all_off(gpu, flow, n, poison):
    ref, ref_iters = _reference(gpu, flow, n)
    valid = (slice(1, -1),) * 3
    assert all(np.isfinite(a[valid]).all() for a in ref) and np.abs(ref[0][valid][..., 0]).max() > 0.05
    new, new_iters = _run(gpu, flow, n, True, poison)
    assert new_iters == ref_iters
    if poison == 0:
        for a, b in zip(new, ref):
            assert np.array_equal(a, b)
        return
    # a poisoned allocator shows in ghost cells nobody writes, with the old forms as with the new ones: the valid regions equal the plain
    # run's, the whole arrays those of the old forms under the same allocator
    old, old_iters = _run(gpu, flow, n, False, poison)
    assert old_iters == ref_iters
    for a, b, c in zip(new, ref, old):
        assert np.array_equal(a[valid], b[valid])
        assert np.array_equal(a, c, equal_nan=True)
