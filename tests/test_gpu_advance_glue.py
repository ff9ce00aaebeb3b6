"""The passes of NavierStokes::advance around the Godunov kernels (IAMRX_ADVANCE_GLUE).  With the switch on, the level
step drops passes whose result it has already (the velocity forcing of the prediction is kept for the advection, the prediction floors
the velocity while it copies it, one pass does the density, tracer and velocity updates and hands rho u*, the right-hand side and its
norms to the viscous solve, arrays of zeros and a fill that is overwritten are gone).  Every expression is the one it replaces
(navierstokes.hip is built with -ffp-contract=off), so the step is the same step bit for bit: two steps after post_init -- the initial
iterations and regular steps -- give the same bytes in the new state, both pressures, Gp, u_mac and aofs, the same dt and the same
iteration counts with the switch off and on.  The counters say which of the items ran, so that no case passes by falling back."""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# predict_velocity on the valid cells; the forcing formed once; no array of zeros for the scalars' viscous terms; no 1e40 fill of the
# viscous terms; the operator of the viscous terms applied to the state in place (no copy of the velocity); the one update pass; that pass
# also forming the viscous right-hand side
COUNTERS = ("ADVANCE_GLUE_PRED_VALID", "ADVANCE_GLUE_FORCE_ONCE", "ADVANCE_GLUE_NO_SVISC", "ADVANCE_GLUE_NO_FILL", "ADVANCE_GLUE_VISC_IN_PLACE",
            "ADVANCE_GLUE_UPDATE", "ADVANCE_GLUE_RHS")
N = 32


def with_keys(lib, keys, fn):
    old = {k: lib.tuning_get(k, 1 if k != "POISON_ALLOC" else 0) for k in keys}
    try:
        for k, v in keys.items():
            lib.tuning_set(k, v)
        return fn()
    finally:
        for k, v in old.items():
            lib.tuning_set(k, v)


def counters(lib):
    return [lib.tuning_get(k, 0) for k in COUNTERS]


def valid_bytes(m, ng):
    """the valid region of every local fab, as bytes (a NaN is equal to the same NaN)"""
    out = []
    for li in range(m.nlocal()):
        a = m.to_numpy(li)[0]
        if ng:
            a = a[ng:-ng, ng:-ng, ng:-ng]
        out.append(np.ascontiguousarray(a).view(np.uint64).copy())
    return out


def level_record(ns):
    T = type(ns)
    rec = {}
    for name, which in (("S_new", T.S_NEW), ("P_new", T.P_NEW), ("P_old", T.P_OLD), ("Gp_new", T.GP_NEW), ("Gp_old", T.GP_OLD),
                        ("umac_x", T.UMAC_X), ("umac_y", T.UMAC_Y), ("umac_z", T.UMAC_Z), ("aofs", T.AOFS)):
        rec[name] = valid_bytes(ns.data(which), T._types[which][2])
    return rec


def run_level(lib, make, steps=2):
    """make() -> (level, stop_time); post_init, then `steps` steps"""
    c0 = counters(lib)
    ns, stop = make()
    ns.post_init(stop)
    dts = [ns.step() for _ in range(steps)]
    lib.sync()
    moved = [int(b - a) for a, b in zip(c0, counters(lib))]
    rec = level_record(ns)
    rec["dt"] = dts
    rec["iters"] = [(s.iters, s.converged) for s in ns.stats()]
    return rec, moved


def same_record(on, off):
    assert on["dt"] == off["dt"], (on["dt"], off["dt"])
    assert on["iters"] == off["iters"], (on["iters"], off["iters"])
    for name in off:
        if name in ("dt", "iters"):
            continue
        assert len(on[name]) == len(off[name])
        for a, b in zip(on[name], off[name]):
            assert np.array_equal(a, b), (name, int((a != b).sum()))
    sn = np.concatenate([a.view(np.float64).ravel() for a in on["S_new"]])
    assert np.isfinite(sn).all() and np.abs(sn).max() > 0.0


def check_items(moved, want):
    """want[k]: True -- the item ran; False -- it did not"""
    for k, w in zip(COUNTERS, want):
        c = moved[COUNTERS.index(k)]
        assert (c > 0) == w, (k, c, dict(zip(COUNTERS, moved)))


def taylorgreen(lib, layout, **par):
    from iamr_amd import ns as NS

    def make():
        g = lib.Geom.make((N, N, N))
        lay = layout()
        p = dict(cfl=0.7, visc_coef=1e-3, init_iter=2, init_shrink=1.0)
        p.update(par)
        ns = NS.NavierStokes(g, lay, NS.ns_params(**p), lib.mg_opts())
        ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
        return ns, -1.0
    return make


def on_and_off(lib, make, keys=None, steps=2):
    keys = keys or {}
    off, moved_off = with_keys(lib, dict(keys, ADVANCE_GLUE=0), lambda: run_level(lib, make, steps))
    on, moved_on = with_keys(lib, dict(keys, ADVANCE_GLUE=1), lambda: run_level(lib, make, steps))
    assert moved_off == [0] * len(COUNTERS), moved_off
    same_record(on, off)
    return moved_on


#            pred  force nosvisc nofill inplace update rhs
ALL_ITEMS = (True, True, True, True, True, True, True)
PERIODIC_CASES = {
    # the flagship in miniature: 32 = two full 14-cell tiles and a partial one
    "one box": (dict(), ALL_ITEMS),
    # the momentum form: the advection's forcing is not the prediction's (no division by rho); the update pass takes its momentum branch
    "do_mom_diff, conservative tracer": (dict(do_mom_diff=1, do_cons_trac=1), (True, False, True, True, True, True, True)),
    # a diffusive tracer: its viscous terms exist, and its solve runs between the update pass and the viscous solve
    "diffusive tracer": (dict(tracer_diff_coef=1e-3), (True, True, False, True, True, True, True)),
    # temperature: divu, and calc_divu / calc_dsdt now behind the velocity update
    "do_temp": (dict(do_temp=1, temp_cond_coef=1e-3), (True, True, False, True, True, True, True)),
    # the 27-point clips sit between the update passes: those stay separate, and with them the first pass of the viscous solve
    "do_denminmax, do_scalminmax": (dict(do_denminmax=1, do_scalminmax=1), (True, True, True, True, True, False, False)),
    # fully implicit: no explicit viscous terms at all (none computed: no fill to drop), no cached terms for the right-hand side
    "be_cn_theta = 1": (dict(be_cn_theta=1.0), (True, True, True, False, False, True, False)),
}


@pytest.mark.parametrize("case", list(PERIODIC_CASES))
def test_periodic_step_is_the_same_step(gpu, case):
    lib = gpu
    par, want = PERIODIC_CASES[case]
    moved = on_and_off(lib, taylorgreen(lib, lambda: lib.Layout.single((N, N, N)), **par))
    check_items(moved, want)
    if case == "one box":
        # four advances: two initial iterations (the first of them skips the viscous solve), two steps
        assert dict(zip(COUNTERS, moved)) == dict(zip(COUNTERS, (4, 4, 4, 4, 4, 4, 3))), moved


def test_eight_boxes(gpu):
    """the same on eight boxes of 16^3: merged into one by the level, or kept (the suite's two box modes)"""
    lib = gpu
    moved = on_and_off(lib, taylorgreen(lib, lambda: lib.Layout.decompose((N, N, N), 16)))
    check_items(moved, ALL_ITEMS)


def test_nothing_reads_a_dropped_fill(gpu):
    """IAMRX_POISON_ALLOC = 1: every array starts as NaN, so a value that one of the dropped fills used to provide would show"""
    lib = gpu
    moved = on_and_off(lib, taylorgreen(lib, lambda: lib.Layout.single((N, N, N))), keys={"POISON_ALLOC": 1})
    check_items(moved, ALL_ITEMS)


def test_lid_driven_cavity(gpu):
    """walls on every side: the prediction keeps FillPatch and the pass over the grown boxes (the boundary functor puts other values
    in the ghost cells) and the tracer is diffusive (ns.scal_diff_coefs = 0.001: its viscous terms exist); everything else runs, the
    ghost layer of rho_ctime taking its boundary fill"""
    lib = gpu
    from iamr_amd import ns as NS, run as R
    from iamr_amd.inputs import Inputs

    def make():
        inp = Inputs([os.path.join(GOLDEN, "regtest.3d.lid_driven_cavity")],
                     [f"amr.n_cell={N} {N} {N}", f"amr.max_grid_size={N}", "max_step=3", f"ns.init_dt={0.0140625 * 64 / N}"])
        pr = inp.problem()
        ns, lay, g, pr = R.build(inp, lib, NS, 1, pr)
        return ns, pr["stop_time"]

    moved = on_and_off(lib, make)
    check_items(moved, (False, True, False, True, True, True, True))


def test_two_levels(gpu):
    """a 16^3 base box and a 16^3 refined box over its centre (the layout of bench.amr_workload), one coarse step: the refined level
    keeps FillPatch everywhere (the coarse interpolant) and its 1e40 fill; both levels form viscous fluxes for the registers, so the
    viscous solve forms its own right-hand side"""
    lib = gpu
    from iamr_amd import ns as NS
    from iamr_amd.amr import Amr
    n0 = 16

    def run():
        c0 = counters(lib)
        g0 = lib.Geom.make((n0,) * 3)
        lays = [lib.Layout([((0,) * 3, (n0 - 1,) * 3)]), lib.Layout([((n0 // 2,) * 3, (n0 // 2 + n0 - 1,) * 3)])]
        amr = Amr(g0, lays, NS.ns_params(cfl=0.7, visc_coef=1e-3, init_iter=2, init_shrink=1.0), lib.mg_opts())
        for l in range(2):
            amr.levels[l].init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
        amr.post_init()
        amr.coarse_step()
        lib.sync()
        moved = [int(b - a) for a, b in zip(c0, counters(lib))]
        rec = {"dt": list(amr.dts()), "iters": []}
        for l in range(2):
            for k, v in level_record(amr.levels[l]).items():
                rec[f"{k}[{l}]"] = v
            rec["iters"] += [(s.iters, s.converged) for s in amr.levels[l].stats()]
        rec["S_new"] = rec["S_new[0]"] + rec["S_new[1]"]
        return rec, moved

    off, moved_off = with_keys(lib, {"ADVANCE_GLUE": 0}, run)
    on, moved_on = with_keys(lib, {"ADVANCE_GLUE": 1}, run)
    assert moved_off == [0] * len(COUNTERS), moved_off
    same_record(on, off)
    check_items(moved_on, (True, True, True, True, True, True, False))
