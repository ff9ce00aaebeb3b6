"""GPU: the turbulent forcing of forced homogeneous isotropic turbulence (reference Tutorials/HIT).
1. the kernel alone (iamrx_turb_force) against the long-double yardstick tests/turb_numpy.py (pinned by tests/test_cpu_turb.py);
2. equivalence with gravity: a one-mode table that is the uniform acceleration (0, 0, g) against the oracle-tested gravity path, on one
   level and on a two-level hierarchy (sub-cycling, mac_sync_compute);
3. the time level of the velocity update;
4. the driver on the tutorial's inputs file: runs, differs from the unforced run, restarts to the bit, off means off.

Bound of 1: max |gpu - longdouble| <= 16 * 2^-53 * S, S = sum over the modes of 2 * 2 pi * max_d(k_d / L_d) * max(|FAX|, |FAY|, |FAZ|)
(turb_numpy.scale).  The fp64 numpy restatement of the direct sum sits at 0.52 and 0.75 of 2^-53 S on the first and fourth shape; the
factor 16 covers device sin / cos at <= 2 ulp against <= 1, the rounding of arguments up to 20 pi and the different order of the sum (the
kernel multiplies per-axis factors, tests/turb_numpy.py sums whole terms)."""
import os
import numpy as np
import pytest

import turb_numpy as tn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORCED = os.path.join(HERE, "golden", "inputs.3d.forced")
CUBE = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
LONG = ((0.0, 0.0, 0.0), (1.0, 1.0, 2.0))
EPS = 2.0 ** -53

# name: (domain box, cells of the level, boxes, ghost layers, nmodes)
SHAPES = {
    "cube_16": (CUBE, (16, 16, 16), [((0, 0, 0), (15, 15, 15))], 1, 4),
    "partial_tiles_20x12x10": (CUBE, (20, 12, 10), [((0, 0, 0), (19, 11, 9))], 1, 4),
    "cube_8_boxes": (CUBE, (16, 16, 16), [((i, j, k), (i + 7, j + 7, k + 7)) for k in (0, 8) for j in (0, 8) for i in (0, 8)], 1, 4),
    "long_12x20x24": (LONG, (12, 20, 24), [((0, 0, 0), (11, 19, 23))], 1, 2),              # zstep = 2: the second mode loop
    "refined_box": (CUBE, (32, 32, 32), [((8, 8, 16), (23, 23, 31))], 3, 4),               # dx / 2, a box away from the origin
}
_REF = {}


def _reference(shape, div_free, t):
    """long-double field on the bounding box of the level's boxes + ghost cells, computed once per (shape, form, time)"""
    key = (shape, div_free, t)
    if key not in _REF:
        box, n, boxes, ng, nmodes = SHAPES[shape]
        k, d = tn.modes(box[0], box[1], nmodes, 0, div_free)
        lo = tuple(min(b[0][q] for b in boxes) - ng for q in range(3))
        hi = tuple(max(b[1][q] for b in boxes) + ng for q in range(3))
        x, y, z = tn.centres(box[0], box[1], n, lo, hi, dtype=np.longdouble)
        _REF[key] = (k, d, lo, tn.field(k, d, div_free, box[0], box[1], x, y, z, t, dtype=np.longdouble), tn.scale(k, d, box[0], box[1]))
    return _REF[key]


def _kernel(lib, shape, div_free, t, k, d, boxes=None):
    box, n, bxs, ng, _ = SHAPES[shape]
    g = lib.Geom.make(n, prob_lo=box[0], prob_hi=box[1])
    lay = lib.Layout(boxes if boxes is not None else bxs)
    out = lib.MultiFab(lay, lib.CELL, 4, ng)
    out.setval(np.nan)
    lib.turb_force(g, k, d, div_free, t, out, ocomp=1)
    return [out.to_numpy(li) for li in range(out.nlocal())]


@pytest.mark.parametrize("t", [0.0, 0.37])
@pytest.mark.parametrize("div_free", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_long_double(gpu, shape, div_free, t):
    k, d, glo, ref, S = _reference(shape, div_free, t)
    worst = 0.0
    for a, lo in _kernel(gpu, shape, div_free, t, k, d):
        assert np.isnan(a[..., 0]).all()                         # the component in front of ocomp is not touched
        f = a[..., 1:4]
        assert np.isfinite(f).all()                              # cells and every ghost cell are written
        sl = tuple(slice(lo[q] - glo[q], lo[q] - glo[q] + f.shape[q]) for q in range(3))
        worst = max(worst, float(np.abs(f.astype(np.longdouble) - ref[sl]).max()))
    print(f"{shape} div_free={div_free} t={t}: max |gpu - longdouble| = {worst:.3e} = {worst / (EPS * S):.3f} x 2^-53 S (S = {S:.4g})")
    assert worst <= 16.0 * EPS * S


@pytest.mark.parametrize("div_free", [1, 0])
def test_boxes_do_not_change_the_field(gpu, div_free):
    """the position comes from the domain's index origin: eight boxes of 8^3 give the bits of the one box of 16^3"""
    k, d, _, _, _ = _reference("cube_16", div_free, 0.37)
    (one, lo1), = _kernel(gpu, "cube_16", div_free, 0.37, k, d)
    for a, lo in _kernel(gpu, "cube_8_boxes", div_free, 0.37, k, d):
        sl = tuple(slice(lo[q] - lo1[q], lo[q] - lo1[q] + a.shape[q]) for q in range(3))
        assert np.array_equal(a[..., 1:4], one[sl + (slice(1, 4),)])


# ---- 2. equivalence with gravity --------------------------------------------------------------------------------------------------------
G = -2.0
TG = os.path.join(HERE, "golden", "inputs.3d.taylorgreen")
TG_AMR = os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")
TG_OVER = ["amr.n_cell=16 16 16", "ns.vel_visc_coef=0.01", "prob.density_ic=2.0", "stop_time=-1", "amr.derive_plot_vars=NONE"]


def _level_run(lib, mode, nsteps=3):
    """mode: 'none', 'gravity' (ns.gravity = G) or 'table' (gravity 0, the one-mode table of the same acceleration)"""
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([TG], TG_OVER + (["ns.gravity=%r" % G] if mode == "gravity" else [])).problem()
    if mode == "table":
        pr["params"]["turb_forcing"] = 1
    ns, lay, g, pr = R.build(None, lib, N, pr=pr)
    if mode == "table":
        ns.set_turb_modes(*tn.gravity_mode(G), div_free=0)
    ns.post_init(-1.0)
    dts = [ns.step() for _ in range(nsteps)]
    return ns.data(N.NavierStokes.S_NEW).gather_valid((16,) * 3), dts


def test_one_mode_table_equals_gravity(gpu):
    S0, dt0 = _level_run(gpu, "none")
    Sg, dtg = _level_run(gpu, "gravity")
    St, dtt = _level_run(gpu, "table")
    assert np.isfinite(St).all()
    dS, ddt = float(np.abs(St - Sg).max()), float(np.abs(np.array(dtt) - np.array(dtg)).max())
    print("one level: table - gravity: state", dS, "dt", ddt, "; gravity - unforced:", float(np.abs(Sg - S0).max()))
    assert dS <= 1e-9 and ddt <= 1e-9                          # velocity, density, tracer and the dt of every step
    assert np.abs(Sg[..., 0:3] - S0[..., 0:3]).max() > 1e-3 and np.abs(St[..., 0:3] - S0[..., 0:3]).max() > 1e-3


def _amr_run(lib, mode, nsteps=2):
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([TG_AMR], ["ns.vel_visc_coef=0.01", "prob.density_ic=2.0", "amr.max_level=1"] + (["ns.gravity=%r" % G] if mode == "gravity" else [])).problem()
    if mode == "table":
        pr["params"]["turb_forcing"] = 1
    amr, lays, g0 = R.build_amr(pr, lib, N)
    assert amr.nlev == 2
    if mode == "table":
        amr.set_turb_modes(*tn.gravity_mode(G), div_free=0)
    amr.post_init(-1.0)
    dts = [amr.coarse_step() for _ in range(nsteps)]
    fmask = np.zeros((32, 32, 32), dtype=bool)
    for lo, hi in pr["fine_boxes"][0]:
        fmask[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    Sc = amr.levels[0].data(N.NavierStokes.S_NEW).gather_valid((16,) * 3)
    Sf = amr.levels[1].data(N.NavierStokes.S_NEW).gather_valid((32,) * 3)[fmask]
    return Sc, Sf, dts


def test_one_mode_table_equals_gravity_two_levels(gpu):
    """fixed two-level grids of inputs.3d.taylorgreen_amr16: sub-cycled fine steps at their own times and the hierarchy's mac_sync_compute"""
    c0, f0, _ = _amr_run(gpu, "none")
    cg, fg, dtg = _amr_run(gpu, "gravity")
    ct, ft, dtt = _amr_run(gpu, "table")
    assert np.isfinite(ct).all() and np.isfinite(ft).all()
    dc, df, ddt = float(np.abs(ct - cg).max()), float(np.abs(ft - fg).max()), float(np.abs(np.array(dtt) - np.array(dtg)).max())
    print("two levels: table - gravity: coarse", dc, "fine", df, "dt", ddt, "; gravity - unforced:", float(np.abs(cg - c0).max()))
    assert dc <= 1e-9 and df <= 1e-9 and ddt <= 1e-9
    assert np.abs(cg[..., 0:3] - c0[..., 0:3]).max() > 1e-3 and np.abs(ct[..., 0:3] - c0[..., 0:3]).max() > 1e-3


# ---- 3. the time level of the velocity update -------------------------------------------------------------------------------------------
def test_velocity_update_uses_the_half_time(gpu):
    """fluid at rest, rho = 2, one mode (0, 0, g cos(omega t)): w = sum_n dt g cos(omega (t_n + dt / 2)), u = v = 0"""
    lib = gpu
    from iamr_amd import ns as N
    g_, omega, dt, nsteps = 1.5, 7.0, 0.01, 4
    geom = lib.Geom.make((16, 16, 16))
    lay = lib.Layout.single((16, 16, 16))
    ns = N.NavierStokes(geom, lay, N.ns_params(fixed_dt=dt, turb_forcing=1))
    ns.set_turb_modes(*tn.gravity_mode(g_, omega), div_free=0)
    ns.init_rest(2.0)
    ns.post_init(-1.0)
    for _ in range(nsteps):
        assert ns.step() == dt
    S = ns.data(N.NavierStokes.S_NEW).gather_valid((16,) * 3)
    w = sum(dt * g_ * np.cos(omega * (n * dt + 0.5 * dt)) for n in range(nsteps))
    print("w", float(S[..., 2].mean()), "expected", w, "max deviation", float(np.abs(S[..., 2] - w).max()), "u, v", float(np.abs(S[..., 0:2]).max()))
    assert np.abs(S[..., 2] - w).max() <= 1e-12
    assert np.abs(S[..., 0:2]).max() == 0.0
    assert np.all(S[..., 3] == 2.0)


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------------
RUN_OVER = ["amr.n_cell=16 16 16", "max_step=4", "amr.plot_int=-1", "amr.check_int=-1", "amr.derive_plot_vars=NONE"]


def _same_plotfiles(a, b):
    from iamr_amd.plotfile import PlotFile
    A, B = PlotFile.read(a), PlotFile.read(b)
    assert len(A.levels) == len(B.levels) and A.time == B.time
    for la, lb in zip(A.levels, B.levels):
        assert la.boxes == lb.boxes and la.step == lb.step
        for x, y in zip(la.data, lb.data):
            assert np.array_equal(x, y), float(np.abs(x - y).max())


def _steps_from(lib, pr, nsteps=4):
    from iamr_amd import ns as N
    from iamr_amd import run as R
    ns, lay, g, pr = R.build(None, lib, N, pr=pr)
    ns.post_init(pr["stop_time"])
    for _ in range(nsteps):
        ns.step()
    return ns.data(N.NavierStokes.S_NEW).gather_valid((16,) * 3), ns.sum_integrated()[2]


def test_driver_runs_the_tutorial_inputs(gpu, tmp_path, capsys):
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    seen = {}

    def observe(ns, step, dt):
        seen[step] = ns.sum_integrated()[2]
    plt, chk = str(tmp_path / "plt"), str(tmp_path / "chk")
    args = [FORCED] + RUN_OVER
    assert R.main(args + ["amr.plot_int=4", f"amr.plot_file={plt}", "amr.check_int=2", f"amr.check_file={chk}"], observe=observe) == 0
    out = capsys.readouterr().out
    assert len([l for l in out.splitlines() if l.startswith("STEP =")]) == 4 and sorted(seen) == [0, 1, 2, 3, 4]
    assert all(np.isfinite(v) and v > 0.0 for v in seen.values())
    # forcing off on the parsed problem: another kinetic energy after the same four steps
    pr = Inputs([FORCED], RUN_OVER).problem()
    pr["params"]["turb_forcing"] = 0
    S_off, ke_off = _steps_from(gpu, pr)
    print("kinetic energy after 4 steps: forced", seen[4], "unforced", ke_off)
    assert abs(seen[4] - ke_off) > 1e-6 * ke_off
    # checkpoint at step 2, restart, two more steps: the uninterrupted run to the bit
    plt2 = str(tmp_path / "rst")
    assert R.main(args + ["amr.plot_int=4", f"amr.plot_file={plt2}", f"amr.restart={chk}00002"]) == 0
    out = capsys.readouterr().out
    assert "RESTART from" in out and len([l for l in out.splitlines() if l.startswith("STEP =")]) == 2
    _same_plotfiles(plt + "00004", plt2 + "00004")
    # turb_forcing = 0 with the other turb_* fields set: the bits of a run that never heard of them
    pr2 = Inputs([FORCED], RUN_OVER).problem()
    pr2["params"].update(turb_forcing=0, turb_nmodes=3, turb_mode_start=1, turb_div_free=0)
    S_set, _ = _steps_from(gpu, pr2)
    pr3 = Inputs([FORCED], RUN_OVER).problem()
    for key in ("turb_forcing", "turb_nmodes", "turb_mode_start", "turb_div_free"):
        del pr3["params"][key]
    S_none, _ = _steps_from(gpu, pr3)
    assert np.array_equal(S_set, S_none) and np.array_equal(S_off, S_none)
