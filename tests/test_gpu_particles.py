"""GPU: tracer particles (iamr_amd/csrc/k_particles.hip) against the numpy yardstick tests/particles_numpy.py and closed-form trajectories.
1. the advect kernel on a periodic two-box level and on a box with two wall faces;
2. redistribution over two levels, the two particle counts, removal beyond a wall, the error status;
3. a uniform flow on a two-level hierarchy with sub-cycling (and with a regrid that moves the patch): x0 + U t;
4. the driver on the reference's two-dimensional particle regression inputs: run, plotfile, checkpoint, restart to the bit;
5. nothing attached: nothing changes.

The container's arithmetic belongs to AMReX, which is not in the reference tree: nothing here is pinned against it (DESIGN.md section 7
row f8).

Bound of 1, per coordinate: 2^-53 (16 max|x| + 128 dt max|u|) -- roughly 15 roundings per pass (FMA included) and the pass-1 error carried
through pass 2, for fields with dt sum_e max|Delta_e u| / dx_e <= 1 (asserted on the input).
Bound of 3: t max|u_mac - U| + 64 2^-53 max|x|, the deviation read from the levels' own u_mac snapshots."""
import os
import numpy as np
import pytest

import particles_numpy as pn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
EPS = 2.0 ** -53

N0 = (16, 12, 8)
PLO, PHI = (0.0, 0.0, 0.0), (2.0, 1.5, 1.0)
DX0 = tuple((PHI[e] - PLO[e]) / N0[e] for e in range(3))
BOXES0 = [((0, 0, 0), (7, 11, 7)), ((8, 0, 0), (15, 11, 7))]


def _smooth_umac(rng, n, per):
    """three face arrays over indices -1 .. n + type (one ghost layer): a few random Fourier modes, periodic images exact in the
    periodic directions"""
    out = []
    for d in range(3):
        idx = [np.arange(-1, n[e] + (1 if e == d else 0) + 1) for e in range(3)]
        ph = []
        for e in range(3):
            pos = idx[e] + (0.0 if e == d else 0.5)
            if per[e]:
                pos = np.mod(pos, n[e])
            ph.append(2.0 * np.pi * pos / n[e])
        X, Y, Z = np.meshgrid(*ph, indexing="ij")
        f = np.zeros(X.shape)
        for _ in range(4):
            k = rng.integers(0, 3, size=3)
            a, p0 = rng.uniform(-0.4, 0.4), rng.uniform(0, 2 * np.pi)
            f += a * np.cos(k[0] * X + k[1] * Y + k[2] * Z + p0)
        out.append(f + rng.uniform(-0.3, 0.3))
    return out


def _edge_positions(rng, n_random, faces):
    """random positions in the domain plus positions within 1e-12 of the given planes (direction, coordinate)"""
    x = rng.uniform(0.0, 1.0, size=(n_random, 3)) * (np.array(PHI) - np.array(PLO)) + np.array(PLO)
    extra = []
    for e, c in faces:
        for s in (-1e-12, 1e-12, -3e-13, 0.0):
            q = rng.uniform(0.0, 1.0, size=(6, 3)) * (np.array(PHI) - np.array(PLO)) + np.array(PLO)
            q[:, e] = c + s
            extra.append(q)
    return np.concatenate([x] + extra)


def _advect_case(lib, per, boxes, x0, wall_junk):
    from iamr_amd.particles import Particles
    rng = np.random.default_rng(7)
    g = lib.Geom.make(N0, PLO, PHI, per)
    lay = lib.Layout(boxes)
    U = _smooth_umac(rng, N0, per)
    if wall_junk:                                   # ghost faces beyond a wall: never to be read (the stencil is clamped to the domain)
        for d in range(3):
            for e in range(3):
                if not per[e]:
                    sl = [slice(None)] * 3
                    sl[e] = 0
                    U[d][tuple(sl)] = 1.0e30
                    sl[e] = -1
                    U[d][tuple(sl)] = 1.0e30
    um = [lib.MultiFab(lay, lib.face(d), 1, 1) for d in range(3)]
    for d in range(3):
        um[d].set_from_global(U[d][..., None], (-1, -1, -1))
    dt = 0.05
    umax = max(np.abs(U[d][1:-1, 1:-1, 1:-1]).max() for d in range(3))
    grad = sum(max(np.abs(np.diff(U[d][1:-1, 1:-1, 1:-1], axis=e)).max() for d in range(3)) / DX0[e] for e in range(3))
    assert dt * grad <= 1.0                         # the condition the bound is derived for
    assert dt * umax / min(DX0) < 0.5
    pc = Particles([g], [lay], 1)
    ids = np.arange(1, len(x0) + 1, dtype=np.int32)
    ids[5] = 0                                      # an invalid particle: dropped by the placement
    pc.add(x0, ids=ids)
    before = pc.read()
    assert pc.count() == len(x0) - 1
    pc.advect(0, um, dt)
    after = pc.read()
    assert np.array_equal(before["id"], after["id"]) and np.array_equal(before["box"], after["box"])
    tol = EPS * (16.0 * np.abs(before["xyz"]).max() + 128.0 * dt * umax)
    worst = 0.0
    for b in range(len(boxes)):
        sel = before["box"] == b
        assert sel.any()
        fabs, los = zip(*[um[d].to_numpy(b) for d in range(3)])
        xn, rn, _ = pn.advect(before["xyz"][sel], before["id"][sel], [f[..., 0] for f in fabs], los, dt, PLO, DX0, (0, 0, 0), tuple(n - 1 for n in N0), per)
        worst = max(worst, np.abs(after["xyz"][sel] - xn).max(), np.abs(after["r"][sel] - rn).max())
    print(f"advect per={per}: worst |gpu - numpy| = {worst:.3e}, bound {tol:.3e}, moved {np.abs(after['xyz'] - before['xyz']).max():.3e}")
    assert worst <= tol
    assert np.abs(after["xyz"] - before["xyz"]).max() > 1e-3


def test_advect_periodic_two_boxes(gpu):
    rng = np.random.default_rng(1)
    x0 = _edge_positions(rng, 1900, [(0, 1.0), (0, 2.0), (0, 0.0), (1, 0.375), (2, 0.5), (1, 1.5), (2, 0.0), (0, 0.125 * 5)])
    _advect_case(gpu, (1, 1, 1), BOXES0, x0, False)


def test_advect_walls_clamp(gpu):
    rng = np.random.default_rng(2)
    x0 = _edge_positions(rng, 1800, [(1, 0.375), (2, 0.5)])
    last = rng.uniform(0.0, 1.0, size=(200, 3)) * (np.array(PHI) - np.array(PLO))
    last[:100, 0] = rng.uniform(0.0, 0.5 * DX0[0], size=100)                    # inside the last half cell at either wall
    last[100:, 0] = PHI[0] - rng.uniform(1e-9, 0.5 * DX0[0], size=100)
    x0 = np.concatenate([np.clip(x0, [1e-9, 0, 0], [PHI[0] - 1e-9, PHI[1], PHI[2]]), last])
    _advect_case(gpu, (0, 1, 1), [((0, 0, 0), (15, 11, 7))], x0, True)


# ---- redistribution --------------------------------------------------------------------------------------------------------------------
FINE_BOX = ((8, 4, 0), (23, 19, 15))                # 16^3 fine cells = coarse cells (4..11, 2..9, 0..7): across the seam of level 0


def _levels():
    return [dict(n=N0, dlo=(0, 0, 0), dx=DX0, boxes=BOXES0),
            dict(n=tuple(2 * n for n in N0), dlo=(0, 0, 0), dx=tuple(0.5 * d for d in DX0), boxes=[FINE_BOX])]


def _two_level_container(lib):
    from iamr_amd.particles import Particles
    g0 = lib.Geom.make(N0, PLO, PHI, (1, 1, 1))
    g1 = lib.Geom.make(tuple(2 * n for n in N0), PLO, PHI, (1, 1, 1))
    l0, l1 = lib.Layout(BOXES0), lib.Layout([FINE_BOX])
    return Particles([g0, g1], [l0, l1], 2), (g0, g1), (l0, l1)


def _counts(lib, pc, lays, which):
    out = []
    for l, lay in enumerate(lays):
        m = lib.MultiFab(lay, lib.CELL, 1, 0)
        (pc.particle_count if which == 0 else pc.total_particle_count)(l, m)
        n = tuple(N0[e] * 2 ** l for e in range(3))
        out.append(m.gather_valid(n)[..., 0])
    return out


def _check_against_yardstick(lib, pc, lays, before, xnew, lev_min, lev_max, ngrow):
    """set the positions xnew (by id), redistribute, compare levels, boxes, positions and both counts with the yardstick"""
    byid = {int(i): q for q, i in enumerate(before["id"])}
    pc.set_positions(xnew)
    removed = pc.redistribute(lev_min, lev_max, ngrow)
    ex, el, eb, st = pn.redistribute(xnew, before["id"], before["level"], before["box"], _levels(), PLO, PHI, (1, 1, 1), lev_min, lev_max, ngrow)
    assert removed == int((st == 1).sum()) and not (st == 2).any()
    got = pc.read()
    keep = st == 0
    assert pc.count() == int(keep.sum())
    q = np.array([byid[int(i)] for i in got["id"]])
    assert np.array_equal(got["level"], el[q]) and np.array_equal(got["box"], eb[q])
    assert np.array_equal(got["xyz"], ex[q])                                   # the wrap is the same arithmetic: to the bit
    key = got["level"] * 1000 + got["box"]
    assert np.all(np.diff(key) >= 0)                                           # stored grouped by level and box
    for which, fn in ((0, pn.particle_count), (1, pn.total_particle_count)):
        dev = _counts(lib, pc, lays, which)
        for l in range(2):
            ref = fn(got["xyz"], got["level"], got["box"], _levels(), PLO, l)
            if l == 1:                                                         # the device array lives on the patch only
                mask = np.zeros(ref.shape, bool)
                mask[tuple(slice(FINE_BOX[0][e], FINE_BOX[1][e] + 1) for e in range(3))] = True
                assert not ref[~mask].any()
            assert np.array_equal(dev[l], ref), (which, l)
    return got


def test_redistribute_two_levels(gpu):
    lib = gpu
    pc, gs, lays = _two_level_container(lib)
    rng = np.random.default_rng(3)
    dxf = [0.5 * d for d in DX0]
    plo_f = [FINE_BOX[0][e] * dxf[e] for e in range(3)]
    phi_f = [(FINE_BOX[1][e] + 1) * dxf[e] for e in range(3)]
    # start: a: left of the seam, outside the patch in y; b: next to the periodic edges; c: around the patch; d: inside the patch next to its faces
    a = np.stack([rng.uniform(0.9, 0.999, 40), rng.uniform(1.3, 1.45, 40), rng.uniform(0, 1, 40)], 1)
    b = np.stack([rng.uniform(1.9, 1.999, 40), rng.uniform(0.01, 0.1, 40), rng.uniform(0.9, 0.999, 40)], 1)
    c = np.stack([rng.uniform(plo_f[0] - 0.1, plo_f[0] - 0.01, 40), rng.uniform(plo_f[1] + 0.1, phi_f[1] - 0.1, 40), rng.uniform(0, 1, 40)], 1)
    d = np.stack([rng.uniform(plo_f[0] + 0.001, plo_f[0] + dxf[0], 40), rng.uniform(phi_f[1] - dxf[1], phi_f[1] - 0.001, 40), rng.uniform(0, 1, 40)], 1)
    x0 = np.concatenate([a, b, c, d, rng.uniform(0, 1, (60, 3)) * np.array(PHI)])
    pc.add(x0)
    s0 = pc.read()
    assert pc.count() == len(x0) and pc.count(1) >= 40 and pc.count(0) >= 120
    ref0 = pn.redistribute(x0, np.arange(1, len(x0) + 1), np.zeros(len(x0), int), np.zeros(len(x0), int), _levels(), PLO, PHI, (1, 1, 1), 0, 1, 0)
    o = s0["id"] - 1
    assert np.array_equal(s0["level"], ref0[1][o]) and np.array_equal(s0["box"], ref0[2][o])

    def moved(state):
        """by hand: a crosses the seam, b crosses the periodic edges, c enters the patch, d leaves it by one fine cell in -x / +y"""
        x = state["xyz"].copy()
        for q, i in enumerate(state["id"]):
            g = (int(i) - 1) // 40
            if g == 0:
                x[q, 0] += 0.11
            elif g == 1:
                x[q] += (0.12, -0.15, 0.11)
            elif g == 2:
                x[q, 0] += 0.13
            elif g == 3:
                if (int(i) % 2) == 0:
                    x[q, 0] -= dxf[0]
                else:
                    x[q, 1] += dxf[1]
        return x

    # ngrow = 1 from level 1: the leavers stay on level 1 (one cell outside its box); level 0 is left alone
    x1 = moved(s0)
    s1 = _check_against_yardstick(lib, pc, lays, s0, x1, 1, 1, 1)
    grp = (s1["id"] - 1) // 40
    assert np.all(s1["level"][grp == 3] == 1)
    cnt1 = _counts(lib, pc, lays, 0)[1]
    assert cnt1.sum() < (s1["level"] == 1).sum()          # the particles outside the valid cells of level 1 are in no count
    # ngrow = 0 from level 1: they cannot be placed -- an error, and the container stays as it was
    with pytest.raises(lib.IamrxError, match="no box"):
        pc.redistribute(1, 1, 0)
    s1b = pc.read()
    assert all(np.array_equal(s1[k], s1b[k]) for k in s1)
    # ngrow = 0 from level 0: everything goes where it belongs; the leavers drop to level 0
    s2 = _check_against_yardstick(lib, pc, lays, s1, s1["xyz"], 0, 1, 0)
    grp = (s2["id"] - 1) // 40
    assert np.all(s2["level"][grp == 3] == 0) and np.all(s2["level"][grp == 2] == 1)
    assert np.all(s2["box"][grp == 0] == 1)               # across the seam
    assert np.all((s2["xyz"] >= np.array(PLO)) & (s2["xyz"] < np.array(PHI)))
    tot0 = _counts(lib, pc, lays, 1)[0]
    assert tot0.sum() == pc.count() == len(x0)            # every live particle is in exactly one cell of level 0's total count
    assert _counts(lib, pc, lays, 0)[0].sum() + _counts(lib, pc, lays, 0)[1].sum() == len(x0)
    # lev_max = 0: everything on level 0
    s3 = _check_against_yardstick(lib, pc, lays, s2, s2["xyz"], 0, 0, 0)
    assert np.all(s3["level"] == 0)


def test_redistribute_wall_removes_and_counts(gpu):
    from iamr_amd.particles import Particles
    lib = gpu
    g = lib.Geom.make(N0, PLO, PHI, (0, 1, 1))
    pc = Particles([g], [lib.Layout(BOXES0)], 1)
    x = np.array([[0.5, 0.5, 0.5], [1.5, 0.2, 0.3], [-0.01, 0.5, 0.5], [2.0, 0.5, 0.5], [1.99, 1.6, -0.1]])
    assert pc.add(x) == 2 and pc.count() == 3 and pc.removed == 2 and pc.next_id == 6
    s = pc.read_sorted()
    assert list(s["id"]) == [1, 2, 5] and list(s["box"]) == [0, 1, 1]
    assert np.allclose(s["xyz"][2], [1.99, 0.1, 0.9], atol=1e-15)
    moved = pc.read()
    moved["xyz"][:, 0] += 0.6                             # the second and the third leave through the high wall
    pc.set_positions(moved["xyz"])
    assert pc.redistribute() == 2 and pc.count() == 1 and pc.removed == 4
    assert pc.add(np.array([[0.1, 0.1, 0.1]])) == 0 and sorted(pc.read()["id"]) == [1, 6]


# ---- uniform flow on a two-level hierarchy ---------------------------------------------------------------------------------------------
UVEL = (1.0, 0.7, -0.4)                              # oblique to the grid
PATCH_A = ((8, 8, 8), (23, 23, 23))                  # 8^3 coarse cells of the 16^3 level 0, in fine indices
PATCH_B = ((12, 8, 4), (27, 23, 19))                 # the same patch moved by two coarse cells in x and z


def _uniform_hierarchy(lib, patch):
    from iamr_amd import run as R, ns as N
    pr = dict(n=[16, 16, 16], prob_lo=[0.0, 0.0, 0.0], prob_hi=[1.0, 1.0, 1.0], periodic=[1, 1, 1], max_grid_size=16, fine_boxes=[[patch]],
              params=dict(cfl=0.9, visc_coef=0.0), regrid=None, slab=None,
              prob=dict(probtype=4, density_ic=1.0, direction=0, interface_width=1.0, blob_radius=0.2, blob_center=[0.5, 0.5, 0.5],
                        velocity_ic=list(UVEL)))
    amr, lays, g0 = R.build_amr(pr, lib, N)
    amr.post_init(-1.0)
    return amr, N


def _around_patch(patch, rng):
    """positions on both sides of every face of the patch, within one fine cell of it, and a few anywhere"""
    dxf = 1.0 / 32
    lo = np.array(patch[0]) * dxf
    hi = (np.array(patch[1]) + 1) * dxf
    pts = []
    for e in range(3):
        for plane in (lo[e], hi[e]):
            for off in (-0.9, -0.45, -0.05, 0.05, 0.45, 0.9):
                q = lo + rng.uniform(0.02, 0.98, size=(6, 3)) * (hi - lo)
                q[:, e] = plane + off * dxf
                pts.append(q)
    pts.append(rng.uniform(0.0, 1.0, size=(40, 3)))
    return np.concatenate(pts)


def _umac_deviation(amr, N):
    dev = 0.0
    for lev in amr.levels:
        for d in range(3):
            m = lev.data(N.NavierStokes.UMAC_X + d)
            for li in range(m.nlocal()):
                dev = max(dev, float(np.abs(m.to_numpy(li)[0] - UVEL[d]).max()))
    return dev


@pytest.mark.parametrize("regrid", [False, True])
def test_uniform_flow_on_a_subcycled_hierarchy(gpu, regrid):
    from iamr_amd.particles import Particles
    lib = gpu
    amr, N = _uniform_hierarchy(lib, PATCH_A)
    pc = Particles.for_hierarchy(amr)
    amr.set_particles(pc)
    assert amr.particles is pc
    x0 = _around_patch(PATCH_A, np.random.default_rng(11))
    pc.add(x0)
    s = pc.read_sorted()
    assert pc.count() == len(x0) and pc.count(1) > 100 and pc.count(0) > 100
    seen_levels = {int(i): {int(l)} for i, l in zip(s["id"], s["level"])}
    dev, patch = 0.0, PATCH_A
    for step in range(4):
        if regrid and step == 2:
            assert amr.install_grids([[PATCH_B]])
            patch = PATCH_B
            q = pc.read()
            inside = np.all((np.floor(q["xyz"] * 32) >= np.array(patch[0])) & (np.floor(q["xyz"] * 32) <= np.array(patch[1])), axis=1)
            assert np.array_equal(q["level"], inside.astype(np.int32))        # post_regrid: everything on the new boxes at once
        amr.coarse_step()
        dev = max(dev, _umac_deviation(amr, N))
        q = pc.read()
        for i, l in zip(q["id"], q["level"]):
            seen_levels[int(i)].add(int(l))
    t = amr.time
    s = pc.read_sorted()
    assert pc.count() == len(x0) and np.array_equal(s["id"], np.arange(1, len(x0) + 1))
    exact = x0 + np.array(UVEL) * t
    err = np.abs((s["xyz"] - exact + 0.5) % 1.0 - 0.5).max()
    bound = t * dev + 64.0 * EPS * max(1.0, np.abs(exact).max())
    print(f"uniform flow regrid={regrid}: t = {t:.6f}, max |u_mac - U| = {dev:.3e}, worst |x - (x0 + U t)| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    inside = np.all((np.floor(s["xyz"] * 32) >= np.array(patch[0])) & (np.floor(s["xyz"] * 32) <= np.array(patch[1])), axis=1)
    assert np.array_equal(s["level"], inside.astype(np.int32))                # on the finest level that holds it
    assert np.all((s["xyz"] >= 0.0) & (s["xyz"] < 1.0))
    changed = sum(1 for v in seen_levels.values() if len(v) == 2)
    assert changed > 50                                                       # particles did enter and leave the patch
    for l, lev in enumerate(amr.levels):                                      # the hierarchy's derive knows the two names
        tot = lev.derive("total_particle_count").gather_valid([16 * 2 ** l] * 3)
        cnt = lev.derive("particle_count").gather_valid([16 * 2 ** l] * 3)
        assert cnt.sum() == pc.count(l) and (l > 0 or tot.sum() == pc.count())
    amr.set_particles(None)
    with pytest.raises(lib.IamrxError, match="unknown derived quantity"):
        amr.levels[0].derive("particle_count")


def test_nothing_attached_changes_nothing(gpu):
    """two steps of a level: as it is; and with an empty container attached and detached before the first step and attached during the
    second -- the same bits"""
    from iamr_amd import ns as N
    from iamr_amd.particles import Particles
    lib = gpu
    g = lib.Geom.make((16, 16, 16))

    def run(with_container):
        lay = lib.Layout.decompose((16, 16, 16), 16)
        ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7, visc_coef=0.01))
        ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
        ns.post_init(-1.0)
        if with_container:
            pc = Particles.for_level(ns)
            ns.set_particles(pc)
            ns.set_particles(None)
            assert ns.particles is None
        ns.step()
        if with_container:
            ns.set_particles(pc)
        ns.step()
        return [ns.data(w).to_numpy(0)[0] for w in (N.NavierStokes.S_NEW, N.NavierStokes.P_NEW, N.NavierStokes.UMAC_X)]
    a, b = run(False), run(True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_single_level_step_moves_and_redistributes(gpu):
    """a level on its own: step() advects with the level's u_mac and redistributes; the count derives follow"""
    from iamr_amd import ns as N
    from iamr_amd.particles import Particles
    lib = gpu
    g = lib.Geom.make((16, 16, 16))
    lay = lib.Layout.decompose((16, 16, 16), 8)
    ns = N.NavierStokes(g, lay, N.ns_params(cfl=0.7))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init(-1.0)
    pc = Particles.for_level(ns)
    ns.set_particles(pc)
    x0 = np.random.default_rng(5).uniform(0, 1, (500, 3))
    pc.add(x0)
    for _ in range(3):
        ns.step()
    s = pc.read_sorted()
    assert pc.count() == 500 and np.all((s["xyz"] >= 0) & (s["xyz"] < 1))
    moved = np.abs((s["xyz"] - x0 + 0.5) % 1.0 - 0.5).max()
    assert 1e-3 < moved < 3 * 0.7 / 16 + 1e-12                             # at most cfl cells per step
    cnt = ns.derive("particle_count").gather_valid((16, 16, 16))[..., 0]
    ref = np.zeros((16, 16, 16))
    np.add.at(ref, tuple(np.floor(s["xyz"] * 16).astype(int).T), 1.0)
    assert np.array_equal(cnt, ref)
    assert np.array_equal(ns.derive("total_particle_count").gather_valid((16, 16, 16))[..., 0], ref)


# ---- the driver on the reference's two-dimensional particle regression test ---------------------------------------------------------------
def test_front_end_run_checkpoint_restart(gpu, tmp_path, capsys):
    from iamr_amd import run as R
    from iamr_amd.plotfile import PlotFile
    from iamr_amd.particles import read_particles_dir, read_particle_file
    inp = os.path.join(GOLD, "run_2d_particles", "regtest.inputs")
    common = [inp, "amr.n_cell=32 32", "max_step=4", "amr.plot_int=4", "amr.derive_plot_vars=particle_count total_particle_count"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    assert R.main(common + [f"amr.plot_file={a}/plt", f"amr.check_file={a}/chk", "amr.check_int=2"]) == 0
    out = capsys.readouterr().out
    assert len([l for l in out.splitlines() if l.startswith("STEP =")]) == 4 and "LEVELS = 2" in out
    assert "particles.timestamp_dir" in out and "particles.timestamp_indices" in out          # reported as ignored
    mid = 0.25                                                             # the slab: 8 cells of 2 / 32, y in [0, 0.5]
    x0 = read_particle_file(os.path.join(GOLD, "run_2d_particles", "particle_file"), mid)
    end = read_particles_dir(str(a / "plt00004"))                           # particles.particles_in_plotfile = true
    assert os.path.isdir(a / "chk00002" / "Particles") and os.path.isdir(a / "chk00004" / "Particles")
    assert len(end["id"]) == 30 and list(end["id"]) == list(range(1, 31)) and end["next_id"] == 31
    assert np.all(end["xyz"][:, 1] == mid)                                 # the slab coordinate is unchanged
    disp = np.abs(end["xyz"][:, [0, 2]] - np.where(x0 >= 1.0, x0 - 2.0, x0)[:, [0, 2]])
    disp = np.minimum(disp, 2.0 - disp)
    assert 1e-4 < disp.max() < 4 * 2.0 / 32                                # they moved, by less than a cell per step (cfl = 0.9)
    pf = PlotFile.read(str(a / "plt00004"))
    assert pf.names[-2:] == ["particle_count", "total_particle_count"] and len(pf.levels) == 2
    q = pf.names.index("particle_count")
    assert sum(float(d[..., q].sum()) for lv in pf.levels for d in lv.data) == 30.0
    assert sum(float(d[..., q + 1].sum()) for d in pf.levels[0].data) == 30.0
    # restart from step 2: the same particles, to the bit
    assert R.main(common + [f"amr.plot_file={b}/plt", f"amr.check_file={b}/chk", f"amr.restart={a}/chk00002"]) == 0
    capsys.readouterr()
    pf2 = PlotFile.read(str(b / "plt00004"))
    for la, lb in zip(pf.levels, pf2.levels):                              # the flow that carries them continued to the bit ...
        assert la.boxes == lb.boxes and all(np.array_equal(x, y) for x, y in zip(la.data, lb.data))
    again = read_particles_dir(str(b / "plt00004"))
    for k in ("xyz", "r", "id", "cpu"):                                    # ... and so did they
        assert np.array_equal(end[k], again[k]), k
    assert again["next_id"] == 31
