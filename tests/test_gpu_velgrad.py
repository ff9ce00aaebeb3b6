"""GPU: the derived fields of the velocity-gradient tensor (include/iamrx.h: iamrx_derive_velgrad; kernel in iamr_amd/csrc/k_velgrad.hip)
and what is built on them: NavierStokes.derive(list), integrate, the histograms of the new names, the driver's plotfile and integrals.

The yardstick is numpy in this file: `fields` is the table of the definitions, evaluated in float64 in the order the kernel documents.
The tolerance is derived, not tuned: |got - want| <= 32 eps B, where B is the same formula with every gradient entry replaced by its
magnitude bound 0.5 (|a| + |b|) / dx and every subtraction by an addition (`fields(..., bound=True)`); the longest chain, r_invariant,
carries about 11 roundings.  strain_rate is compared as got^2 against 2 SS.  The tile of the marching form is 32 x 8: the shapes are one
tile, one-cell remainders, a single plane, one odd box, unequal boxes off the tile grid, and 4^3 boxes (the plain form)."""
import math
import os
import numpy as np
import pytest
import hist_numpy as HN
from test_gpu_profile import random_state, put_state, one_level
import ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
FORCED = os.path.join(GOLD, "inputs.3d.forced")
DSL2D = os.path.join(GOLD, "inputs.2d.doubleshearlayer_c3")
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]
EPS = 2.0 ** -52
TEN = ["diveru", "vort_x", "vort_y", "vort_z", "enstrophy", "strain_rate", "dissipation", "q_criterion", "r_invariant", "helicity"]
SENTINEL = -7.25e33


# ------------------------------------------------------------------------------------------------------------------ the yardstick
def gradient(G, dx, bound=False):
    """G: (nx + 2, ny + 2, nz + 2, 3) velocity with one ghost layer -> A[n][d] on the interior, 0.5 * (a - b) * (1 / dx_d) left to right;
    bound: the magnitude bound 0.5 * (|a| + |b|) / dx_d"""
    c = (slice(1, -1),) * 3
    A = [[None] * 3 for _ in range(3)]
    for n in range(3):
        for d in range(3):
            hi = tuple(slice(2, None) if q == d else slice(1, -1) for q in range(3)) + (n,)
            lo = tuple(slice(0, -2) if q == d else slice(1, -1) for q in range(3)) + (n,)
            A[n][d] = 0.5 * (np.abs(G[hi]) + np.abs(G[lo])) / dx[d] if bound else 0.5 * (G[hi] - G[lo]) * (1.0 / dx[d])
    U = [np.abs(G[c + (n,)]) if bound else G[c + (n,)] for n in range(3)]
    return A, U


def fields(G, dx, mu, bound=False):
    """the ten quantities (strain_rate as its square 2 SS under the key "strain_rate^2") in the kernel's order of evaluation; bound:
    every entry its magnitude bound, every subtraction an addition"""
    A, U = gradient(G, dx, bound)
    sub = (lambda a, b: a + b) if bound else (lambda a, b: a - b)
    f = {}
    f["diveru"] = (A[0][0] + A[1][1]) + A[2][2]
    wx, wy, wz = sub(A[2][1], A[1][2]), sub(A[0][2], A[2][0]), sub(A[1][0], A[0][1])
    f["vort_x"], f["vort_y"], f["vort_z"] = wx, wy, wz
    ens = 0.5 * (wx * wx + wy * wy + wz * wz)
    f["enstrophy"] = ens
    s01, s02, s12 = A[0][1] + A[1][0], A[0][2] + A[2][0], A[1][2] + A[2][1]
    ss = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + 0.5 * (s01 * s01 + s02 * s02 + s12 * s12)
    f["strain_rate^2"] = 2 * ss
    f["dissipation"] = abs(mu) * (2 * ss) if bound else mu * (2 * ss)
    f["q_criterion"] = 0.5 * sub(ens, ss)
    det = sub(A[0][0] * sub(A[1][1] * A[2][2], A[1][2] * A[2][1]), A[0][1] * sub(A[1][0] * A[2][2], A[1][2] * A[2][0])) \
        + A[0][2] * sub(A[1][0] * A[2][1], A[1][1] * A[2][0])
    f["r_invariant"] = det if bound else -det
    f["helicity"] = U[0] * wx + U[1] * wy + U[2] * wz
    return f


def check_fields(got, G, dx, mu, names, tag):
    """got (nx, ny, nz, len(names)) against the yardstick on G (one ghost layer); prints the worst error in units of the bound"""
    want, B = fields(G, dx, mu), fields(G, dx, mu, bound=True)
    worst = 0.0
    for q, nm in enumerate(names):
        key = "strain_rate^2" if nm == "strain_rate" else nm
        g = got[..., q] * got[..., q] if nm == "strain_rate" else got[..., q]
        assert np.isfinite(g).all(), (tag, nm)
        if nm == "strain_rate":
            assert (got[..., q] >= 0.0).all()
        err, bd = np.abs(g - want[key]), 32 * EPS * B[key]
        w = float(np.max(err / np.where(bd > 0, bd, 1.0)))
        worst = max(worst, w)
        print(f"{tag} {nm}: max |got - want| = {float(err.max()):.3e}, worst error / bound = {w:.3f}, bit-equal cells {int((g == want[key]).sum())} of {g.size}")
        assert np.all(err <= bd), (tag, nm, w)
    return worst


# ------------------------------------------------------------------------------------------------------------------ 1 / 2. the kernel
DX = (1.0 / 16, 0.7 / 16, 1.3 / 16)
SHAPES = {
    "one_tile": ((32, 8, 2), None),
    "remainders": ((33, 9, 3), None),
    "one_plane": ((64, 16, 1), None),
    "odd_box": ((40, 24, 5), None),
    # lower corners (33, 0), (33, 13): not on the tile grid; the 7-wide boxes are smaller than a tile, beside one that holds a full tile
    "unequal_boxes": ((40, 24, 5), [((0, 0, 0), (32, 23, 4)), ((33, 0, 0), (39, 12, 4)), ((33, 13, 0), (39, 23, 4))]),
    "small_boxes": ((8, 8, 8), [((i, j, k), (i + 3, j + 3, k + 3)) for k in (0, 4) for j in (0, 4) for i in (0, 4)]),
}
MARCHING = ["one_tile", "remainders", "one_plane", "odd_box", "unequal_boxes"]


def kernel_case(name, seed=0):
    """(geom, vel with TWO ghost layers, G, n): the first layer holds random values, the second layer and every edge and corner cell of
    the first hold NaN; G: the global velocity with one ghost layer, index origin -1"""
    from iamr_amd import lib as L
    n, boxes = SHAPES[name]
    lay = L.Layout(boxes) if boxes else L.Layout.single(n)
    g = L.Geom.make(list(n), prob_hi=tuple(DX[d] * n[d] for d in range(3)), periodic=(0, 0, 0))
    rng = np.random.default_rng(100 + seed + sum(n))
    G = rng.uniform(-1.0, 1.0, size=tuple(v + 2 for v in n) + (3,)) + np.array([0.3, -0.2, 0.1])
    vel = L.MultiFab(lay, L.CELL, 3, 2)
    for li in range(vel.nlocal()):
        glo, ghi = vel.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (3,), np.nan, order="F")
        # the box grown by one cell, from G ...
        a[1:-1, 1:-1, 1:-1] = G[tuple(slice(lo[d] - 1 + 1, hi[d] + 1 + 2) for d in range(3))]
        # ... without its edges and corners: a cell outside the box in two or more directions
        idx = np.meshgrid(*[np.arange(glo[d], ghi[d] + 1) for d in range(3)], indexing="ij")
        nout = sum(((idx[d] < lo[d]) | (idx[d] > hi[d])).astype(int) for d in range(3))
        a[nout >= 2] = np.nan
        vel.from_numpy(a, li)
    return g, lay, vel, G, n


def run_kernel(g, lay, vel, which, path=0, mu=0.37, one_at_a_time=False):
    """-> (out valid cells gathered (n, len(which)), the fabs with their ghost layer)"""
    from iamr_amd import lib as L
    out = L.MultiFab(lay, L.CELL, len(which), 1)
    out.setval(SENTINEL)
    if one_at_a_time:
        for q, w in enumerate(which):
            L.derive_velgrad(g, out, vel, [w], ocomp=q, mu=mu, path=path)
    else:
        L.derive_velgrad(g, out, vel, which, mu=mu, path=path)
    return out


def valid_and_ghosts(out, lay, n):
    G = out.gather_valid(n)
    for li in range(out.nlocal()):
        a, _ = out.to_numpy(li)
        shell = np.ones(a.shape[:3], dtype=bool)
        shell[1:-1, 1:-1, 1:-1] = False
        assert np.all(a[shell] == SENTINEL), "a ghost cell of out was written"
    return G


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_against_numpy(gpu, name):
    from iamr_amd import lib as L
    g, lay, vel, G, n = kernel_case(name)
    assert L.velgrad_path(vel, 0) == (1 if name in MARCHING else 2)
    got = valid_and_ghosts(run_kernel(g, lay, vel, TEN), lay, n)
    assert not np.isnan(got).any() and not np.any(got == SENTINEL)
    check_fields(got, G, DX, 0.37, TEN, name)
    single = valid_and_ghosts(run_kernel(g, lay, vel, TEN, one_at_a_time=True), lay, n)
    assert single.tobytes() == got.tobytes()
    # a subset in another order, into the middle of a wider array
    sub = ["helicity", "diveru", "q_criterion"]
    out = L.MultiFab(lay, L.CELL, 5, 0)
    out.setval(SENTINEL)
    L.derive_velgrad(g, out, vel, sub, ocomp=1, mu=0.37)
    S = out.gather_valid(n)
    assert np.all(S[..., 0] == SENTINEL) and np.all(S[..., 4] == SENTINEL)
    assert np.ascontiguousarray(S[..., 1:4]).tobytes() == np.ascontiguousarray(got[..., [9, 0, 7]]).tobytes()


@pytest.mark.parametrize("name", MARCHING)
def test_forms_agree(gpu, name):
    g, lay, vel, G, n = kernel_case(name, seed=1)
    a = valid_and_ghosts(run_kernel(g, lay, vel, TEN, path=1), lay, n)
    b = valid_and_ghosts(run_kernel(g, lay, vel, TEN, path=2), lay, n)
    assert not np.isnan(a).any() and np.array_equal(a, b) and a.tobytes() == b.tobytes()


def test_kernel_errors(gpu):
    from iamr_amd import lib as L
    from iamr_amd.lib import IamrxError
    g, lay, vel, G, n = kernel_case("small_boxes")
    with pytest.raises(IamrxError, match="path 1"):
        run_kernel(g, lay, vel, TEN, path=1)
    with pytest.raises(IamrxError):
        run_kernel(g, lay, vel, TEN, path=3)
    with pytest.raises(IamrxError):
        L.derive_velgrad(g, L.MultiFab(lay, L.CELL, 2, 0), vel, [0, 10])                 # an id outside 0 .. 9
    with pytest.raises(IamrxError):
        L.derive_velgrad(g, L.MultiFab(lay, L.CELL, 2, 0), vel, [0, 1, 2])               # three outputs into two components
    with pytest.raises(IamrxError):
        L.derive_velgrad(g, L.MultiFab(lay, L.CELL, 1, 0), L.MultiFab(lay, L.CELL, 3, 0), [0])      # no ghost layer
    assert L.velgrad_path(vel, 2) == 2


# ------------------------------------------------------------------------------------------------------------------ 3. layouts
N3 = (32, 16, 8)


def periodic_G(S):
    return np.pad(S[..., :3], ((1, 1), (1, 1), (1, 1), (0, 0)), mode="wrap")


def test_layout_independence(gpu):
    """the same periodic field in 1, 4 and 16 boxes through a level object: the same bits"""
    S = random_state(N3, 41)
    got = []
    for mgs, nb in ((None, 1), ((16, 8, 8), 4), ((8, 8, 4), 16)):
        ns, lay = one_level(N3, S, mgs)
        assert len(lay.boxes) == nb
        got.append(ns.derive(TEN).gather_valid(N3))
        assert got[-1].shape == N3 + (10,)
    check_fields(got[0], periodic_G(S), [1.0 / v for v in N3], 0.0, TEN, "one box")
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 4. identities
def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_discrete_identities(gpu):
    """centred differences commute and are skew-adjoint on a periodic level: sum q + sum diveru^2 / 2 = 0; the three components are the
    terms under the root of mag_vort"""
    S = random_state(N3, 43)
    ns, lay = one_level(N3, S, (16, 8, 8))
    f = ns.derive(["q_criterion", "diveru", "vort_x", "vort_y", "vort_z", "enstrophy"]).gather_valid(N3)
    q, div, wx, wy, wz, ens = (f[..., c] for c in range(6))
    terms = np.concatenate([q.ravel(), 0.5 * (div * div).ravel()])
    total, bound = math.fsum(terms), 32 * EPS * q.size * float(np.abs(terms).max())
    print(f"sum q + sum div^2 / 2 = {total:.3e}, bound {bound:.3e}, sum |terms| = {float(np.abs(terms).sum()):.3e}")
    assert abs(total) <= bound
    mv = ns.derive("mag_vort").gather_valid(N3)[..., 0]
    assert mv.min() > 0.0
    assert ulps(np.sqrt(wx * wx + wy * wy + wz * wz), mv).max() <= 4
    assert ulps(2 * ens, mv * mv).max() <= 4
    # a single name through derive(str) is the same field
    assert ns.derive("q_criterion").gather_valid(N3)[..., 0].tobytes() == np.ascontiguousarray(q).tobytes()


# ------------------------------------------------------------------------------------------------------------------ 5. known answer
def test_taylor_green_known_answer(gpu):
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    n, mu = (16, 16, 16), 0.01
    g = L.Geom.make(list(n), periodic=(1, 1, 1))
    lay = L.Layout.decompose(n, 8)
    ns = N.NavierStokes(g, lay, N.ns_params(visc_coef=mu))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    names = ["diveru", "vort_z", "enstrophy", "dissipation"]
    f = ns.derive(names).gather_valid(n)
    dx, k = 1.0 / 16, 2 * np.pi
    x = (np.arange(16) + 0.5) * dx
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    kd = np.sin(k * dx) / dx                               # the centred difference of sin / cos(k x): the discrete wavenumber
    sx, cx, sy, cy, sz, cz = np.sin(k * X), np.cos(k * X), np.sin(k * Y), np.cos(k * Y), np.sin(k * Z), np.cos(k * Z)
    # u = sx cy cz, v = -cx sy cz, w = 0
    ux, uy, uz = kd * cx * cy * cz, -kd * sx * sy * cz, -kd * sx * cy * sz
    vx, vy, vz = kd * sx * sy * cz, -kd * cx * cy * cz, kd * cx * sy * sz
    wx_, wy_, wz_ = -vz, uz, vx - uy
    ss = ux * ux + vy * vy + 0.5 * ((uy + vx) ** 2 + uz ** 2 + vz ** 2)
    want = [np.zeros(n), wz_, 0.5 * (wx_ ** 2 + wy_ ** 2 + wz_ ** 2), mu * 2 * ss]
    # The tolerance, from the two sides' rounding.  The arguments k x are the same doubles on both sides; a velocity sample (two products
    # of three library sines / cosines of at most 2 ulp each, magnitude <= 1) is within 8 eps of the exact product, so a computed
    # entry 0.5 (a - b) / dx is within 8 eps / dx of the exact difference, which IS kd cos(k x) ... ; the analytic side adds 32 eps of
    # its own (kd and three factors): dA = 8 eps / dx + 32 eps.  Entries are at most kd in magnitude.
    #   diveru, vort_z: two non-zero entries each                                   -> 2 dA
    #   enstrophy = (wx^2 + wy^2 + wz^2) / 2, |wx|, |wy| <= kd, |wz| <= 2 kd       -> kd dA + kd dA + 2 kd 2 dA = 6 kd dA
    #   2 SS = 2 (ux^2 + vy^2) + (uy + vx)^2 + uz^2 + vz^2                          -> (4 + 4 + 8 + 2 + 2) kd dA = 20 kd dA, times mu
    dA = 8 * EPS / dx + 32 * EPS
    tol = [2 * dA, 2 * dA, 6 * kd * dA, mu * 20 * kd * dA]
    for q, nm in enumerate(names):
        err = float(np.abs(f[..., q] - want[q]).max())
        print(f"TaylorGreen {nm}: max error {err:.3e}, tolerance {tol[q]:.3e}")
        assert err <= tol[q], nm
    assert float(np.abs(want[1]).max()) > 1.0 and float(want[3].max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------ 6. hierarchy
def level_velocity(amr, l):
    """the FillPatched velocity of level l at the new time, one ghost layer, on the level's layout"""
    from iamr_amd import lib as L
    lev, lay, t = amr.levels[l], amr.layouts[l], amr.time
    S = lev.data(lev.S_NEW)
    vel = L.MultiFab(lay, L.CELL, 3, 1)
    if l == 0:
        L.parallel_copy(vel, S, 0, 0, 3)
        vel.fill_boundary(amr.level_geom(0))
    else:
        crse = amr.levels[l - 1]
        L.fillpatch_two_levels(vel, t, (None, S, t, t), (None, crse.data(crse.S_NEW), t, t), amr.level_geom(l - 1), amr.level_geom(l), 0, 3)
    return vel


def test_hierarchy(gpu):
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    mu = 0.01
    amr, lays, g0 = R.build_amr(Inputs([AMR16], ["ns.vel_visc_coef=0.01"]).problem(), L, N)
    amr.post_init(-1.0)
    amr.coarse_step()
    assert amr.nlev == 3
    n0 = list(amr.geom0.n)
    names = ["x_velocity", "q_criterion", "energy", "r_invariant", "vort_z", "dissipation"]
    vg = [1, 3, 4, 5]
    derived, states = [], []
    for l in range(amr.nlev):
        lev, lay, nl = amr.levels[l], amr.layouts[l], [v << l for v in n0]
        dx = [1.0 / v for v in nl]
        vel, out = level_velocity(amr, l), lev.derive(names)
        S = lev.data(lev.S_NEW)
        for li in range(out.nlocal()):
            o, G, s = out.to_numpy(li)[0], vel.to_numpy(li)[0], S.to_numpy(li)[0]
            ng = (s.shape[0] - o.shape[0]) // 2
            s = s[ng:s.shape[0] - ng, ng:s.shape[1] - ng, ng:s.shape[2] - ng]
            assert np.isfinite(G[1:-1, 1:-1, 1:-1]).all()
            check_fields(o[..., vg], G, dx, mu, [names[q] for q in vg], f"level {l} box {li}")
            assert np.array_equal(o[..., 0], s[..., 0])
            assert np.array_equal(o[..., 2], 0.5 * s[..., 3] * (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1] + s[..., 2] * s[..., 2]))
        derived.append(lev.derive(["enstrophy", "dissipation"]).gather_valid(nl))
        states.append(S.gather_valid(nl))
    # the composite integrals
    boxes = [amr.layouts[l].boxes for l in range(amr.nlev)]
    counted = HN.counted_masks(boxes, n0)
    a, b = amr.integrate(["density", "tracer", "energy"]), np.array(amr.sum_integrated())
    vol = [(1.0 / (n0[0] << l)) ** 3 for l in range(amr.nlev)]
    ke = [0.5 * s[..., 3] * (s[..., 0] ** 2 + s[..., 1] ** 2 + s[..., 2] ** 2) for s in states]
    mags = [sum(vol[l] * math.fsum(np.abs(c[l][counted[l]])) for l in range(amr.nlev)) for c in ([s[..., 3] for s in states], [s[..., 4] for s in states], ke)]
    print("integrate", a, "sum_integrated", b, "sums of magnitudes", mags)
    assert np.all(np.abs(a - b) <= 1e-13 * np.array(mags)) and a[0] > 0.0 and a[2] > 0.0
    got = amr.integrate(["enstrophy", "dissipation"])
    for q in range(2):
        terms = np.concatenate([derived[l][..., q][counted[l]] * (1.0 / (n0[0] << l)) ** 3 for l in range(amr.nlev)])
        want, mags = math.fsum(terms), math.fsum(np.abs(terms))
        print(f"integral {q}: got {got[q]:.17g} want {want:.17g}")
        assert want > 0.0 and abs(got[q] - want) <= 1e-13 * mags
    # one level of it: all cells
    lev = amr.levels[1]
    one = lev.integrate(["enstrophy"])[0]
    m = HN.box_mask(boxes[1], derived[1].shape[:3])
    w1 = math.fsum(derived[1][..., 0][m] * (1.0 / (n0[0] << 1)) ** 3)
    assert abs(one - w1) <= 1e-13 * w1


# ------------------------------------------------------------------------------------------------------------------ 7. histograms
def hist_slots(h):
    return np.concatenate([h["counts"], h["below"][:, None], h["above"][:, None], h["nan"][:, None]], axis=1)


def test_histograms(gpu):
    from iamr_amd.lib import IamrxError
    n = (20, 12, 6)
    ns, lay = one_level(n, random_state(n, 3), 8)
    names = ["q_criterion", "x_velocity", "r_invariant"]
    cols = ns.derive(names).gather_valid(n)
    assert np.isfinite(cols).all()
    ranges = [(0.5 * cols[..., 0].min(), 0.5 * cols[..., 0].max()), (-0.5, 1.0), (0.6 * cols[..., 2].min(), 0.4 * cols[..., 2].max())]
    h = ns.histogram(names, 32, ranges)
    ref = HN.hist_reference([cols], [lay.boxes], list(n), [r[0] for r in ranges], [r[1] for r in ranges], 32)
    assert np.array_equal(hist_slots(h), ref) and h["below"].sum() > 0 and h["above"].sum() > 0 and not h["nan"].any()
    h2 = ns.histogram2("r_invariant", "q_criterion", (6, 11), (ranges[2], ranges[0]))
    c2, o2 = HN.hist2(cols[..., 2], cols[..., 0], (ranges[2][0], ranges[0][0]), (ranges[2][1], ranges[0][1]), (6, 11))
    assert np.array_equal(h2["counts"], c2) and h2["outside"] == o2 and o2 > 0
    h3 = ns.histogram2("q_criterion", "density", (5, 7), (ranges[0], (0.75, 2.0)))       # a gradient name with a state name
    rho = ns.data(ns.S_NEW).gather_valid(n)[..., 3]
    c3, o3 = HN.hist2(cols[..., 0], rho, (ranges[0][0], 0.75), (ranges[0][1], 2.0), (5, 7))
    assert np.array_equal(h3["counts"], c3) and h3["outside"] == o3
    with pytest.raises(IamrxError, match="mag_vort") as e:
        ns.histogram(["x_velocity", "vorticity"], 8, [(0.0, 1.0), (0.0, 1.0)])
    assert "q_criterion" in str(e.value)
    # the hierarchy: TaylorGreen initial data, automatic range
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    amr, lays, g0 = R.build_amr(Inputs([AMR16]).problem(), L, N)
    amr.post_init(-1.0)
    n0 = list(amr.geom0.n)
    boxes = [amr.layouts[l].boxes for l in range(amr.nlev)]
    f = [amr.levels[l].derive(names).gather_valid([v << l for v in n0]) for l in range(amr.nlev)]
    h = amr.histogram(names, 32)
    assert np.array_equal(hist_slots(h), HN.hist_reference(f, boxes, n0, h["range"][:, 0], h["range"][:, 1], 32))
    assert not h["below"].any() and not h["above"].any() and not h["nan"].any()
    lo, hi = (h["range"][2][0], h["range"][0][0]), (h["range"][2][1], h["range"][0][1])
    h2 = amr.histogram2("r_invariant", "q_criterion", (8, 8), ((lo[0], hi[0]), (lo[1], hi[1])))
    c2, o2 = HN.hist2_reference([a[..., 2] for a in f], [a[..., 0] for a in f], boxes, n0, lo, hi, (8, 8))
    assert np.array_equal(h2["counts"], c2) and h2["outside"] == o2 == 0


# ------------------------------------------------------------------------------------------------------------------ 8. driver
def test_driver_plotfile_with_the_files_own_keys(gpu, tmp_path, monkeypatch):
    """inputs.3d.forced with its own amr.derive_plot_vars = mag_vort diveru avg_pressure: the plotfile holds them, diveru is derive's"""
    from iamr_amd import run as R
    from iamr_amd.plotfile import PlotFile
    seen = {}

    def observe(run, step, dt):
        if step == 2:
            seen["diveru"] = run.derive("diveru").gather_valid((16, 16, 16))[..., 0]
            seen["mag_vort"] = run.derive("mag_vort").gather_valid((16, 16, 16))[..., 0]

    monkeypatch.chdir(tmp_path)
    assert R.main([FORCED, "amr.n_cell=16 16 16", "max_step=2", "amr.plot_int=2", "amr.check_int=-1", "amr.max_grid_size=8"], observe) == 0
    pf = PlotFile.read(str(tmp_path / "plt00002"))
    assert pf.names[-3:] == ["mag_vort", "diveru", "avg_pressure"]
    lv = pf.levels[0]
    got = np.zeros((16, 16, 16, len(pf.names)))
    for (lo, hi), a in zip(lv.boxes, lv.data):
        got[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] = a
    assert np.array_equal(got[..., pf.names.index("diveru")], seen["diveru"])
    assert np.array_equal(got[..., pf.names.index("mag_vort")], seen["mag_vort"])
    assert np.abs(seen["diveru"]).max() > 0.0


def test_driver_integrals(gpu, tmp_path, monkeypatch):
    from iamr_amd import run as R
    from iamr_amd.integrals import read_integrals
    names = ["energy", "enstrophy", "dissipation"]
    seen = {}

    def observe(run, step, dt):
        seen[step] = (run.time, run.integrate(names))

    d1 = tmp_path / "on"
    d1.mkdir(exist_ok=True)          # (the test may run once per box mode)
    monkeypatch.chdir(d1)
    assert R.main([AMR16, "ns.vel_visc_coef=0.01", "max_step=2", "ns.integrate_interval=1", 'ns.integrate_vars="energy enstrophy dissipation"'] + QUIET, observe) == 0
    assert os.listdir(d1) == ["integ"]
    r = read_integrals(str(d1 / "integ"))
    assert r["names"] == tuple(names) and np.array_equal(r["step"], [0, 1, 2])
    for row, step in enumerate((0, 1, 2)):
        assert r["time"][row] == seen[step][0]
        for q, nm in enumerate(names):
            assert r[nm][row] == seen[step][1][q] and r[nm][row] > 0.0, (step, nm)
    assert r["energy"][2] < r["energy"][0]                               # (the viscous run loses energy)
    # without the keys nothing is written
    d2 = tmp_path / "off"
    d2.mkdir(exist_ok=True)
    monkeypatch.chdir(d2)
    assert R.main([AMR16, "max_step=1"] + QUIET) == 0
    assert os.listdir(d2) == []


def test_driver_slab_accepts_dissipation(gpu, tmp_path, monkeypatch):
    from iamr_amd import run as R
    from iamr_amd.integrals import read_integrals
    monkeypatch.chdir(tmp_path)
    assert R.main([DSL2D, "max_step=1", "ns.vel_visc_coef=0.001", "ns.integrate_interval=1", "ns.integrate_vars=dissipation enstrophy",
                   "amr.derive_plot_vars=dissipation", "amr.plot_int=1", "amr.check_int=-1"]) == 0
    r = read_integrals(str(tmp_path / "integ"))
    assert np.array_equal(r["step"], [0, 1]) and np.all(r["dissipation"] > 0.0) and np.all(r["enstrophy"] > 0.0)
    from iamr_amd.plotfile import PlotFile
    pf = PlotFile.read(str(tmp_path / "plt00001"))
    assert pf.names[-1] == "dissipation" and all(np.isfinite(a).all() and a[..., -1].max() > 0.0 for a in pf.levels[0].data)


# ------------------------------------------------------------------------------------------------------------------ 9. two ranks
N9, MGS9 = (16, 16, 8), 8
NAMES9 = ["q_criterion", "x_velocity", "r_invariant", "helicity", "energy", "dissipation"]


def _two_ranks(rank, world, port, out_dir):
    lib = ranks.start_rank(rank, world, port)
    from iamr_amd import ns as N
    g = lib.Geom.make(list(N9), periodic=(1, 1, 1))
    lay = lib.Layout.decompose(N9, MGS9, world)
    ns = N.NavierStokes(g, lay, N.ns_params(visc_coef=0.02))
    ns.init_rest(1.0)
    put_state(ns, lay, random_state(N9, 91))
    out = ns.derive(NAMES9)
    integ = ns.integrate(NAMES9)
    idx = [lay.local_box(li)[2] for li in range(lay.nlocal())]
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), idx=np.array(idx), integ=integ, **{f"box{q}": out.to_numpy(li)[0] for li, q in enumerate(idx)})
    ranks.stop_rank()


@pytest.mark.merged_only
def test_two_ranks_on_one_device(gpu, tmp_path):
    """the boxes of one level dealt to two ranks (sharing the device over the gloo callback transport): the fields of every box are the
    one-rank fields to the bit, the integrals agree within 1e-13 of the sum of magnitudes"""
    ranks.spawn(_two_ranks, 2, ranks.free_port(), str(tmp_path))
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    S = random_state(N9, 91)
    lay = L.Layout.decompose(N9, MGS9)
    ns = N.NavierStokes(L.Geom.make(list(N9), periodic=(1, 1, 1)), lay, N.ns_params(visc_coef=0.02))
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    ref = ns.derive(NAMES9).gather_valid(N9)
    want = ns.integrate(NAMES9)
    mags = np.abs(ref).sum(axis=(0, 1, 2)) / (N9[0] * N9[1] * N9[2])
    seen = set()
    for rank in range(2):
        z = np.load(str(tmp_path / f"r{rank}.npz"))
        assert len(z["idx"]) == 2
        for q in z["idx"]:
            lo, hi = lay.boxes[int(q)]
            assert z[f"box{q}"].tobytes() == np.ascontiguousarray(ref[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]).tobytes(), (rank, q)
            seen.add(int(q))
        print("rank", rank, "integrals", z["integ"], "one rank", want)
        assert np.all(np.abs(z["integ"] - want) <= 1e-13 * mags)
    assert seen == set(range(len(lay.boxes)))
