"""CPU: the long-double reference of tests/tensor_numpy.py against the oracle's tensor operator (orc_tensor_apply_bcn,
orc_tensor_extensive_flux) on every case of tests/test_gpu_tensor_bc_matrix.py, and the conditions on those cases that keep a GPU
case from passing vacuously (asserted on the reference and the layouts alone).

The distance measured here -- a double evaluation from the exact one -- is what the bars of the GPU module stand on: it stays below
1e-14 of max |y| (and of max |flux_d|) and below 1e-15 max |u| in the ghost cells, two decades and more under the GPU bars of
1e-12 and 1e-13.  Largest distances seen: DESIGN.md section 2."""
import ctypes as C
import numpy as np
import pytest

import tensor_numpy as tn

Y_BAR, FLUX_BAR, GHOST_BAR = 1e-14, 1e-14, 1e-15


def oracle_case(orc, cs, fac=1.0):
    """orc_tensor_apply_bcn + orc_tensor_extensive_flux on the inputs of a case -> (u after the fill, y, [flux_d])"""
    L = orc.lib()
    n = cs["n"]
    g = orc.geom(n, probhi=cs["prob_hi"], periodic=cs["bc"]["per"])
    u = orc.Fab(n, orc.CELL, 1, 3); u.a[...] = cs["u"]
    eta = []
    for d in range(3):
        e = orc.Fab(n, orc.face(d), 0, 1); e.a[...] = cs["eta"][d]; eta.append(e)
    ac = None
    if cs["acoef"] is not None:
        ac = orc.Fab(n, orc.CELL, 0, 1); ac.a[...] = cs["acoef"]
    y = orc.Fab(n, orc.CELL, 0, 3)
    lo9, hi9 = (C.c_int * 9)(*cs["bc"]["lo"]), (C.c_int * 9)(*cs["bc"]["hi"])
    L.orc_tensor_apply_bcn(C.byref(g), y.ref(), u.ref(), C.c_double(cs["a"]), C.c_double(cs["b"]), ac.ref() if ac is not None else None,
                           orc.fabptrs(eta), lo9, hi9, cs["maxorder"])
    fl = [orc.Fab(n, orc.face(d), 0, 3, fill=7.0e30) for d in range(3)]
    L.orc_tensor_extensive_flux(C.byref(g), 0, None, 2, orc.fabptrs(fl), u.ref(), orc.fabptrs(eta), C.c_double(fac), 0, None, cs["maxorder"])
    return u.a, y.a, [f.a for f in fl]


def distances(cs, u, y, fl):
    """(ghost cells / max |u|, y / max |y|, max_d flux_d / max |flux_d|) of double results from the reference of a case; max |u| is
    taken over the filled array, ghost layer included (an extrapolated ghost value can exceed every cell)"""
    ref_u = cs["u_filled"]
    du = float(np.abs(u - ref_u).max() / np.abs(ref_u).max())
    dy = float(np.abs(y - cs["y"]).max() / np.abs(cs["y"]).max())
    df = max(float(np.abs(fl[d] - cs["flux"][d]).max() / np.abs(cs["flux"][d]).max()) for d in range(3))
    return du, dy, df


MATRIX = [(lay, visc, mo) for lay in tn.LAYOUTS for visc in tn.VISCOSITIES for mo in tn.MAXORDERS]


@pytest.mark.parametrize("layout,visc,maxorder", MATRIX)
def test_reference_equals_oracle(orc, layout, visc, maxorder):
    """ghost cells (faces, edges, corners), y and the fluxes of all three directions, every BC set"""
    worst = [0.0, 0.0, 0.0]
    for bc in tn.BC_SETS:
        cs = tn.case(layout, visc, bc["name"], maxorder)
        d = distances(cs, *oracle_case(orc, cs))
        worst = [max(a, b) for a, b in zip(worst, d)]
        assert d[0] <= GHOST_BAR and d[1] <= Y_BAR and d[2] <= FLUX_BAR, (bc["name"], d)
    print(f"\n[tensor ref/oracle] {layout} {visc} maxorder {maxorder}: ghost {worst[0]:.2e} y {worst[1]:.2e} flux {worst[2]:.2e}")


@pytest.mark.parametrize("layout,visc,form,prob_hi", [
    (tn.TILE_LAYOUTS[0], "constant", "implicit", tn.PROB_HI), (tn.TILE_LAYOUTS[1], "array", "implicit", tn.PROB_HI),
    (tn.TILE_LAYOUTS[0], "constant", "explicit", tn.PROB_HI_ANISO), (tn.TILE_LAYOUTS[0], "array", "explicit", tn.PROB_HI_ANISO)])
def test_reference_equals_oracle_forms_and_cell_sizes(orc, layout, visc, form, prob_hi):
    """the a-term, and three different cell sizes"""
    for bcname, mo in (("yhi-symmetry", 2), ("zlo-slip", 3), ("periodic-y", 3)):
        cs = tn.case(layout, visc, bcname, mo, form, prob_hi)
        d = distances(cs, *oracle_case(orc, cs))
        assert d[0] <= GHOST_BAR and d[1] <= Y_BAR and d[2] <= FLUX_BAR, (bcname, d)
    if prob_hi is tn.PROB_HI_ANISO:
        h = cs["h"]
        assert len({round(v * 1e6) for v in h}) == 3, h


def test_reference_is_consistent():
    """the operator on polynomial fields whose exact result is known: every coefficient of tau on every face direction"""
    n, h = (6, 5, 4), (0.5, 0.25, 0.125)
    ax = [(np.arange(-1, n[d] + 1) + 0.5) * h[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    u = np.stack([X * Y + 2 * X * X + Z * Z, 3 * Y * Z + X * X - Y * Y, X * Z + 5 * Y * Y + 4 * Z * Z], axis=-1)
    eta = [np.full(tuple(n[e] + (e == d) for e in range(3)), 0.5) for d in range(3)]
    # div tau = eta (lap u + grad div u) - 2/3 eta grad div u = eta (lap u + 1/3 grad div u): div u = 5 x - 2 y + 11 z + ... exactly
    # u_x = y + 4 x, v_y = 3 z - 2 y, w_z = x + 8 z -> div u = 5 x - y + 11 z, grad div u = (5, -1, 11); lap u = (6, 0, 18)
    y = tn.apply(u, eta, 0.0, -1.0, None, h)
    want = 0.5 * (np.array([6.0, 0.0, 18.0]) + np.array([5.0, -1.0, 11.0]) / 3.0)
    assert np.abs(y - want).max() <= 1e-15 * np.abs(u).max() / min(h) ** 2
    fl = tn.extensive_flux(u, eta, 2.0, h)
    # x-face between the cells i - 1 and i at x = i h: tau_xx = eta (4/3 u_x - 2/3 (v_y + w_z))
    xf = np.arange(n[0] + 1) * h[0]
    Xf, Yc, Zc = np.meshgrid(xf, ax[1][1:-1], ax[2][1:-1], indexing="ij")
    txx = 0.5 * (4.0 / 3.0 * (Yc + 4 * Xf) - 2.0 / 3.0 * ((3 * Zc - 2 * Yc) + (Xf + 8 * Zc)))
    assert np.abs(fl[0][..., 0] + 2.0 * h[1] * h[2] * txx).max() <= 1e-14
    txy = 0.5 * (2 * Xf + Xf)            # eta (dv/dx + du/dy) = eta (2 x + x)
    assert np.abs(fl[0][..., 1] + 2.0 * h[1] * h[2] * txy).max() <= 1e-14


def test_ghost_rules_by_hand():
    """a 2 x 2 x 2 box: face, edge and corner values of the three rules written out"""
    rng = np.random.default_rng(3)
    u = rng.standard_normal((4, 4, 4, 3))
    lo, hi = tn._bc9((0, 0, 0), {(0, 0, 0): tn.NEU, (0, 1, 0): tn.ODD})
    f = tn.fill_ghosts(u, u, (0, 0, 0), lo, hi, 2)
    L = np.longdouble
    assert np.array_equal(f[1:-1, 1:-1, 1:-1], u[1:-1, 1:-1, 1:-1].astype(L))
    assert f[0, 1, 1, 0] == L(u[1, 1, 1, 0])                             # Neumann
    assert f[1, 0, 1, 0] == -L(u[1, 1, 1, 0])                            # reflect_odd
    assert f[1, 1, 0, 0] == 2 * L(u[1, 1, 0, 0]) - L(u[1, 1, 1, 0])      # Dirichlet, two points
    assert f[0, 1, 1, 1] == 2 * L(u[0, 1, 1, 1]) - L(u[1, 1, 1, 1])      # component 1 is Dirichlet at x-lo
    # the edge x-lo / y-lo of component 0: mean of Neumann along x on the y-ghost row and reflect_odd along y on the x-ghost row
    assert f[0, 0, 1, 0] == (f[1, 0, 1, 0] - f[0, 1, 1, 0]) / 2
    # the corner: mean of the three rules on the edge cells, the Dirichlet one with the value stored in the corner itself
    assert abs(f[0, 0, 0, 0] - (f[1, 0, 0, 0] - f[0, 1, 0, 0] + 2 * L(u[0, 0, 0, 0]) - f[0, 0, 1, 0]) / 3) <= 1e-18
    f3 = tn.fill_ghosts(u, u, (0, 0, 0), lo, hi, 3)
    assert abs(f3[1, 1, 0, 0] - (L(8) / 3 * u[1, 1, 0, 0] - 2 * L(u[1, 1, 1, 0]) + L(u[1, 1, 2, 0]) / 3)) <= 1e-18
    g = tn.fill_ghosts(u, u, (1, 0, 0), *tn._bc9((1, 0, 0)), 2)
    assert np.array_equal(g[0], g[2]) and np.array_equal(g[3], g[1])      # images, the ghost cells of the other directions included


# ---------------------------------------------------------------------------------------------------------------------------
# conditions that keep the GPU cases from passing vacuously
def _layers(y, face, lo, hi):
    """the cell layers lo..hi - 1 counted from a face"""
    d, s = face
    sl = [slice(None)] * 3
    sl[d] = slice(lo, hi) if s == 0 else slice(y.shape[d] - hi, y.shape[d] - lo)
    return y[tuple(sl)]


@pytest.mark.parametrize("visc", tn.VISCOSITIES)
def test_every_single_bc_change_shows_next_to_its_face(visc):
    """36 changes of one (face, type, component) from the all-Dirichlet box: the result changes by more than 1e-2 max |y| in the cell
    layer at the face and not at all more than two cells away"""
    n = tn.LAYOUTS[tn.TILE_LAYOUTS[0]]["n"]
    base = tn.build(n, visc, tn.ALL_DIRICHLET, 2)["y"]
    scale = np.abs(base).max()
    smallest = np.inf
    for face in tn.FACES:
        for code in (tn.NEU, tn.ODD):
            for comp in range(3):
                y = tn.build(n, visc, tn.single_change(face, code, comp), 2)["y"]
                diff = np.abs(y - base)
                near = float(_layers(diff, face, 0, 1).max() / scale)
                smallest = min(smallest, near)
                assert near > 1e-2, (face, code, comp, near)
                assert _layers(diff, face, 2, n[face[0]]).max() == 0.0, (face, code, comp)
    print(f"\n[tensor bc effect] {visc}: smallest single change {smallest:.2e} of max |y|")


def test_every_bc_set_differs_from_all_dirichlet_at_its_face():
    """the sets of the GPU matrix themselves, on every layout"""
    for layout in tn.LAYOUTS:
        base = tn.case(layout, "constant", "all-101", 2)["y"]
        scale = np.abs(base).max()
        for bc in tn.BC_SETS:
            y = tn.case(layout, "constant", bc["name"], 2)["y"]
            assert np.abs(y - base).max() > 1e-2 * scale, (layout, bc["name"])


def test_maxorder_and_periodicity_show():
    n = tn.LAYOUTS[tn.TILE_LAYOUTS[0]]["n"]
    y2 = tn.build(n, "constant", tn.ALL_DIRICHLET, 2)["y"]
    y3 = tn.build(n, "constant", tn.ALL_DIRICHLET, 3)["y"]
    scale = np.abs(y2).max()
    for face in tn.FACES:
        assert _layers(np.abs(y3 - y2), face, 0, 1).max() > 1e-2 * scale, face
    per = (0, 1, 0)
    lo, hi = tn._bc9(per)
    yp = tn.build(n, "constant", dict(name="p", per=per, lo=lo, hi=hi, boost=None), 2)["y"]
    for face in ((1, 0), (1, 1)):
        assert _layers(np.abs(yp - y2), face, 0, 1).max() > 1e-2 * scale, face


def test_layouts_reach_the_paths_they_are_named_for():
    for name, L in tn.LAYOUTS.items():
        n, boxes = L["n"], L["boxes"]
        cover = np.zeros(n, dtype=int)
        for lo, hi in boxes:
            cover[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] += 1
        assert np.all(cover == 1), name
        ml = tn.max_len(boxes)
        if "tile path" in name:
            assert ml[0] >= 32 and ml[1] >= 8, (name, ml)
        if "plain path" in name:
            assert (ml[0] < 32 or ml[1] < 8) and len(boxes) > 1, (name, ml)
        if "partial tiles" in name:
            assert ml[0] % 32 != 0 and ml[1] % 8 != 0 and ml[2] % tn.z_chunk(ml[2]) != 0, (name, ml)
        if "dead tiles" in name:
            assert any(hi[0] - lo[0] + 1 < ml[0] for lo, hi in boxes) and any(hi[1] - lo[1] + 1 < ml[1] for lo, hi in boxes), name
            assert len({tuple(hi[d] - lo[d] + 1 for d in range(3)) for lo, hi in boxes}) == len(boxes) == 8, name
    assert tn.LAYOUTS["tile path, dead tiles"]["n"] == (48, 16, 12) and tn.max_len(tn.LAYOUTS["tile path, dead tiles"]["boxes"]) == (40, 12, 8)
    for name in tn.TILE_LAYOUTS:
        h = tn.cell_sizes(tn.LAYOUTS[name]["n"], tn.PROB_HI)
        assert len({round(v * 1e9) for v in h}) >= 2, (name, h)


def test_inputs_are_what_the_matrix_asks_for():
    assert len(tn.BC_SETS) == 18 + 6 + 1 + 2 and len({b["name"] for b in tn.BC_SETS}) == len(tn.BC_SETS)
    n = (16, 12, 10)
    for kind in tn.VISCOSITIES:
        e = tn.viscosity(n, kind)
        ratio = max(v.max() for v in e) / min(v.min() for v in e)
        assert (ratio == 1.0 and e[0].flat[0] == 0.013) if kind == "constant" else ratio >= 1.8, (kind, ratio)
    u = tn.velocity(n, tn.ALL_DIRICHLET)
    vals = {(f, c): u[tuple((0 if f[1] == 0 else n[d] + 1) if d == f[0] else 1 + n[d] // 2 for d in range(3)) + (c,)]
            for f in tn.FACES for c in range(3)}
    assert len({round(v, 6) for v in vals.values()}) == 18 and min(abs(v) for v in vals.values()) > 0.05      # inhomogeneous, all different
    up = tn.velocity(n, tn.BC_BY_NAME["periodic-y"])
    assert np.array_equal(up[:, 0], up[:, n[1]]) and np.array_equal(up[:, n[1] + 1], up[:, 1])
