"""GPU: the viscous tensor operator (iamr_amd/csrc/k_tensor.hip) at walls on every kernel path, against the long-double reference of
tests/tensor_numpy.py -- face x BC type x component, lo / hi asymmetric sets, per-component (slip, symmetry) sets, periodic mixes, max_order
2 and 3, on layouts that reach the tile kernels with partial and dead tiles (k_tensor_uni, k_tensor_cross_zm) and the plain one
(k_tensor_cross) on several boxes; the a-term, the residual form, the tile shapes and the face-flux form of the constant-viscosity
kernel; the extensive fluxes.  tests/test_cpu_tensor_ref.py holds the reference against the oracle and the conditions on these cases.

Bars: 1e-12 of max |y| for the result, 1e-12 of max |flux_d| for the fluxes, 1e-13 max |u| for the ghost cells
-- a correct double evaluation stays below 1e-14 / 1e-15 (measured on the CPU on the same inputs), the smallest effect of a boundary
condition is 7e-2."""
import numpy as np
import pytest

import tensor_numpy as tn

pytestmark = pytest.mark.gpu

Y_BAR, FLUX_BAR, GHOST_BAR = 1e-12, 1e-12, 1e-13
SENTINEL = 7.0e30


class Dev:
    """the inputs of a case on the device, on the boxes of its layout"""

    def __init__(self, lib, cs):
        self.lib, self.cs = lib, cs
        n, per = cs["n"], cs["bc"]["per"]
        self.lay = lib.Layout(cs["boxes"])
        self.g = lib.Geom.make(n, prob_hi=cs["prob_hi"], periodic=per)
        self.vel = lib.MultiFab(self.lay, lib.CELL, 3, 1); self.vel.set_from_global(cs["u"], (-1, -1, -1))
        self.eta = []
        for d in range(3):
            m = lib.MultiFab(self.lay, lib.face(d), 1, 0); m.set_from_global(cs["eta"][d], (0, 0, 0)); self.eta.append(m)
        self.acoef = None
        if cs["acoef"] is not None:
            self.acoef = lib.MultiFab(self.lay, lib.CELL, 1, 0); self.acoef.set_from_global(cs["acoef"], (0, 0, 0))
        self.out = lib.MultiFab(self.lay, lib.CELL, 3, 0); self.out.setval(SENTINEL)
        lo9, hi9 = cs["bc"]["lo"], cs["bc"]["hi"]
        tri = lambda v: [list(v[3 * c:3 * c + 3]) for c in range(3)]
        alike = tri(lo9)[0] == tri(lo9)[1] == tri(lo9)[2] and tri(hi9)[0] == tri(hi9)[1] == tri(hi9)[2]
        self.lobc, self.hibc = (tri(lo9)[0], tri(hi9)[0]) if alike else (tri(lo9), tri(hi9))      # one triple, or one per component

    def apply(self):
        from iamr_amd import ns as N
        cs = self.cs
        N.tensor_apply(self.g, self.out, self.vel, cs["a"], cs["b"], self.acoef, self.eta, lobc=self.lobc, hibc=self.hibc, maxorder=cs["maxorder"])


def box_distance(mf, ref, glo, tag):
    """largest |mf - ref| over every box of mf (ghost cells included); ref: a global array with index origin glo.  Every box and
    component is visited, and no cell may keep the sentinel."""
    worst = 0.0
    assert mf.nlocal() == len(mf.layout.boxes), tag
    for li in range(mf.nlocal()):
        a, lo = mf.to_numpy(li)
        assert a.shape[3] == ref.shape[3], tag
        assert not np.any(a == SENTINEL), (tag, li, "cells the kernel did not write")
        sl = tuple(slice(lo[d] - glo[d], lo[d] - glo[d] + a.shape[d]) for d in range(3))
        assert ref[sl].shape == a.shape, (tag, li)
        worst = max(worst, float(np.abs(a - ref[sl]).max()))
    return worst


def check_apply(dev, tag, y_ref=None):
    """y on every box, and the ghost cells of the velocity after the call: faces, edges and corners of every box"""
    cs = dev.cs
    y_ref = cs["y"] if y_ref is None else y_ref
    dy = box_distance(dev.out, y_ref, (0, 0, 0), tag) / float(np.abs(y_ref).max())
    du = box_distance(dev.vel, cs["u_filled"], (-1, -1, -1), tag) / float(np.abs(cs["u_filled"]).max())
    assert dy <= Y_BAR and du <= GHOST_BAR, (tag, dy, du)
    return dy, du


@pytest.mark.parametrize("maxorder", tn.MAXORDERS)
@pytest.mark.parametrize("visc", tn.VISCOSITIES)
@pytest.mark.parametrize("layout", list(tn.LAYOUTS))
def test_bc_matrix(gpu, layout, visc, maxorder):
    worst = [0.0, 0.0]
    for bc in tn.BC_SETS:
        dev = Dev(gpu, tn.case(layout, visc, bc["name"], maxorder))
        dev.apply()
        d = check_apply(dev, (layout, visc, bc["name"], maxorder))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print(f"\n[tensor gpu/ref] {layout} {visc} maxorder {maxorder}: y {worst[0]:.2e} ghost {worst[1]:.2e}")


@pytest.mark.parametrize("visc", tn.VISCOSITIES)
def test_three_different_cell_sizes(gpu, visc):
    """h = (1/20, 1/24, 1/40): no two directions can be swapped unnoticed"""
    worst = [0.0, 0.0]
    for bc in tn.BC_SETS:
        dev = Dev(gpu, tn.case(tn.TILE_LAYOUTS[0], visc, bc["name"], 3, "explicit", tn.PROB_HI_ANISO))
        dev.apply()
        d = check_apply(dev, (visc, bc["name"]))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print(f"\n[tensor gpu/ref] three cell sizes {visc}: y {worst[0]:.2e} ghost {worst[1]:.2e}")


WALL_CASE = {tn.TILE_LAYOUTS[0]: ("yhi-symmetry", 3), tn.TILE_LAYOUTS[1]: ("xlo-slip", 2)}


def _forms(gpu, layout, visc, tag):
    """apply without and with the a-term (HASA), and the residual rhs - A u on the ghost cells the apply left (RES)"""
    bcname, mo = WALL_CASE[layout]
    worst = 0.0
    for form in tn.FORMS:
        cs = tn.case(layout, visc, bcname, mo, form)
        dev = Dev(gpu, cs)
        dev.apply()
        dy, _ = check_apply(dev, (tag, layout, visc, form))
        rng = np.random.default_rng(17)
        rhs = np.asfortranarray(float(np.abs(cs["y"]).max()) * rng.standard_normal(tuple(cs["n"]) + (3,)))
        rhs_d = gpu.MultiFab(dev.lay, gpu.CELL, 3, 0); rhs_d.set_from_global(rhs, (0, 0, 0))
        dev.out.setval(SENTINEL)
        gpu.abec_residual(dev.g, cs["a"], cs["b"], dev.acoef, dev.eta, dev.out, dev.vel, rhs=rhs_d, tensor=1)
        dr, _ = check_apply(dev, (tag, layout, visc, form, "residual"), y_ref=rhs.astype(tn.LD) - cs["y"])
        worst = max(worst, dy, dr)
    return worst


@pytest.mark.parametrize("visc", tn.VISCOSITIES)
@pytest.mark.parametrize("layout", tn.TILE_LAYOUTS)
def test_forms(gpu, layout, visc):
    w = _forms(gpu, layout, visc, "default")
    print(f"\n[tensor gpu/ref] forms {layout} {visc}: y {w:.2e}")


@pytest.mark.parametrize("layout", tn.TILE_LAYOUTS)
def test_tile_shapes_and_face_flux_form(gpu, layout):
    """constant viscosity: TENSOR_UNI_CC 1..5 are the tile shapes of k_tensor_uni, 0 the fused face-flux form (k_tensor_cross_zm);
    TENSOR_UNI_KC the planes of a z-chunk; TENSOR_FUSED = 0 the 7-point kernel followed by the cross terms"""
    lib = gpu
    cc_old, fused_old, kc_old = lib.tuning_get("TENSOR_UNI_CC", 1), lib.tuning_get("TENSOR_FUSED", 1), lib.tuning_get("TENSOR_UNI_KC", 0)
    try:
        for cc in range(6):
            lib.tuning_set("TENSOR_UNI_CC", cc)
            w = _forms(gpu, layout, "constant", f"TENSOR_UNI_CC={cc}")
            print(f"\n[tensor gpu/ref] TENSOR_UNI_CC={cc} {layout}: y {w:.2e}")
        lib.tuning_set("TENSOR_UNI_CC", cc_old)
        for kc in (1, 3):                # z-chunks of one plane (no plane fetched ahead), and of a length that divides neither 8 nor 10
            lib.tuning_set("TENSOR_UNI_KC", kc)
            w = _forms(gpu, layout, "constant", f"TENSOR_UNI_KC={kc}")
            print(f"\n[tensor gpu/ref] TENSOR_UNI_KC={kc} {layout}: y {w:.2e}")
        lib.tuning_set("TENSOR_UNI_KC", kc_old)
        lib.tuning_set("TENSOR_FUSED", 0)
        w = _forms(gpu, layout, "constant", "TENSOR_FUSED=0")
        print(f"\n[tensor gpu/ref] TENSOR_FUSED=0 {layout}: y {w:.2e}")
    finally:
        lib.tuning_set("TENSOR_UNI_CC", cc_old)
        lib.tuning_set("TENSOR_UNI_KC", kc_old)
        lib.tuning_set("TENSOR_FUSED", fused_old)


@pytest.mark.parametrize("visc", tn.VISCOSITIES)
@pytest.mark.parametrize("layout", tn.TILE_LAYOUTS)
def test_extensive_flux(gpu, layout, visc):
    """all three directions and components on the velocity the operator left; add on top of a flux that is not zero; fac scales"""
    from iamr_amd import ns as N
    lib = gpu
    bcname, mo = WALL_CASE[layout]
    cs = tn.case(layout, visc, bcname, mo)
    dev = Dev(gpu, cs)
    dev.apply()
    flux = [lib.MultiFab(dev.lay, lib.face(d), 3, 0) for d in range(3)]
    for f in flux:
        f.setval(SENTINEL)

    def distance(factor, tag):
        w = 0.0
        for d in range(3):
            ref = tn.LD(factor) * cs["flux"][d]
            dd = box_distance(flux[d], ref, (0, 0, 0), (tag, d)) / float(np.abs(ref).max())
            assert dd <= FLUX_BAR, (layout, visc, tag, d, dd)
            w = max(w, dd)
        return w
    N.tensor_extensive_flux(dev.g, dev.vel, dev.eta, flux, 1.0)
    w = distance(1.0, "fac 1")
    N.tensor_extensive_flux(dev.g, dev.vel, dev.eta, flux, 0.5, add=True)
    w = max(w, distance(1.5, "add 0.5"))
    N.tensor_extensive_flux(dev.g, dev.vel, dev.eta, flux, -2.0)
    w = max(w, distance(-2.0, "fac -2"))
    print(f"\n[tensor gpu/ref] flux {layout} {visc}: {w:.2e}")
