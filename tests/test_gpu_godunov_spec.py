"""GPU: the specialised instantiations of the fused Godunov kernels (k_god_z / k_pred_z with the launch-uniform flags as template
parameters, tuning key GODUNOV_SPEC, iamr_amd/csrc/k_godunov.hip) against the multi-pass kernels (GODUNOV_Z = 0) and against the run-time
fused kernels (GODUNOV_SPEC = 0) through the C-ABI on the same device data, to 1e-13 relative to the field's maximum (the bar of
tests/test_gpu_godunov_fused.py: FMA contraction may differ between instruction streams).

A box of 20 x 18 x 20 cells holds a full 14 x 14 tile and partial tiles 6 wide and 4 tall; GODUNOV_ZKC = 8 marches it in three z-chunks;
the two-box layout splits it in z (12 + 8 planes; arrays made through the C-ABI keep the caller's boxes, only level objects merge).
Every case of the matrix -- periodic / walls on every side, forcing absent / late / early, divu absent / non-zero, no outputs / fluxes /
edge states and fluxes -- runs an all-convective, an all-conservative and a mixed component list and asserts from the library's launch counters which kernel ran: a
specialised one per form of the components where the flags have an instantiation (late forcing, no edge states), the run-time
kernel otherwise.  aofs carries a sentinel in a component no launch may touch and a second sentinel in the components every launch must
write, so a component the table loses or names twice is seen.

Sensitivity (scratch mutations of k_godunov.hip, each run against this file on an MI355X):
  the entries of the convective and of the conservative component table swapped (cv.c[0] <-> cs.c[0])   -> 16 of 92 tests fail
  the conservative body selected for the convective components (launch <.., CNS = 1> for both tables)   -> 16 of 92 tests fail
(a swap of two entries INSIDE one table only changes which workgroup computes which component and is value-neutral by construction).
"""
import numpy as np
import pytest

from test_gpu_godunov_fused import smooth, close, REFLECT_ODD, INT_DIR, REFLECT_EVEN, FOEXTRAP, EXT_DIR, HOEXTRAP, PER_BC5

pytestmark = pytest.mark.gpu

N = (20, 18, 20)
# walls on every side, every BC type the wall kernel covers on some face of some component
WALL6_BC5 = [((EXT_DIR, HOEXTRAP, EXT_DIR), (EXT_DIR, FOEXTRAP, HOEXTRAP)),
             ((EXT_DIR, EXT_DIR, HOEXTRAP), (HOEXTRAP, EXT_DIR, EXT_DIR)),
             ((REFLECT_EVEN, REFLECT_ODD, EXT_DIR), (FOEXTRAP, REFLECT_EVEN, EXT_DIR)),
             ((FOEXTRAP, REFLECT_EVEN, FOEXTRAP), (EXT_DIR, HOEXTRAP, REFLECT_EVEN)),
             ((HOEXTRAP, FOEXTRAP, REFLECT_ODD), (REFLECT_ODD, EXT_DIR, FOEXTRAP))]
COMP_LISTS = {"conv": (0, 0, 0, 0, 0), "cons": (1, 1, 1, 1, 1), "mixed": (0, 0, 0, 1, 0)}
COUNTERS = ("GODUNOV_Z_SPEC_CONV_LAUNCHES", "GODUNOV_Z_SPEC_CONS_LAUNCHES", "GODUNOV_Z_RUNTIME_LAUNCHES",
            "PRED_Z_SPEC_LAUNCHES", "PRED_Z_RUNTIME_LAUNCHES")


class tuning:
    """set tuning keys for a block, restore them afterwards"""

    def __init__(self, lib, **kv):
        self.lib, self.kv = lib, kv

    def __enter__(self):
        self.old = {k: self.lib.tuning_get(k, d) for k, d in (("GODUNOV_Z", 1), ("GODUNOV_SPEC", 1), ("GODUNOV_ZKC", 0))
                    if k in self.kv}
        for k, v in self.kv.items():
            self.lib.tuning_set(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.lib.tuning_set(k, v)


def counters(lib):
    return np.array([lib.tuning_get(k, 0) for k in COUNTERS])


_inputs = {}


def inputs(lib, walls, two_boxes):
    """geometry, layout and the device fields of a (BC, layout) pair: built once, read only"""
    key = (walls, two_boxes)
    if key in _inputs:
        return _inputs[key]
    periodic = (0, 0, 0) if walls else (1, 1, 1)
    bc5 = WALL6_BC5 if walls else PER_BC5
    g = lib.Geom.make(N, periodic=periodic)
    lay = (lib.Layout([((0, 0, 0), (N[0] - 1, N[1] - 1, 11)), ((0, 0, 12), (N[0] - 1, N[1] - 1, N[2] - 1))]) if two_boxes
           else lib.Layout.single(N))
    S = lib.MultiFab(lay, lib.CELL, 5, 3)
    S.set_from_global(np.stack([(1.5 if c >= 3 else 0.0) + smooth(N, 3, 10 + c) for c in range(5)], axis=-1), (-3, -3, -3))
    S.fill_boundary(g)
    if walls:
        S.fill_physbc(g, bc5, [[0.1 * (c + 1)] * 3 for c in range(5)], [[-0.05 * (c + 1)] * 3 for c in range(5)])
    frc = lib.MultiFab(lay, lib.CELL, 5, 1)
    frc.set_from_global(np.stack([2.0 * smooth(N, 1, 30 + c) for c in range(5)], axis=-1), (-1, -1, -1))
    divu = lib.MultiFab(lay, lib.CELL, 1, 1)
    divu.set_from_global(0.3 * smooth(N, 1, 50)[..., None], (-1, -1, -1))
    zero = lib.MultiFab(lay, lib.CELL, 1, 1)
    zero.setval(0.0)
    mac = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 1)
        m.set_from_global(smooth(N, 1, 70 + d, lib.face(d))[..., None], (-1, -1, -1))
        mac.append(m)
    _inputs[key] = (g, lay, bc5, S, frc, divu, zero, mac)
    return _inputs[key]


def advect(lib, inp, iconserv, force, fit, divu, out, **keys):
    """one godunov_compute_aofs call under the tuning keys: (aofs, edges, fluxes) as global arrays and the launch counters it moved"""
    g, lay, bc5, S, frc, _dv, _zero, mac = inp
    aofs = lib.MultiFab(lay, lib.CELL, 6, 0)
    aofs.setval(-7.0)
    edge = [lib.MultiFab(lay, lib.face(d), 5, 0) for d in range(3)] if out == "edge+flux" else None
    flux = [lib.MultiFab(lay, lib.face(d), 5, 0) for d in range(3)] if out != "none" else None
    for m in (edge or []) + (flux or []):
        m.setval(-9.0)
    c0 = counters(lib)
    with tuning(lib, GODUNOV_ZKC=8, **keys):
        lib.godunov_compute_aofs(g, aofs, 1, S, 5, frc if force else None, divu, mac, iconserv, 0.4 / max(N), bc5, 1, fit, edge=edge, flux=flux)
    dc = counters(lib) - c0
    return aofs.gather_valid(N), [e.gather_valid(N) for e in edge or []], [f.gather_valid(N) for f in flux or []], dc


def compare(a, b, tag):
    close(a[0], b[0], (tag, "aofs"))
    for d in range(len(a[1])):
        close(a[1][d], b[1][d], (tag, "edge", d))
    for d in range(len(a[2])):
        close(a[2][d], b[2][d], (tag, "flux", d))


@pytest.mark.parametrize("out", ["none", "flux", "edge+flux"])
@pytest.mark.parametrize("with_divu", [False, True], ids=["nodivu", "divu"])
@pytest.mark.parametrize("forcing", ["noforce", "late", "early"])
@pytest.mark.parametrize("two_boxes", [False, True], ids=["1box", "2boxes"])
@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "walls"])
def test_specialised_advection(gpu, walls, two_boxes, forcing, with_divu, out):
    lib = gpu
    inp = inputs(lib, walls, two_boxes)
    force, fit = forcing != "noforce", 1 if forcing == "early" else 0
    divu = inp[5] if with_divu else None
    has_inst = forcing == "late" and out != "edge+flux"
    for name, ic in COMP_LISTS.items():
        ref = advect(lib, inp, ic, force, fit, divu, out, GODUNOV_Z=0)
        rt = advect(lib, inp, ic, force, fit, divu, out, GODUNOV_SPEC=0)
        sp = advect(lib, inp, ic, force, fit, divu, out, GODUNOV_SPEC=1)
        print(name, "counters ref/rt/spec", ref[3], rt[3], sp[3])
        assert list(ref[3][:3]) == [0, 0, 0] and list(rt[3][:3]) == [0, 0, 1]
        if has_inst:
            assert list(sp[3][:3]) == [1 if 0 in ic else 0, 1 if 1 in ic else 0, 0], name
        else:
            assert list(sp[3][:3]) == [0, 0, 1], name
        for r in (rt, sp):
            assert np.all(r[0][..., 0] == -7.0), name               # acomp offset respected
            assert not np.any(r[0][..., 1:] == -7.0), name          # every component of every cell written
            for m in r[1] + r[2]:
                assert not np.any(m == -9.0), name                  # every face of every component written
        compare(sp, ref, (name, "spec vs multi-pass"))
        compare(sp, rt, (name, "spec vs run-time"))


@pytest.mark.parametrize("forcing", ["noforce", "late", "early"])
@pytest.mark.parametrize("two_boxes", [False, True], ids=["1box", "2boxes"])
@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "walls"])
def test_specialised_prediction(gpu, walls, two_boxes, forcing):
    lib = gpu
    g, lay, bc5, S, frc, _dv, _zero, _mac = inputs(lib, walls, two_boxes)
    fit = 1 if forcing == "early" else 0
    res = {}
    for tag, keys in (("ref", {"GODUNOV_Z": 0}), ("rt", {"GODUNOV_SPEC": 0}), ("spec", {"GODUNOV_SPEC": 1})):
        um = [lib.MultiFab(lay, lib.face(d), 1, 1) for d in range(3)]
        for m in um:
            m.setval(-9.0)
        c0 = counters(lib)
        with tuning(lib, GODUNOV_ZKC=8, **keys):
            lib.godunov_extrap_vel_to_faces(g, S, frc if forcing != "noforce" else None, um, 0.4 / max(N), bc5[:3], fit)
        res[tag] = ([m.gather_valid(N) for m in um], counters(lib) - c0)
        print(tag, "counters", res[tag][1])
    assert list(res["ref"][1][3:]) == [0, 0] and list(res["rt"][1][3:]) == [0, 1]
    assert list(res["spec"][1][3:]) == ([1, 0] if forcing == "late" else [0, 1])
    for d in range(3):
        assert not np.any(res["spec"][0][d] == -9.0)
        close(res["spec"][0][d], res["ref"][0][d], ("umac spec vs multi-pass", d))
        close(res["spec"][0][d], res["rt"][0][d], ("umac spec vs run-time", d))


@pytest.mark.parametrize("spec", [0, 1], ids=["runtime", "spec"])
@pytest.mark.parametrize("two_boxes", [False, True], ids=["1box", "2boxes"])
@pytest.mark.parametrize("walls", [False, True], ids=["periodic", "walls"])
def test_no_divu_equals_zero_divu(gpu, walls, two_boxes, spec):
    """divu absent against a divu array of zeros: every term dropped is a product with 0.0, so the values are equal (np.array_equal treats
    +0 and -0 as equal)"""
    lib = gpu
    inp = inputs(lib, walls, two_boxes)
    for name, ic in COMP_LISTS.items():
        a = advect(lib, inp, ic, True, 0, None, "edge+flux" if spec == 0 else "flux", GODUNOV_SPEC=spec)
        b = advect(lib, inp, ic, True, 0, inp[6], "edge+flux" if spec == 0 else "flux", GODUNOV_SPEC=spec)
        for r in (a, b):                                                # both calls: the specialised kernels / the run-time kernel
            assert (r[3][2] == 0 and r[3][0] + r[3][1] >= 1) if spec else list(r[3][:3]) == [0, 0, 1], name
        assert np.array_equal(a[0], b[0]), (name, "aofs")
        for x, y in zip(a[1] + a[2], b[1] + b[2]):
            assert np.array_equal(x, y), name
