"""CPU suite: how a smoothing call and the bottom solve of the nodal multigrid run on a level (nodal_smooth_plan through the host-only query
iamrx_host_nodal_smoother_plan), pinned at the smallest shapes that separate the paths.  One box spanning the domain unless boxes are given;
ghost widths as the solver allocates them.  The expected values are the conditions of NodalMG before the plan existed, read term by term."""
import pytest

NEUMANN, DIRICHLET = 102, 101
WALLS, X_PERIODIC = (0, 0, 0), (1, 0, 0)
OUTFLOW = dict(per=WALLS, bc=NEUMANN, hibc=(DIRICHLET, NEUMANN, NEUMANN), has_mask=True)       # one Dirichlet (outflow) face: the level has a mask


def two(nx, ny, nz):
    """two boxes side by side in x"""
    return dict(boxes=[((0, 0, 0), (nx - 1, ny - 1, nz - 1)), ((nx, 0, 0), (2 * nx - 1, ny - 1, nz - 1))])


# name: (domain, query arguments, tuning keys and the value they are set to, expected fields)
TABLE = {
    "48^3 periodic": ((48,) * 3, {}, {}, dict(path="GSR", ngrow=4, wrap=1, refl=0, images=1, zero_start=1, written_first=1, splits=0, bottom="NONE")),
    "32^3 periodic: below GSR_MIN": ((32,) * 3, {}, {}, dict(path="GS4", ngrow=4, wrap=1, images=1, zero_start=0, written_first=0)),
    "48 x 47 x 48 periodic": ((48, 47, 48), {}, {}, dict(path="GS4", wrap=1)),
    "GSR = 0": ((48,) * 3, {}, dict(GSR=0), dict(path="GS4", wrap=1, images=1, zero_start=0, written_first=0)),
    "GSR_MIN = 32": ((32,) * 3, {}, dict(GSR_MIN=32), dict(path="GSR", zero_start=1, written_first=1)),
    "Neumann walls": ((48,) * 3, dict(per=WALLS, bc=NEUMANN), {}, dict(path="GSR", wrap=1, refl=7, images=1, written_first=1)),
    "periodic in x, walls in y and z": ((48,) * 3, dict(per=X_PERIODIC, bc=NEUMANN), {}, dict(path="GSR", wrap=1, refl=6)),
    "NODAL_REFLECT_WRAP = 0, walls": ((48,) * 3, dict(per=WALLS, bc=NEUMANN), dict(NODAL_REFLECT_WRAP=0),
                                      dict(path="GSR", wrap=0, refl=0, images=0, written_first=0, zero_start=1)),
    "NODAL_REFLECT_WRAP = 0, periodic": ((48,) * 3, {}, dict(NODAL_REFLECT_WRAP=0), dict(wrap=1, images=1)),
    "PERIODIC_WRAP = 0, periodic": ((48,) * 3, {}, dict(PERIODIC_WRAP=0), dict(path="GSR", wrap=0, images=0, written_first=0)),
    "PERIODIC_WRAP = 0, walls": ((48,) * 3, dict(per=WALLS, bc=NEUMANN), dict(PERIODIC_WRAP=0), dict(path="GSR", wrap=0, refl=0, images=0)),
    "3 cells in z": ((48, 48, 3), {}, {}, dict(path="GSR", wrap=0, images=0)),
    "outflow face": ((48,) * 3, OUTFLOW, {}, dict(path="GSR", wrap=0, refl=0, images=0, written_first=0, zero_start=1)),
    "outflow face, NODAL_ZERO_START = 2": ((48,) * 3, OUTFLOW, dict(NODAL_ZERO_START=2), dict(path="GSR", zero_start=0)),
    "outflow face, right-hand side of another width": ((48,) * 3, dict(ngrow=(4, 3), **OUTFLOW), {}, dict(path="GS4", zero_start=0)),
    "NODAL_ZERO_START = 2, periodic": ((48,) * 3, {}, dict(NODAL_ZERO_START=2), dict(zero_start=1)),
    "NODAL_ZERO_START = 0": ((48,) * 3, {}, dict(NODAL_ZERO_START=0), dict(path="GSR", zero_start=0)),
    "NODAL_IMAGE_READERS = 0": ((48,) * 3, {}, dict(NODAL_IMAGE_READERS=0), dict(wrap=1, images=0, written_first=1)),
    "NODAL_SKIP_FILLS = 0": ((48,) * 3, {}, dict(NODAL_SKIP_FILLS=0), dict(wrap=1, images=1, written_first=0)),
    "NODAL_FUSED = 0": ((48,) * 3, {}, dict(NODAL_FUSED=0), dict(path="COLOUR8", ngrow=1, wrap=0, images=0, written_first=0, zero_start=0, splits=0)),
    "Jacobi": ((48,) * 3, dict(nodal_smoother=2), {}, dict(path="JACOBI", ngrow=4, wrap=0, images=0, written_first=0, zero_start=0)),
    "8^3 periodic": ((8,) * 3, {}, {}, dict(path="SMALL", images=1, zero_start=0, bottom="NONE")),
    "8^3 periodic, NODAL_SMALL = 0": ((8,) * 3, {}, dict(NODAL_SMALL=0), dict(path="GS4", wrap=1)),
    "8^3 periodic, NODAL_FUSED = 0": ((8,) * 3, {}, dict(NODAL_FUSED=0), dict(path="SMALL", ngrow=1, images=0)),
    "8^3 with walls": ((8,) * 3, dict(per=WALLS, bc=NEUMANN), {}, dict(path="GS4", wrap=1, refl=7)),
    "8^3 with a mask": ((8,) * 3, dict(has_mask=True), {}, dict(path="GS4", wrap=0)),
    "640 cells": ((10, 8, 8), {}, {}, dict(path="GS4", wrap=1)),
    "an odd length": ((6, 6, 7), {}, {}, dict(path="GS4", wrap=1)),
    "two boxes of 112 x 112 x 16": ((224, 112, 16), two(112, 112, 16), {}, dict(path="GSR", wrap=0, images=0, written_first=0, zero_start=1, par_fill=1, splits=1)),
    "two boxes of 104 x 104 x 16: two tiles of 56": ((208, 104, 16), two(104, 104, 16), {}, dict(path="GSR", wrap=0, splits=0)),
    "two boxes of 112 x 112 x 8": ((224, 112, 8), two(112, 112, 8), {}, dict(path="GSR", wrap=0, splits=0)),
    "two boxes, NODAL_PARITY_FILL = 0: in one piece": ((224, 112, 16), two(112, 112, 16), dict(NODAL_PARITY_FILL=0), dict(path="GSR", par_fill=0, splits=0)),
    "two boxes, GSR = 0": ((224, 112, 16), two(112, 112, 16), dict(GSR=0), dict(path="GS4", splits=0, zero_start=0)),
    "coarsest 8^3 periodic": ((8,) * 3, dict(coarsest=True), {}, dict(path="SMALL", bottom="DEVICE_PERIODIC")),
    "coarsest 8 x 8 x 16 periodic": ((8, 8, 16), dict(coarsest=True), {}, dict(bottom="HOST_KRYLOV")),
    "coarsest 8^3 with walls": ((8,) * 3, dict(coarsest=True, per=WALLS, bc=NEUMANN), {}, dict(bottom="DEVICE_GENERAL")),
    "coarsest 8^3 periodic with a mask": ((8,) * 3, dict(coarsest=True, has_mask=True), {}, dict(bottom="DEVICE_GENERAL")),
    "coarsest 9 x 8 x 8 with walls": ((9, 8, 8), dict(coarsest=True, per=WALLS, bc=NEUMANN), {}, dict(bottom="HOST_KRYLOV")),
    "coarsest, MG_DEVICE_BOTTOM = 0": ((8,) * 3, dict(coarsest=True), dict(MG_DEVICE_BOTTOM=0), dict(bottom="HOST_KRYLOV")),
    "coarsest, MG_DEVICE_BOTTOM_GENERAL = 0, walls": ((8,) * 3, dict(coarsest=True, per=WALLS, bc=NEUMANN), dict(MG_DEVICE_BOTTOM_GENERAL=0),
                                                      dict(bottom="HOST_KRYLOV")),
    "coarsest, MG_DEVICE_BOTTOM_GENERAL = 0, periodic": ((8,) * 3, dict(coarsest=True), dict(MG_DEVICE_BOTTOM_GENERAL=0), dict(bottom="DEVICE_PERIODIC")),
    "coarsest, smoother only": ((8,) * 3, dict(coarsest=True, bottom_smoother_only=True), {}, dict(bottom="SMOOTHER_ONLY")),
    "coarsest, device_bottom off": ((8,) * 3, dict(coarsest=True, device_bottom=False), {}, dict(bottom="HOST_KRYLOV")),
    "coarsest, Jacobi with device_bottom": ((8,) * 3, dict(coarsest=True, nodal_smoother=2), {}, dict(path="JACOBI", bottom="HOST_KRYLOV")),
    "four sweeps": ((48,) * 3, dict(nodal_sweeps=4), {}, dict(sweeps=4)),
}


def plan(lib, n, boxes=None, per=(1, 1, 1), bc=0, hibc=None, **kw):
    lobc = tuple(0 if per[d] else bc for d in range(3))
    boxes = boxes or [((0, 0, 0), tuple(v - 1 for v in n))]
    g = lib.Geom.make(n, periodic=per)
    if "ngrow" not in kw:      # what the solver allocates
        kw["ngrow"] = (lib.host_nodal_smoother_plan(g, boxes)["ngrow"],) * 2
    return lib.host_nodal_smoother_plan(g, boxes, lobc=lobc, hibc=hibc or lobc, **kw)


@pytest.mark.parametrize("name", list(TABLE))
def test_nodal_smoother_plan_of_a_level(name):
    from iamr_amd import lib
    n, args, keys, expect = TABLE[name]
    old = {k: lib.tuning_get(k, 48 if k == "GSR_MIN" else 1) for k in keys}
    for k, v in keys.items():
        lib.tuning_set(k, v)
    try:
        got = plan(lib, n, **args)
    finally:
        for k, v in old.items():
            lib.tuning_set(k, v)
    assert {k: got[k] for k in expect} == expect, got


def test_plan_is_made_anew_for_every_query():
    """nothing is cached beyond the call: a key flipped between two queries shows in the second"""
    from iamr_amd import lib
    assert plan(lib, (48,) * 3)["path"] == "GSR"
    lib.tuning_set("GSR", 0)
    try:
        assert plan(lib, (48,) * 3)["path"] == "GS4"
    finally:
        lib.tuning_set("GSR", 1)
    assert plan(lib, (48,) * 3)["path"] == "GSR"
