"""GPU: the forms of the nodal transfer operators and of the nodal divergence behind their run-time switches write the same doubles.

Restriction (IAMRX_NODAL_RESTRICT_TILE 1 against 0) and interpolation (IAMRX_NODAL_INTERP_LDS 1 against 0) on boxes that are no
multiple of the kernels' tiles -- one periodic box, two boxes kept side by side, one box with mirrored sigma ghosts (Neumann walls) -- and
the divergence (IAMRX_NODAL_DIVU_ZM 1 against 0) with a wall and an inflow face in every direction.  Whole arrays are compared, ghost
layers included.  The old divergence is pinned to the oracle by tests/test_gpu_ns.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEUMANN, INFLOW = 102, 103


def _whole(mf):
    return [mf.to_numpy(li)[0].copy() for li in range(mf.nlocal())]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _fine_coarse_layouts(lib, boxes):
    fine = lib.Layout(boxes)
    crse = lib.Layout([(tuple(v // 2 for v in lo), tuple((v + 1) // 2 - 1 for v in hi)) for lo, hi in boxes])
    return fine, crse


# fine boxes: none is a multiple of the 64 x 16 x 8 fine-node footprint of a 32 x 8 coarse tile or of the 32 x 8 x 8 interpolation tile
ONE_BOX = [((0, 0, 0), (47, 23, 19))]
TWO_BOXES = [((0, 0, 0), (31, 15, 15)), ((32, 0, 0), (63, 15, 15))]
TALL_BOX = [((0, 0, 0), (39, 23, 135))]      # 69 coarse node planes: the 8-plane z-chunks of the restriction
SMALL_BOX = [((0, 0, 0), (23, 15, 11))]      # 12 x 8 x 6 coarse cells: below the tile kernels' threshold
WIDE_BOX = [((0, 0, 0), (99, 17, 11))]       # 50 coarse cells in x: the tiled restriction takes it without being asked


def _domain(boxes):
    return tuple(max(hi[d] for _, hi in boxes) + 1 for d in range(3))


def _random_nodes(lib, lay, n, rng, ng):
    m = lib.MultiFab(lay, lib.NODE, 1, ng)
    m.set_from_global(rng.standard_normal(tuple(v + 1 + 2 * ng for v in n) + (1,)), (-ng,) * 3)
    return m


def _restrict_forms(lib, boxes, seed, min_x=16):
    """min_x: the tiled form takes levels of at least so many coarse cells in x (48 unless told otherwise; the small shapes here ask for 16)"""
    from iamr_amd import ns as N
    rng = np.random.default_rng(seed)
    flay, clay = _fine_coarse_layouts(lib, boxes)
    n = _domain(boxes)
    fine = _random_nodes(lib, flay, n, rng, 1)
    start = rng.standard_normal(tuple(v // 2 + 3 for v in n) + (1,))
    out = {}
    lib.tuning_set("NODAL_RESTRICT_MIN", min_x)
    for form in (0, 1):
        lib.tuning_set("NODAL_RESTRICT_TILE", form)
        crse = lib.MultiFab(clay, lib.NODE, 1, 1)
        crse.set_from_global(start, (-1, -1, -1))
        N.nodal_restrict(crse, fine)
        lib.sync()
        out[form] = _whole(crse)
    lib.tuning_set("NODAL_RESTRICT_TILE", 1)
    lib.tuning_set("NODAL_RESTRICT_MIN", 48)
    return out, fine, start


@pytest.mark.parametrize("boxes", [ONE_BOX, TALL_BOX, SMALL_BOX], ids=["48x24x20", "40x24x136", "24x16x12"])
def test_restriction_forms_write_the_same_doubles(gpu, boxes):
    out, fine, start = _restrict_forms(gpu, boxes, 11)
    assert _same(out[0], out[1])
    # full weighting (1, 2, 1)^3 / 64 in numpy: 27 terms of size O(1), so 1e-13 is hundreds of roundings; the ghost layer keeps its data
    f = fine.to_numpy(0)[0][..., 0]
    c = out[1][0][..., 0]
    ref = np.zeros(tuple(v - 2 for v in c.shape))
    for dk in range(3):
        for dj in range(3):
            for di in range(3):
                w = (2.0 if di == 1 else 1.0) * (2.0 if dj == 1 else 1.0) * (2.0 if dk == 1 else 1.0)
                ref += w * f[di:f.shape[0] - 2 + di:2, dj:f.shape[1] - 2 + dj:2, dk:f.shape[2] - 2 + dk:2]
    assert np.abs(c[1:-1, 1:-1, 1:-1] - ref / 64.0).max() <= 1e-13
    assert np.array_equal(c[0], start[0, :, :, 0]) and np.array_equal(c[:, :, -1], start[:, :, -1, 0])


def test_restriction_forms_at_the_default_threshold(gpu):
    out, _, _ = _restrict_forms(gpu, WIDE_BOX, 13, min_x=48)
    assert _same(out[0], out[1])


@pytest.mark.boxes_kept
def test_restriction_forms_on_two_boxes(gpu):
    out, _, _ = _restrict_forms(gpu, TWO_BOXES, 12)
    assert len(out[0]) == 2 and np.isfinite(out[1][1]).all() and _same(out[0], out[1])


def _divu_forms(lib, n, per, lobc, hibc, seed, ncomp=3, vcomp=0):
    from iamr_amd import ns as N
    rng = np.random.default_rng(seed)
    g = lib.Geom.make(n, periodic=per)
    lay = lib.Layout.single(n)
    vel = lib.MultiFab(lay, lib.CELL, ncomp, 1)
    vel.set_from_global(rng.standard_normal(tuple(v + 2 for v in n) + (ncomp,)), (-1, -1, -1))
    out = {}
    for form in (0, 1):
        lib.tuning_set("NODAL_DIVU_ZM", form)
        rhs = lib.MultiFab(lay, lib.NODE, 1, 1)
        rhs.setval(7.0)
        N.nodal_divu(g, rhs, vel, vcomp, lobc, hibc)
        lib.sync()
        out[form] = _whole(rhs)
    lib.tuning_set("NODAL_DIVU_ZM", 1)
    return out


def _face_cases():
    cases = [("periodic", (1, 1, 1), (0, 0, 0), (0, 0, 0))]
    for d in range(3):
        for lo, hi, tag in ((NEUMANN, INFLOW, "wall-inflow"), (INFLOW, NEUMANN, "inflow-wall")):
            per = [1, 1, 1]; per[d] = 0
            lobc = [0, 0, 0]; lobc[d] = lo
            hibc = [0, 0, 0]; hibc[d] = hi
            cases.append((f"{'xyz'[d]}-{tag}", tuple(per), tuple(lobc), tuple(hibc)))
    cases.append(("walls-and-inflow-everywhere", (0, 0, 0), (NEUMANN, INFLOW, NEUMANN), (INFLOW, NEUMANN, INFLOW)))
    return cases


@pytest.mark.parametrize("tag,per,lobc,hibc", _face_cases(), ids=[c[0] for c in _face_cases()])
def test_divergence_forms_write_the_same_doubles(gpu, tag, per, lobc, hibc):
    out = _divu_forms(gpu, (40, 24, 20), per, lobc, hibc, 21)
    a = out[0][0]
    assert np.isfinite(a).all() and np.array_equal(a[0], np.full_like(a[0], 7.0))        # ghost nodes are not touched
    assert np.abs(a[1:-1, 1:-1, 1:-1]).max() > 1.0
    assert _same(out[0], out[1])


def test_divergence_forms_in_z_chunks_and_inside_a_state(gpu):
    """36 cells in z: three 16-plane chunks per tile column; velocity at components 1 .. 3 of a five-component array"""
    out = _divu_forms(gpu, (40, 24, 36), (1, 0, 1), (0, NEUMANN, 0), (0, INFLOW, 0), 22, ncomp=5, vcomp=1)
    assert _same(out[0], out[1])
    small = _divu_forms(gpu, (12, 8, 8), (0, 1, 1), (INFLOW, 0, 0), (NEUMANN, 0, 0), 23)       # below the tile kernel's threshold
    assert _same(small[0], small[1])


def _interp_forms(lib, boxes, seed, walls=False):
    """fine += interpolated coarse data by the two forms, on the same random data; sigma's ghost cells are random (periodic or neighbour
    data of some kind) or, with walls, the mirror image of the first interior cells"""
    from iamr_amd import ns as N
    rng = np.random.default_rng(seed)
    flay, clay = _fine_coarse_layouts(lib, boxes)
    n = _domain(boxes)
    S = 0.5 + rng.random(tuple(v + 2 for v in n) + (1,))
    if walls:
        S[0], S[-1] = S[1], S[-2]
        S[:, 0], S[:, -1] = S[:, 1], S[:, -2]
        S[:, :, 0], S[:, :, -1] = S[:, :, 1], S[:, :, -2]
    sig = lib.MultiFab(flay, lib.CELL, 1, 1)
    sig.set_from_global(S, (-1, -1, -1))
    crse = _random_nodes(lib, clay, tuple(v // 2 for v in n), rng, 1)
    start = rng.standard_normal(tuple(v + 3 for v in n) + (1,))
    out = {}
    for form in (0, 1):
        lib.tuning_set("NODAL_INTERP_LDS", form)
        fine = lib.MultiFab(flay, lib.NODE, 1, 1)
        fine.set_from_global(start, (-1, -1, -1))          # the kernel adds: the target starts non-zero
        N.nodal_interp_add(fine, crse, sig)
        lib.sync()
        out[form] = _whole(fine)
    lib.tuning_set("NODAL_INTERP_LDS", 1)
    return out, start


@pytest.mark.parametrize("boxes,walls", [(ONE_BOX, False), (ONE_BOX, True), (TALL_BOX, False), (WIDE_BOX, True)],
                         ids=["48x24x20-periodic", "48x24x20-walls", "40x24x136", "100x18x12-walls"])
def test_interpolation_forms_write_the_same_doubles(gpu, boxes, walls):
    out, start = _interp_forms(gpu, boxes, 31, walls)
    a = out[0][0]
    assert np.isfinite(a).all() and np.array_equal(a[0], start[0]) and np.array_equal(a[:, :, -1], start[:, :, -1])       # ghost nodes keep their data
    assert np.count_nonzero(a[1:-1, 1:-1, 1:-1] != start[1:-1, 1:-1, 1:-1]) > 0.99 * a[1:-1, 1:-1, 1:-1].size
    assert _same(out[0], out[1])


@pytest.mark.boxes_kept
def test_interpolation_forms_on_two_boxes(gpu):
    out, _ = _interp_forms(gpu, TWO_BOXES, 32)
    assert len(out[0]) == 2 and np.isfinite(out[1][1]).all()
    assert _same(out[0], out[1])
