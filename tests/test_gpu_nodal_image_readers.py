"""GPU: the image-reading forms of the nodal residual and restriction, and the nodal multigrid without its per-cycle ghost fills
(IAMRX_NODAL_IMAGE_READERS), write the doubles of the ghost-reading forms.

On a level that is one box spanning its domain a node outside the box is the periodic image (or, between Neumann walls, the mirror image)
of a valid node.  Kernel tests: the existing entry on an array whose ghost nodes hold those images is the reference; the new entry gets the
same valid nodes with NaN in every ghost node.  The random node data carry equal values on the duplicate nodes of a periodic direction
(node n is node 0), as every array of the solver does: a ghost node next to such a pair has two sources, and only then does it not matter
which one a fill or an image read takes.  The expressions and their operands are the same, so everything is compared to the bit.

Solver tests: a solve and three time steps with the switch on against off, also under an allocator that hands out NaNs or zeros
(IAMRX_POISON_ALLOC = 1 / 2), which shows a read of a ghost node nobody fills any more."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEUMANN = 102
BCS = {"periodic": (1, 1, 1), "periodic-x-walls-yz": (1, 0, 0), "walls": (0, 0, 0)}


def _codes(per):
    c = tuple(0 if p else NEUMANN for p in per)
    return c, c


def _node_map(n, per, ng=1):
    """valid node index (0 .. n) behind the nodes -ng .. n + ng of a direction"""
    i = np.arange(-ng, n + 1 + ng)
    return np.where(i < 0, i + n, np.where(i > n, i - n, i)) if per else np.where(i < 0, -i, np.where(i > n, 2 * n - i, i))


def _cell_map(n, per, ng=1):
    i = np.arange(-ng, n + ng)
    return np.where(i < 0, i + n, np.where(i > n - 1, i - n, i)) if per else np.where(i < 0, -1 - i, np.where(i > n - 1, 2 * n - 1 - i, i))


def _valid_nodes(rng, n, per):
    v = rng.standard_normal(tuple(m + 1 for m in n))
    for d in range(3):
        if per[d]:
            hi, lo = [slice(None)] * 3, [slice(None)] * 3
            hi[d], lo[d] = n[d], 0
            v[tuple(hi)] = v[tuple(lo)]
    return v


def _node_arrays(lib, lay, v, n, per):
    """(ghost nodes = images, ghost nodes = NaN) around the valid nodes v, one ghost layer"""
    filled = v[np.ix_(*[_node_map(n[d], per[d]) for d in range(3)])]
    nan = np.full_like(filled, np.nan)
    nan[1:-1, 1:-1, 1:-1] = v
    out = []
    for a in (filled, nan):
        m = lib.MultiFab(lay, lib.NODE, 1, 1)
        m.set_from_global(np.ascontiguousarray(a[..., None]), (-1, -1, -1))
        out.append(m)
    return out


def _whole(mf):
    return mf.to_numpy(0)[0][..., 0].copy()


VALID = (slice(1, -1),) * 3
KCS = (1, 4, 8, 16, 32)       # the library's own choice on these small boxes is 2 planes per workgroup; the 257^3 level of the benchmark runs 32
_RES = {}


def _residuals(lib, n, bc):
    """reference and image-reading residual of one case, computed once: (reference array, image array, image norm, image arrays by kc)"""
    if (n, bc) in _RES:
        return _RES[(n, bc)]
    from iamr_amd import ns as N
    per = BCS[bc]
    rng = np.random.default_rng(100 + sum(n))
    g = lib.Geom.make(n, periodic=per)
    lay = lib.Layout.single(n)
    x_filled, x_nan = _node_arrays(lib, lay, _valid_nodes(rng, n, per), n, per)
    s = 0.5 + rng.random(n)
    sig = lib.MultiFab(lay, lib.CELL, 1, 1)
    sig.set_from_global(np.ascontiguousarray(s[np.ix_(*[_cell_map(n[d], per[d]) for d in range(3)])][..., None]), (-1, -1, -1))
    rhs = lib.MultiFab(lay, lib.NODE, 1, 0)
    rhs.set_from_global(rng.standard_normal(tuple(m + 1 for m in n) + (1,)), (0, 0, 0))
    lobc, hibc = _codes(per)

    def run(images):
        out = lib.MultiFab(lay, lib.NODE, 1, 1)
        out.setval(7.0)
        norm = N.nodal_residual_images(g, out, x_nan, sig, rhs, lobc, hibc) if images else N.nodal_residual(g, out, x_filled, sig, rhs)
        lib.sync()
        return _whole(out), norm

    ref, _ = run(False)
    new, norm = run(True)
    by_kc = {}
    if n[0] >= 16:                                  # the z-marching kernel: other chunk lengths
        try:
            for kc in KCS:
                lib.tuning_set("NODAL_RES_KC", kc)
                by_kc[kc] = run(True)
        finally:
            lib.tuning_set("NODAL_RES_KC", 0)
    _RES[(n, bc)] = (ref, new, norm, by_kc)
    return _RES[(n, bc)]


# cells: one partly filled 32 x 8 tile; ragged tiles and, with 8 / 16 / 32 planes per workgroup, a ragged last chunk; 129 planes (with 32 per
# workgroup: chunks of 32, 32, 32, 32 and 1); the per-node form below the tile kernel's threshold.  The library's own chunk length on boxes
# this small is 2: the longer ones, 32 included, come from the override below
RES_BOXES = [(16, 8, 8), (40, 24, 36), (32, 32, 128), (8, 8, 8)]


@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("n", RES_BOXES, ids=["x".join(map(str, n)) for n in RES_BOXES])
def test_residual_reads_images_for_ghost_nodes(gpu, n, bc):
    ref, new, norm, _ = _residuals(gpu, n, bc)
    assert np.isfinite(ref[VALID]).all() and np.abs(ref[VALID]).max() > 1.0
    assert not np.isnan(new).any()
    assert np.array_equal(new[VALID], ref[VALID])
    assert norm == np.abs(ref[VALID]).max()
    ghosts = np.ones(new.shape, bool)
    ghosts[VALID] = False
    assert (new[ghosts] == 7.0).all()                # nothing is written outside the box


@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("n", RES_BOXES[:3], ids=["x".join(map(str, n)) for n in RES_BOXES[:3]])
def test_residual_chunk_length_changes_no_double(gpu, n, bc):
    ref, new, norm, by_kc = _residuals(gpu, n, bc)
    assert sorted(by_kc) == list(KCS)
    for kc, (a, nrm) in by_kc.items():
        assert np.array_equal(a, new), kc                        # the default chunk length
        assert np.array_equal(a[VALID], ref[VALID]), kc          # the ghost-reading reference
        assert nrm == norm == np.abs(ref[VALID]).max(), kc


# fine cells: 48 coarse cells in x, the smallest level the tiled restriction takes by default; ragged tiles and 8-plane chunks; the per-node form
RESTRICT_BOXES = [(96, 16, 16), (128, 48, 40), (16, 16, 16)]


@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("n", RESTRICT_BOXES, ids=["x".join(map(str, n)) for n in RESTRICT_BOXES])
def test_restriction_reads_images_for_ghost_nodes(gpu, n, bc):
    from iamr_amd import ns as N
    lib = gpu
    per = BCS[bc]
    rng = np.random.default_rng(200 + sum(n))
    g = lib.Geom.make(n, periodic=per)
    flay = lib.Layout.single(n)
    nc = tuple(m // 2 for m in n)
    clay = lib.Layout.single(nc)
    f_filled, f_nan = _node_arrays(lib, flay, _valid_nodes(rng, n, per), n, per)
    start = rng.standard_normal(tuple(m + 3 for m in nc) + (1,))
    lobc, hibc = _codes(per)
    out = []
    for images in (False, True):
        crse = lib.MultiFab(clay, lib.NODE, 1, 1)
        crse.set_from_global(start, (-1, -1, -1))
        if images:
            N.nodal_restrict_images(g, crse, f_nan, lobc, hibc)
        else:
            N.nodal_restrict(crse, f_filled)
        lib.sync()
        out.append(_whole(crse))
    ref, new = out
    assert np.isfinite(ref).all() and np.count_nonzero(ref[VALID] != start[..., 0][VALID]) > 0.99 * ref[VALID].size
    assert not np.isnan(new).any()
    assert np.array_equal(new, ref)                  # valid nodes; the ghost layer keeps its data


def test_entries_refuse_a_level_that_does_not_qualify(gpu):
    from iamr_amd import ns as N
    lib = gpu
    n = (32, 16, 16)
    g = lib.Geom.make(n, periodic=(1, 1, 1))
    two = lib.Layout([((0, 0, 0), (15, 15, 15)), ((16, 0, 0), (31, 15, 15))])
    x = lib.MultiFab(two, lib.NODE, 1, 1)
    x.setval(1.0)
    sig = lib.MultiFab(two, lib.CELL, 1, 1)
    sig.setval(1.0)
    out = lib.MultiFab(two, lib.NODE, 1, 1)
    with pytest.raises(lib.IamrxError):
        N.nodal_residual_images(g, out, x, sig, None)
    crse = lib.MultiFab(lib.Layout.single((16, 8, 8)), lib.NODE, 1, 1)
    with pytest.raises(lib.IamrxError):
        N.nodal_restrict_images(g, crse, x)
    # a Dirichlet (outflow) face has no image
    one = lib.Layout.single(n)
    gw = lib.Geom.make(n, periodic=(1, 1, 0))
    x1, s1, o1 = lib.MultiFab(one, lib.NODE, 1, 1), lib.MultiFab(one, lib.CELL, 1, 1), lib.MultiFab(one, lib.NODE, 1, 1)
    x1.setval(1.0)
    s1.setval(1.0)
    with pytest.raises(lib.IamrxError):
        N.nodal_residual_images(gw, o1, x1, s1, None, (0, 0, NEUMANN), (0, 0, 101))


def _solve(lib, n, per, images, poison):
    from iamr_amd import ns as N
    rng = np.random.default_rng(300 + sum(n))
    g = lib.Geom.make(n, periodic=per)
    lay = lib.Layout.single(n)
    lib.tuning_set("NODAL_IMAGE_READERS", images)
    lib.tuning_set("POISON_ALLOC", poison)
    try:
        sig = lib.MultiFab(lay, lib.CELL, 1, 1)
        sig.set_from_global(1.0 + 0.5 * rng.random(tuple(m + 2 for m in n) + (1,)), (-1, -1, -1))
        rhs = lib.MultiFab(lay, lib.NODE, 1, 0)
        rhs.set_from_global(np.ascontiguousarray(_valid_nodes(rng, n, per)[..., None]), (0, 0, 0))
        phi = lib.MultiFab(lay, lib.NODE, 1, 1)
        phi.setval(0.0)
        lobc, hibc = _codes(per)
        st = N.nodal_solve(g, phi, rhs, sig, 0, lobc, hibc, rel_tol=1e-9, abs_tol=0.0)
        lib.sync()
        return _whole(phi), st.iters
    finally:
        lib.tuning_set("POISON_ALLOC", 0)
        lib.tuning_set("NODAL_IMAGE_READERS", 1)


SOLVES = [((32, 32, 32), (1, 1, 1)), ((32, 32, 32), (0, 0, 0)), ((64, 32, 48), (1, 1, 1)), ((64, 32, 48), (0, 0, 0))]


@pytest.mark.parametrize("n,per", SOLVES, ids=["x".join(map(str, n)) + ("-periodic" if p[0] else "-walls") for n, p in SOLVES])
def test_solve_without_the_fills_equals_the_solve_with_them(gpu, n, per):
    ref, ref_iters = _solve(gpu, n, per, 0, 0)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0.0 and ref_iters >= 2
    for poison in (0, 1, 2):
        for images in (1, 0):
            phi, iters = _solve(gpu, n, per, images, poison)
            assert iters == ref_iters, (images, poison)
            assert np.array_equal(phi, ref), (images, poison)          # ghost nodes included


LID = [0.0] * 9
LID[2 * 3 + 0] = 1.0


def _steps(lib, flow, n, images):
    from iamr_amd import ns as N
    lib.tuning_set("NODAL_IMAGE_READERS", images)
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
        return [ns.data(w).to_numpy(0)[0].copy() for w in (N.NavierStokes.S_NEW, N.NavierStokes.P_NEW)], iters
    finally:
        lib.tuning_set("NODAL_IMAGE_READERS", 1)


# 64^3: the level the register-resident smoother (k_nodal_gsr) takes
STEPS = [("taylorgreen", (32, 32, 32)), ("taylorgreen", (64, 64, 64)), ("cavity", (32, 32, 32))]


@pytest.mark.parametrize("flow,n", STEPS, ids=[f"{f}-{n[0]}" for f, n in STEPS])
def test_three_steps_without_the_fills_equal_three_steps_with_them(gpu, flow, n):
    ref, ref_iters = _steps(gpu, flow, n, 0)
    new, new_iters = _steps(gpu, flow, n, 1)
    assert all(np.isfinite(a[VALID]).all() for a in ref) and np.abs(ref[0][VALID][..., 0]).max() > 0.05
    assert new_iters == ref_iters
    for a, b in zip(new, ref):
        assert a.tobytes() == b.tobytes()
