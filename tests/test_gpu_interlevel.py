"""GPU: the inter-level transfer operators of iamr_amd/csrc/amr.hip (fillpatch_two_levels with k_cellconslin, sync_interp_cellcons,
FluxRegister, average_down, create_umac_grown) at every face, BC type and ratio, against the references of tests/interlevel_numpy.py.

amr.hip is built with -ffp-contract=off and the references restate its expressions in its order: every comparison is np.array_equal.
The input data of the fill-patch cases are chosen so that every branch of the limiter is taken in the cells a case interpolates;
tests/test_cpu_interlevel_ref.py asserts that on the reference's bookkeeping.  Every destination starts from a sentinel."""
import ctypes as C
import numpy as np
import pytest

import interlevel_numpy as il

pytestmark = pytest.mark.gpu
SENT = il.SENTINEL


def same(got, ref, tag):
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = got != ref
        w = np.argwhere(bad)[0]
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.size} differ, max |diff| {float(np.abs(got - ref)[bad].max()):.3e}, first at {tuple(w)}: "
                             f"{got[tuple(w)]!r} != {ref[tuple(w)]!r}")


def cell_mf(lib, lay, G, ng=0):
    """cell-centred MultiFab on lay from a global array (valid cells; ghost cells, if any, hold the sentinel)"""
    if G is None:
        return None
    m = lib.MultiFab(lay, lib.CELL, G.shape[3], ng)
    if ng:
        m.setval(SENT)
    for li in range(m.nlocal()):
        lo, hi, _ = lay.local_box(li)
        a = G[il.box_slices(lo, hi, (0, 0, 0))]
        if ng:
            b, _ = m.to_numpy(li)
            b[ng:-ng, ng:-ng, ng:-ng] = a
            a = b
        m.from_numpy(a, li)
    return m


def typed_mf(lib, lay, typ, G, ng=0, fill=SENT):
    """MultiFab of index type typ from a global array over the domain's points of that type; ghost points hold `fill`"""
    m = lib.MultiFab(lay, typ, G.shape[3], ng)
    for li in range(m.nlocal()):
        lo, hi, _ = lay.local_box(li)
        hi = tuple(hi[d] + typ[d] for d in range(3))
        a = np.full(tuple(hi[d] - lo[d] + 1 + 2 * ng for d in range(3)) + (G.shape[3],), fill)
        a[tuple(slice(ng, a.shape[d] - ng) for d in range(3))] = G[il.box_slices(lo, hi, (0, 0, 0))]
        m.from_numpy(a, li)
    return m


def by_box(mf):
    """{global box index: (array, lo)} of the local fabs"""
    return {mf.layout.local_box(li)[2]: mf.to_numpy(li) for li in range(mf.nlocal())}


# ---------------------------------------------------------------------------------------------------------------------------
# fill-patch
def gpu_fillpatch(lib, nc, ratio, per, fboxes, ng, time, fine_td, crse_td, bcs=None, edlo=None, edhi=None, scomp=0, dcomp=0, ncomp=None,
                  dst_ncomp=None, crse_chop=(4, 8, 5)):
    """fine_td / crse_td: (old global array or None, new, t_old, t_new); returns {box: (array with ghost cells, lo)}"""
    nf = tuple(ratio * v for v in nc)
    cg, fg = lib.Geom.make(nc, periodic=per), lib.Geom.make(nf, periodic=per)
    crse_lay = lib.Layout.decompose(nc, crse_chop)
    fine_lay = lib.Layout(fboxes)
    fo, fn = cell_mf(lib, fine_lay, fine_td[0]), cell_mf(lib, fine_lay, fine_td[1])
    co, cn = cell_mf(lib, crse_lay, crse_td[0]), cell_mf(lib, crse_lay, crse_td[1])
    ncomp = crse_td[1].shape[3] - scomp if ncomp is None else ncomp
    dst = lib.MultiFab(fine_lay, lib.CELL, dcomp + ncomp if dst_ncomp is None else dst_ncomp, ng)
    dst.setval(SENT)
    lib.fillpatch_two_levels(dst, time, (fo, fn, fine_td[2], fine_td[3]), (co, cn, crse_td[2], crse_td[3]), cg, fg, scomp=scomp, ncomp=ncomp,
                             dcomp=dcomp, ratio=ratio, bc=bcs, extdir_lo=edlo, extdir_hi=edhi)
    return by_box(dst)


def run_case(lib, orc, case, seed=3):
    fb = il.case_fine_boxes(case)
    F = il.case_fine_data(case, seed)
    got = gpu_fillpatch(lib, case["nc"], case["ratio"], case["per"], fb, case["ng"], 0.0, (None, F, 0.0, 0.0), (None, case["crse"], 0.0, 0.0),
                        case["bcs"], case["edlo"], case["edhi"])
    ref = il.case_ref(orc, case)
    return got, ref


def check_case(got, ref, tag):
    assert len(got) == len(ref.boxes)
    for b, (ra, rlo) in enumerate(ref.boxes):
        ga, glo = got[b]
        assert tuple(glo) == tuple(rlo)
        assert not (ra == SENT).any(), (tag, b)             # the reference fills every cell, ghost cells outside the walls included
        same(ga, ra, (tag, "box", b))


@pytest.mark.parametrize("d,side,ratio", il.WALL_CASES)
def test_fillpatch_at_a_wall_every_bc_type(orc, gpu, d, side, ratio):
    """a two-box patch on each of the six faces (ratio 2; y-lo and z-hi also at ratio 4), ng = 3: reflect_odd, reflect_even, foextrap,
    ext_dir and hoextrap on the touched face for five wall-normal ramps (the one-sided slope of cslope is what reaches the result
    in the ext_dir and hoextrap components), + the general and the kinked component.  Every cell, ghost cells outside the wall
    included, bit-equal to the reference."""
    case = il.wall_case(d, side, ratio)
    got, ref = run_case(gpu, orc, case)
    check_case(got, ref, ("wall", d, side, ratio))


def test_fillpatch_in_a_corner_of_three_walls(orc, gpu):
    """a patch on the x-lo, y-lo and z-hi walls with a different BC type on each and another assignment per component: the ghost
    cells outside two and three walls (fine level: composition of the one-dimensional fills; coarse patch: the 27-cell range of the
    excursion limiter reads them)"""
    got, ref = run_case(gpu, orc, il.corner_case())
    check_case(got, ref, "corner")


@pytest.mark.parametrize("name,ng,ratio", il.LAYOUT_CASES)
def test_fillpatch_layouts_fully_periodic(orc, gpu, name, ng, ratio):
    """span_x: the patch's own image covers its x ghost cells; neg_yz: ghost cells through images with negative coarse indices (y) and
    past the hi end (z); ell: three unequal boxes with a re-entrant corner; one / two / eight: one region in 1, 2 and 8 boxes"""
    got, ref = run_case(gpu, orc, il.layout_case(name, ng, ratio))
    check_case(got, ref, (name, ng, ratio))


def test_fillpatch_does_not_depend_on_how_the_region_is_chopped(gpu):
    """the same region as 1, 2 and 8 boxes (the claim at fp_info): every cell of every box of the chopped layouts, ghost cells
    included, is bit-equal to that cell of the one-box result"""
    res = {}
    for name in ("one", "two", "eight"):
        case = il.layout_case(name, 3, 2)
        fb = il.case_fine_boxes(case)
        res[name] = gpu_fillpatch(gpu, case["nc"], 2, case["per"], fb, 3, 0.0, (None, il.case_fine_data(case), 0.0, 0.0), (None, case["crse"], 0.0, 0.0))
    base, blo = res["one"][0]
    assert not (base == SENT).any()
    for name in ("two", "eight"):
        for b, (a, lo) in res[name].items():
            sl = tuple(slice(lo[d] - blo[d], lo[d] - blo[d] + a.shape[d]) for d in range(3))
            same(a, base[sl], (name, b))


def _neg_case(ncomp_kinds):
    nc, cboxes, T = il.LAYOUTS["neg_yz"]
    comps = [il.data_G(nc, 2 + 7 * n) if k == "G" else il.data_K(nc, T) + float(n) for n, k in enumerate(ncomp_kinds)]
    return dict(nc=nc, ratio=2, per=(1, 1, 1), cboxes=cboxes, ng=3, bcs=None, edlo=None, edhi=None, crse=np.stack(comps, axis=-1), kinds=ncomp_kinds)


def test_fillpatch_component_offsets(orc, gpu):
    """scomp = 2, dcomp = 1, ncomp = 3 from 6-component sources into a 5-component destination: components 0 and 4 keep the sentinel"""
    case = _neg_case("GKGKGK")
    fb = il.case_fine_boxes(case)
    F = il.case_fine_data(case)
    got = gpu_fillpatch(gpu, case["nc"], 2, case["per"], fb, 3, 0.0, (None, F, 0.0, 0.0), (None, case["crse"], 0.0, 0.0), scomp=2, dcomp=1, ncomp=3, dst_ncomp=5)
    ref = il.fillpatch_ref(orc, fb, 3, 0.0, (None, F[..., 2:5], 0.0, 0.0), fb, (None, case["crse"][..., 2:5], 0.0, 0.0), case["nc"], 2, case["per"])
    for b, (ra, rlo) in enumerate(ref.boxes):
        ga, _ = got[b]
        assert not (ra == SENT).any()
        same(ga[..., 1:4], ra, ("offsets", b))
        assert (ga[..., 0] == SENT).all() and (ga[..., 4] == SENT).all()


def test_fillpatch_eight_components(orc, gpu):
    """ncomp = 8, the cap of k_cellconslin's BC table"""
    case = _neg_case("GKGKGKGK")
    got, ref = run_case(gpu, orc, case)
    check_case(got, ref, "ncomp8")


@pytest.mark.parametrize("which", ["fine", "crse"])
def test_fillpatch_time_interpolation(orc, gpu, which):
    """the TimeData of one level holds old (t = 0.25) and new (t = 1.5) data, the other level new data only (old = None).  time = t_old,
    t_new and t_new - 0.5e-3 dt (inside the snap window): bit-equal to a call that is given that array alone.  time = t_old + 0.3 dt:
    a * old + b * new as the reference forms it, and different from both."""
    case = _neg_case("GK")
    nc, per, fb = case["nc"], case["per"], il.case_fine_boxes(case)
    F0, F1 = il.case_fine_data(case, 3), il.case_fine_data(case, 4)
    C1 = case["crse"]
    C0 = np.stack([il.data_G(nc, 40), il.data_K(nc, 11)], axis=-1)
    t_old, t_new = 0.25, 1.5
    dt = t_new - t_old

    def tds(old, new):
        fine = (F0 if old else None, F1 if new else F0, t_old, t_new) if which == "fine" else (None, F1, 0.0, 0.0)
        crse = (C0 if old else None, C1 if new else C0, t_old, t_new) if which == "crse" else (None, C1, 0.0, 0.0)
        return fine, crse

    def gpu_at(time, old=True, new=True):
        fine, crse = tds(old, new)
        return gpu_fillpatch(gpu, nc, 2, per, fb, 3, time, fine, crse)[0][0]

    def ref_at(time):
        fine, crse = tds(True, True)
        return il.fillpatch_ref(orc, fb, 3, time, fine, fb, crse, nc, 2, per).boxes[0][0]
    new_alone, old_alone = gpu_at(7.0, old=False), gpu_at(7.0, old=False, new=False)
    assert not np.array_equal(new_alone, old_alone)
    same(new_alone, ref_at(t_new), "new alone")
    same(old_alone, ref_at(t_old), "old alone")
    same(gpu_at(t_old), old_alone, "time = t_old")
    same(gpu_at(t_new), new_alone, "time = t_new")
    same(gpu_at(t_new - 0.5e-3 * dt), new_alone, "time inside the snap window of t_new")
    mid = gpu_at(t_old + 0.3 * dt)
    same(mid, ref_at(t_old + 0.3 * dt), "time = t_old + 0.3 dt")
    assert np.abs(mid - new_alone).max() > 0.1 and np.abs(mid - old_alone).max() > 0.1
    # just outside the window the data are interpolated
    out = gpu_at(t_new - 2.0e-3 * dt)
    same(out, ref_at(t_new - 2.0e-3 * dt), "time just outside the snap window")
    assert not np.array_equal(out, new_alone)


@pytest.mark.parametrize("walled", [True, False])
def test_sync_interp_matches_fillpatch_ref_with_an_empty_fine_level(orc, gpu, walled):
    """sync_interp_cellcons: every valid cell of the fine boxes interpolated from the coarse increment, homogeneous ext_dir values;
    walled (y): a bcrec with ext_dir, hoextrap and reflect_odd and boxes on both walls; periodic: bcrec = None.  The destination's
    ghost cells and other components keep the sentinel."""
    lib = gpu
    nc, ratio = (12, 8, 8), 2
    nf = tuple(ratio * v for v in nc)
    per = (1, 0, 1) if walled else (1, 1, 1)
    cboxes = [((0, 0, 2), (5, 3, 5)), ((6, 4, 0), (11, 7, 3)), ((2, 4, 6), (4, 5, 7))]
    fb = [il.refine_box(b, ratio) for b in cboxes]
    crse = np.stack([il.data_W(nc, 1, 0, 4), il.data_G(nc, 2), il.data_K(nc, 12), il.data_W(nc, 1, 1, 9)], axis=-1)
    bcs = None
    if walled:
        bcs = [((0, il.BC_EXT_DIR, 0), (0, il.BC_HOEXTRAP, 0)), ((0, il.BC_REFLECT_ODD, 0), (0, il.BC_EXT_DIR, 0)),
               ((0, il.BC_HOEXTRAP, 0), (0, il.BC_FOEXTRAP, 0))]
    cg, fg = lib.Geom.make(nc, periodic=per), lib.Geom.make(nf, periodic=per)
    cmf = cell_mf(lib, lib.Layout.decompose(nc, (5, 8, 4)), crse)
    dst = lib.MultiFab(lib.Layout(fb), lib.CELL, 5, 1)
    dst.setval(SENT)
    lib.check(lib.lib().iamrx_sync_interp(dst.h, 2, cmf.h, 1, 3, C.byref(cg), C.byref(fg), ratio, lib._bcrec(3, bcs) if walled else None))
    ref = il.fillpatch_ref(orc, fb, 0, 0.0, None, [], (None, crse[..., 1:4], 0.0, 0.0), nc, ratio, per, bcs, [[0.0] * 3] * 3, [[0.0] * 3] * 3)
    assert ref.interp.sum() == sum(np.prod([hi[d] - lo[d] + 1 for d in range(3)]) for lo, hi in fb)      # no fine data: every cell of every box
    got = by_box(dst)
    for b, (ra, _) in enumerate(ref.boxes):
        ga, _ = got[b]
        assert not (ra == SENT).any()
        same(ga[1:-1, 1:-1, 1:-1, 2:5], ra, ("sync_interp", b))
        keep = ga.copy()
        keep[1:-1, 1:-1, 1:-1, 2:5] = SENT
        assert (keep == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------------
# flux register
def face_arrays(rng, n, ncomp, per):
    """one random array per direction on the faces of a domain of n cells; the face at n repeats face 0 in a periodic direction"""
    out = []
    for d in range(3):
        s = list(n); s[d] += 1
        a = rng.standard_normal(tuple(s) + (ncomp,))
        if per[d]:
            lo = [slice(None)] * 3; hi = [slice(None)] * 3
            lo[d] = 0; hi[d] = n[d]
            a[tuple(hi)] = a[tuple(lo)]
        out.append(a)
    return out


def _side_boxes(nc, d, side):
    """two coarse boxes, four cells thick in d, on the (d, side) face of the domain; interior in the other directions"""
    lo, hi = [2, 2, 2], [nc[0] - 3, nc[1] - 3, nc[2] - 3]
    lo[d], hi[d] = (0, 3) if side == 0 else (nc[d] - 4, nc[d] - 1)
    e = (d + 1) % 3
    h1, l2 = list(hi), list(lo)
    h1[e] = lo[e] + 1; l2[e] = lo[e] + 2
    return [(tuple(lo), tuple(h1)), (tuple(l2), tuple(hi))]


FLUX_CASES = {f"periodic-{d}-{s}": dict(cboxes=("side", d, s)) for d in range(3) for s in (0, 1)}
FLUX_CASES.update({
    "wall-0-0": dict(cboxes=("side", 0, 0), per=(0, 1, 1)),
    "wall-2-1": dict(cboxes=("side", 2, 1), per=(1, 1, 0)),
    "ell": dict(cboxes=il.LAYOUTS["ell"][1]),
    "chopped": dict(cboxes=[((2, 1, 1), (9, 6, 6))], chop=(5, 3, 4)),
    "ratio4": dict(cboxes=("side", 1, 1), ratio=4),
    "crse_add": dict(cboxes=("side", 0, 1), add=True),
    "offsets": dict(cboxes=il.LAYOUTS["ell"][1], nflux=4, nreg=4, nstate=5, fl_sc=1, reg_c=1, st_dc=2, ncomp=2),
    "scale": dict(cboxes=("side", 2, 0), scale=-0.5),
})


@pytest.mark.parametrize("name", list(FLUX_CASES))
def test_flux_register_matches_direct_evaluation(gpu, name):
    """CrseInit(-dt_c) [+ CrseInit(add = True) of a second flux], two FineAdd(+dt_f), Reflux into a random state, on a 12 x 8 x 8 coarse
    level: a patch on each of the six periodic faces (the correction lands on the far side of the domain), on two walls (nothing is
    added outside the domain), an L of three boxes (a register also corrects the coarse cells under a neighbouring fine box, which
    average_down overwrites later: a deliberate departure from AMReX), a coarse layout whose boxes the slabs
    straddle, ratio 4 (16 fine faces per coarse face), component offsets on the flux, register and state side (flux 1 -> register 1 ->
    state 2, two components of 4 / 4 / 5; the other register and state components untouched), scale = -0.5"""
    lib = gpu
    cfg = FLUX_CASES[name]
    nc = (12, 8, 8)
    per, ratio, scale = cfg.get("per", (1, 1, 1)), cfg.get("ratio", 2), cfg.get("scale", 1.0)
    cboxes = _side_boxes(nc, cfg["cboxes"][1], cfg["cboxes"][2]) if cfg["cboxes"][0] == "side" else cfg["cboxes"]
    nflux, nreg, nstate = cfg.get("nflux", 2), cfg.get("nreg", 2), cfg.get("nstate", 2)
    fl_sc, reg_c, st_dc, ncomp = cfg.get("fl_sc", 0), cfg.get("reg_c", 0), cfg.get("st_dc", 0), cfg.get("ncomp", 2)
    nf = tuple(ratio * v for v in nc)
    rng = np.random.default_rng(6)
    CF, CF2, FF1, FF2 = (face_arrays(rng, nc, nflux, per), face_arrays(rng, nc, nflux, per), face_arrays(rng, nf, nflux, per),
                         face_arrays(rng, nf, nflux, per))
    S0 = rng.standard_normal(nc + (nstate,))
    dt_c, dt_f, vol = 0.1, 0.1 / ratio, 0.25
    cg = lib.Geom.make(nc, periodic=per)
    crse_lay = lib.Layout.decompose(nc, cfg.get("chop", (6, 8, 4)))
    fine_lay = lib.Layout([il.refine_box(b, ratio) for b in cboxes])
    fr = lib.FluxRegister(fine_lay, crse_lay, cg, ratio, nreg)
    rr = il.FluxRegRef(cboxes, nc, per, ratio, nreg)
    if name == "offsets":           # the register components that no call below addresses start from 2 and must still hold it at the end
        fr.setVal(2.0); rr.set_val(2.0)
    for d in range(3):
        t = lib.face(d)
        fr.CrseInit(typed_mf(lib, crse_lay, t, CF[d]), d, fl_sc, reg_c, ncomp, -dt_c)
        rr.crse_init(CF[d], d, fl_sc, reg_c, ncomp, -dt_c)
        if cfg.get("add"):
            fr.CrseInit(typed_mf(lib, crse_lay, t, CF2[d]), d, fl_sc, reg_c, ncomp, 0.3, add=True)
            rr.crse_init(CF2[d], d, fl_sc, reg_c, ncomp, 0.3, add=True)
        for FF in (FF1, FF2):
            fr.FineAdd(typed_mf(lib, fine_lay, t, FF[d]), d, fl_sc, reg_c, ncomp, dt_f)
            rr.fine_add(FF[d], d, fl_sc, reg_c, ncomp, dt_f)
    S = cell_mf(lib, crse_lay, S0)
    fr.Reflux(S, vol, scale, reg_c, st_dc, ncomp)
    exp = S0.copy()
    rr.reflux(exp, vol, scale, reg_c, st_dc, ncomp)
    if name == "offsets":           # register components 0 and 3, read out through state components 0 and 4
        for rc, sc in ((0, 0), (3, 4)):
            fr.Reflux(S, vol, scale, rc, sc, 1)
            rr.reflux(exp, vol, scale, rc, sc, 1)
        assert all((rr.reg[k][..., [0, 3]] == 2.0).all() for k in rr.reg)
    got = S.gather_valid(nc)
    changed = (exp != S0).any(axis=-1)
    assert changed.sum() >= 40 and np.abs(exp - S0).max() > 0.5
    if cfg["cboxes"][0] == "side":
        d, side = cfg["cboxes"][1], cfg["cboxes"][2]
        far = [slice(None)] * 3
        far[d] = nc[d] - 1 if side == 0 else 0
        assert changed[tuple(far)].any() == bool(per[d])              # through the periodic boundary, and not through a wall
    same(got, exp, name)
    untouched = [n for n in range(nstate) if not st_dc <= n < st_dc + ncomp and not (name == "offsets" and n in (0, 4))]
    assert np.array_equal(got[..., untouched], S0[..., untouched])


def test_flux_register_telescopes_at_ratio_4(gpu):
    """fine fluxes that are the exact refinement of the coarse ones (coarse / 16 on each of the 16 children, four fine steps of dt_c / 4):
    the registers cancel and Reflux changes nothing, to the round-off of the 69 operations behind a register entry, divided by the volume"""
    lib = gpu
    nc, ratio, ncomp = (12, 8, 8), 4, 2
    nf = tuple(ratio * v for v in nc)
    cboxes = il.LAYOUTS["ell"][1]
    cg = lib.Geom.make(nc)
    crse_lay = lib.Layout.decompose(nc, (6, 8, 4))
    fine_lay = lib.Layout([il.refine_box(b, ratio) for b in cboxes])
    CF = face_arrays(np.random.default_rng(9), nc, ncomp, (1, 1, 1))
    dt_c, vol = 0.1, 0.25
    fr = lib.FluxRegister(fine_lay, crse_lay, cg, ratio, ncomp)
    for d in range(3):
        idx = [np.arange(nf[e] + (e == d)) // ratio for e in range(3)]          # fine face r i <-> coarse face i; the others are never read
        Fd = CF[d][np.ix_(*idx)] * (1.0 / 16.0)
        fr.CrseInit(typed_mf(lib, crse_lay, lib.face(d), CF[d]), d, 0, 0, ncomp, -dt_c)
        m = typed_mf(lib, fine_lay, lib.face(d), Fd)
        for _ in range(ratio):
            fr.FineAdd(m, d, 0, 0, ncomp, dt_c / ratio)
    S = lib.MultiFab(crse_lay, lib.CELL, ncomp, 0); S.setval(0.0)
    fr.Reflux(S, vol, 1.0, 0, 0, ncomp)
    # a register entry is -dt_c c + 4 (dt_c / 4) (16 terms c / 16), exactly zero without rounding.  Roundings: 1 in CrseInit, and per
    # FineAdd 15 in the sum, 1 in the product with dt_f and 1 in the addition to the register: 69 in all, each at most 2^-53 of a partial
    # result of magnitude <= dt_c |c| (c / 16 and dt_c / 4 are exact).  A coarse cell takes at most one entry / vol per direction (the
    # boxes of the L touch a cell from one side per direction at most).
    bound = sum(69 * 2.0 ** -53 * dt_c * np.abs(CF[d]).max() / vol for d in range(3))
    assert np.abs(S.gather_valid(nc)).max() <= bound


# ---------------------------------------------------------------------------------------------------------------------------
# average down
@pytest.mark.parametrize("ratio", [2, 4])
@pytest.mark.parametrize("typ", ["cell", "facex", "facey", "facez", "node"])
def test_average_down_at_the_hi_corner_of_the_domain(gpu, typ, ratio):
    """a two-box fine patch in the (hi, hi, hi) corner of a 12 x 8 x 8 level (the last face / node index of the domain is written), a
    coarse layout whose boxes the coarsened fine boxes straddle, scomp = 1 of 3 components; component 0 bit-unchanged"""
    lib = gpu
    nc = (12, 8, 8)
    t = {"cell": lib.CELL, "facex": lib.face(0), "facey": lib.face(1), "facez": lib.face(2), "node": lib.NODE}[typ]
    cboxes = [((6, 4, 3), (8, 7, 7)), ((9, 4, 3), (11, 7, 7))]
    crse_lay = lib.Layout.decompose(nc, (5, 3, 8))
    fine_lay = lib.Layout([il.refine_box(b, ratio) for b in cboxes])
    rng = np.random.default_rng(4)
    F = rng.standard_normal(tuple(ratio * nc[d] + t[d] for d in range(3)) + (3,))
    Cg = rng.standard_normal(tuple(nc[d] + t[d] for d in range(3)) + (3,))
    fine, crse = typed_mf(lib, fine_lay, t, F), typed_mf(lib, crse_lay, t, Cg)
    lib.average_down(fine, crse, scomp=1, ncomp=2, ratio=ratio)
    exp = il.average_down_ref(F, Cg, t, cboxes, ratio, 1, 2)
    got = crse.gather_valid(nc)
    assert exp[nc[0] - 1 + t[0], nc[1] - 1 + t[1], nc[2] - 1 + t[2], 1] != Cg[nc[0] - 1 + t[0], nc[1] - 1 + t[1], nc[2] - 1 + t[2], 1]
    assert (exp[..., 1] != Cg[..., 1]).sum() == np.prod([6 + t[0], 4 + t[1], 5 + t[2]])
    same(got, exp, (typ, ratio))
    assert np.array_equal(got[..., 0], Cg[..., 0])


# ---------------------------------------------------------------------------------------------------------------------------
# create_umac_grown
UMAC_CASES = {
    "lo_corner": dict(nc=(8, 8, 8), cboxes=[((0, 0, 0), (3, 3, 2))]),
    "hi_corner": dict(nc=(8, 8, 8), cboxes=[((5, 4, 4), (7, 7, 7))]),
    "wall_ylo": dict(nc=(8, 8, 8), cboxes=[((2, 0, 2), (5, 3, 5))], per=(1, 0, 1)),
    "ell": dict(nc=(12, 8, 8), cboxes=il.LAYOUTS["ell"][1]),
    "divu": dict(nc=(12, 8, 8), cboxes=il.LAYOUTS["ell"][1], divu=True),
    "ratio4": dict(nc=(8, 8, 8), cboxes=[((0, 2, 4), (3, 5, 7)), ((4, 2, 4), (5, 3, 7))], ratio=4, divu=True),
}


def umac_property(g, r, fbox, fdx, divu, tag):
    """on the arrays g = (u, v, w) of one box grown by one cell: div(u) - divu at round-off in the not-covered ghost cells inside the
    domain with exactly one face neighbour in the level, the FaceLinear / fine values `lin` of the reference on every face of those with
    0 or >= 2 such neighbours; returns the numbers of cells of the two kinds"""
    lo, mlo, mask = r["lo"], r["mask_lo"], r["mask"]
    fixed = set(r["count1"])
    bhi = fbox[1]
    n_fixed = n_kept = 0
    for k in range(lo[2], bhi[2] + 2):
        for j in range(lo[1], bhi[1] + 2):
            for i in range(lo[0], bhi[0] + 2):
                if mask[i - mlo[0], j - mlo[1], k - mlo[2]] != 2:
                    continue
                a, b, c = i - lo[0], j - lo[1], k - lo[2]
                if (i, j, k) in fixed:
                    terms = [(g[0][a + 1, b, c] - g[0][a, b, c]) / fdx[0], (g[1][a, b + 1, c] - g[1][a, b, c]) / fdx[1],
                             (g[2][a, b, c + 1] - g[2][a, b, c]) / fdx[2]]
                    dv = float(divu[i + 1, j + 1, k + 1]) if divu is not None else 0.0
                    scale = sum(abs(g[e][a + (e == 0), b + (e == 1), c + (e == 2)]) + abs(g[e][a, b, c]) for e in range(3)) / min(fdx) + abs(dv)
                    assert abs(terms[0] + terms[1] + terms[2] - dv) <= 16 * 2.0 ** -52 * scale, (tag, (i, j, k))
                    n_fixed += 1
                else:
                    for e in range(3):
                        for s in (0, 1):
                            q = (a + s * (e == 0), b + s * (e == 1), c + s * (e == 2))
                            assert g[e][q] == r["lin"][e][q], (tag, (i, j, k), e, s)
                    n_kept += 1
    return n_fixed, n_kept


@pytest.mark.parametrize("name", list(UMAC_CASES))
def test_create_umac_grown_matches_the_per_box_reference(gpu, name):
    """FaceLinear fill of the ghost faces from the periodically extended coarse faces, fine data of sibling boxes and periodic images
    on top, the level mask (covered cells of an L-shaped patch: 1; outside a wall: 3) and the divergence fix with and without divu:
    every face of every box grown by one cell bit-equal to the reference.  wall_ylo: only the faces on or inside the closed domain
    are compared -- what lies outside a wall is the BC fill's business, create_umac_grown leaves there what the zero-initialised coarse
    patch gives.  Property: a not-covered ghost cell inside the domain with exactly one face neighbour in the level has
    div(u) - divu at round-off afterwards; one with 0 or >= 2 such neighbours keeps its FaceLinear / fine values."""
    lib = gpu
    cfg = UMAC_CASES[name]
    nc, ratio, per = cfg["nc"], cfg.get("ratio", 2), cfg.get("per", (1, 1, 1))
    nf = tuple(ratio * v for v in nc)
    fboxes = [il.refine_box(b, ratio) for b in cfg["cboxes"]]
    rng = np.random.default_rng(12)
    UC, UF = face_arrays(rng, nc, 1, per), face_arrays(rng, nf, 1, per)
    cg, fg = lib.Geom.make(nc, periodic=per), lib.Geom.make(nf, periodic=per)
    crse_lay = lib.Layout.decompose(nc, (4, 8, 5))
    fine_lay = lib.Layout(fboxes)
    uc = [typed_mf(lib, crse_lay, lib.face(d), UC[d]) for d in range(3)]
    uf = [typed_mf(lib, fine_lay, lib.face(d), UF[d], ng=1, fill=7.0e30) for d in range(3)]
    divu_mf, divu = None, None
    if cfg.get("divu"):
        D = 3.0 * rng.standard_normal(nf)
        divu = D[np.ix_(*[np.arange(-1, nf[d] + 1) % nf[d] for d in range(3)])]
        divu_mf = lib.MultiFab(fine_lay, lib.CELL, 1, 1)
        divu_mf.set_from_global(divu[..., None], (-1, -1, -1))
    lib.create_umac_grown(uf, uc, cg, fg, ratio, divu=divu_mf)
    fdx = tuple(float(v) for v in fg.dx)
    ref = il.umac_grown_ref([a[..., 0] for a in UC], [a[..., 0] for a in UF], fboxes, nc, ratio, per, divu, fdx)
    got = [by_box(m) for m in uf]
    n_fixed = n_kept = 0
    for b, r in enumerate(ref):
        g = [got[d][b][0][..., 0] for d in range(3)]
        for d in range(3):
            assert tuple(got[d][b][1]) == tuple(r["lo"])
            ok = np.ones(g[d].shape, bool)
            for e in range(3):
                if not per[e]:
                    ix = np.arange(r["lo"][e], r["lo"][e] + g[d].shape[e])
                    m = (ix >= 0) & (ix <= nf[e] - 1 + (e == d))
                    ok &= m.reshape([-1 if q == e else 1 for q in range(3)])
            assert np.abs(g[d][ok]).max() < 1e3                         # no sentinel left
            same(np.where(ok, g[d], 0.0), np.where(ok, r["u"][d], 0.0), (name, "box", b, "dir", d))
        nfx, nkp = umac_property(g, r, fboxes[b], fdx, divu, (name, b))
        n_fixed += nfx; n_kept += nkp
    assert n_fixed >= 100 and n_kept >= 12
    if name in ("ell", "divu"):
        assert any((r["mask"] == 1).any() for r in ref)
    if name == "wall_ylo":
        assert (ref[0]["mask"] == 3).any()
