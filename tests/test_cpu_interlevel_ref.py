"""CPU: the references of tests/interlevel_numpy.py against the oracle's single-box entry points, and the conditions on the input
data of tests/test_gpu_interlevel.py (asserted on the reference's bookkeeping alone, so that no GPU case can pass vacuously)."""
import ctypes as C
import math
import numpy as np
import pytest

import interlevel_numpy as il


# ---------------------------------------------------------------------------------------------------------------------------
def _umac_data(nc, ratio, seed, per=(1, 1, 1)):
    rng = np.random.default_rng(seed)
    nf = tuple(ratio * v for v in nc)
    UC, UF = [], []
    for d in range(3):
        for n, out in ((nc, UC), (nf, UF)):
            s = list(n); s[d] += 1
            a = rng.standard_normal(tuple(s))
            if per[d]:
                lo = [slice(None)] * 3; hi = [slice(None)] * 3
                lo[d] = 0; hi[d] = n[d]
                a[tuple(hi)] = a[tuple(lo)]            # the periodic image of face 0
            out.append(a)
    return UC, UF


@pytest.mark.parametrize("vbox", [((8, 12, 8), (23, 19, 23)), ((0, 0, 8), (15, 7, 23))], ids=["interior", "periodic_lo"])
def test_umac_grown_ref_one_box_equals_oracle(orc, vbox):
    """one box, divu = None: bit-equal to orc_create_umac_grown (the configuration of the existing GPU test's union box, and a box on
    the periodic lo faces in x and y, where the coarse faces come through images with negative indices)"""
    L = orc.lib()
    nc, ratio = (16, 16, 16), 2
    nf = tuple(ratio * v for v in nc)
    vlo, vhi = vbox
    UC, UF = _umac_data(nc, ratio, 12)
    ucf, uff = [], []
    for d in range(3):
        cf = orc.Fab(nc, orc.face(d), 2, 1)
        idx = [np.mod(np.arange(cf.lo[e], cf.hi[e] + 1), nc[e]) for e in range(3)]
        fi = np.arange(cf.lo[d], cf.hi[d] + 1)
        idx[d] = np.where(fi < 0, fi + nc[d], np.where(fi > nc[d], fi - nc[d], fi))
        cf.a[..., 0] = UC[d][np.ix_(*idx)]
        ucf.append(cf)
        lo = [vlo[e] - 1 for e in range(3)]; hi = [vhi[e] + 1 + (1 if e == d else 0) for e in range(3)]
        ff = orc.Fab(nf, orc.face(d), 0, 1, lo=lo, hi=hi)
        ff.a[...] = 7.0e30
        ff.a[1:-1, 1:-1, 1:-1, 0] = UF[d][vlo[0]:vhi[0] + 1 + (d == 0), vlo[1]:vhi[1] + 1 + (d == 1), vlo[2]:vhi[2] + 1 + (d == 2)]
        uff.append(ff)
    fdx = (C.c_double * 3)(*[1.0 / nf[e] for e in range(3)])
    L.orc_create_umac_grown(orc.fabptrs(uff), orc.i3(vlo), orc.i3(vhi), orc.fabptrs(ucf), ratio, fdx, orc.i3(nf), orc.i3((1, 1, 1)))
    ref = il.umac_grown_ref(UC, UF, [vbox], nc, ratio, (1, 1, 1))[0]
    assert len(ref["count1"]) == 2 * sum((vhi[a] - vlo[a] + 1) * (vhi[b] - vlo[b] + 1) for a, b in ((0, 1), (0, 2), (1, 2)))
    for d in range(3):
        assert np.array_equal(ref["u"][d], uff[d].a[..., 0]), d
        assert not np.array_equal(ref["u"][d], ref["lin"][d])


def test_umac_grown_ref_leaves_the_re_entrant_corner_of_an_ell_alone():
    """three boxes in an L: the ghost cells along the re-entrant corner have two face neighbours in the level (one in the box itself,
    mask 0, one in the sibling, mask 1) and keep their FaceLinear faces; the cells next to them, with one neighbour, are corrected."""
    nc, cboxes = il.LAYOUTS["ell"][0], il.LAYOUTS["ell"][1]
    fboxes = [il.refine_box(b, 2) for b in cboxes]
    UC, UF = _umac_data(nc, 2, 12)
    ref = il.umac_grown_ref(UC, UF, fboxes, nc, 2, (1, 1, 1))
    r = ref[0]                                          # the box [2..13] x [2..5] x [4..11]; its sibling [2..5] x [6..11] sits on top of it
    lo, mlo = r["lo"], r["mask_lo"]
    for k in range(4, 12):
        assert r["mask"][6 - mlo[0], 6 - mlo[1], k - mlo[2]] == 2 and r["mask"][5 - mlo[0], 6 - mlo[1], k - mlo[2]] == 1
        assert (6, 6, k) not in r["count1"] and (7, 6, k) in r["count1"]
        assert r["u"][1][6 - lo[0], 7 - lo[1], k - lo[2]] == r["lin"][1][6 - lo[0], 7 - lo[1], k - lo[2]]
        assert r["u"][1][7 - lo[0], 7 - lo[1], k - lo[2]] != r["lin"][1][7 - lo[0], 7 - lo[1], k - lo[2]]


def test_fillpatch_ref_reproduces_the_two_box_recipe(orc):
    """the recipe of test_gpu_amr.test_fillpatch_two_levels_matches_oracle (one oracle call on the union of the two boxes) on that
    test's configuration: every cell of both boxes bit-equal to fillpatch_ref, which fills the whole level and cuts the boxes out"""
    L = orc.lib()
    nc, nf, ncomp, ng, ratio = (16, 16, 16), (32, 32, 32), 3, 3, 2
    per = (1, 0, 1)
    fboxes = [((0, 0, 8), (15, 15, 15)), ((0, 0, 16), (15, 15, 23))]
    bcs = [((0, 2, 0), (0, 2, 0)), ((0, 3, 0), (0, 3, 0)), ((0, 4, 0), (0, 4, 0))]
    edlo = [[0.0, 0.0, 0.0], [0.0, 0.3, 0.0], [0.0, 0.0, 0.0]]
    edhi = [[0.0, 0.0, 0.0], [0.0, -0.2, 0.0], [0.0, 0.0, 0.0]]
    rng = np.random.default_rng(8)
    X, Y, Z = np.meshgrid(*[(np.arange(nc[d]) + 0.5) / nc[d] for d in range(3)], indexing="ij")

    def smooth(seed):
        r = np.random.default_rng(seed)
        out = np.zeros(nc + (ncomp,))
        for n in range(ncomp):
            a, b, c = r.random(3)
            out[..., n] = np.sin(2 * np.pi * (X + a)) * np.cos(np.pi * (Y + b)) * np.sin(2 * np.pi * (Z + c)) + 0.3 * r.standard_normal(nc)
        return out
    Cold, Cnew = smooth(1), smooth(2)
    Fnew = rng.standard_normal(nf + (ncomp,))
    t_co, t_cn, time = 0.0, 1.0, 0.3
    g_c, g_f = orc.geom(nc, periodic=per), orc.geom(nf, periodic=per)
    cf = orc.Fab(nc, orc.CELL, 4, ncomp)
    cf.a[4:-4, 4:-4, 4:-4, :] = (t_cn - time) / (t_cn - t_co) * Cold + (time - t_co) / (t_cn - t_co) * Cnew
    L.orc_fill_periodic(cf.ref(), C.byref(g_c), orc.i3(orc.CELL))
    bcr = (orc.CBCRec * ncomp)()
    for n in range(ncomp):
        bcr[n].lo = (C.c_int * 3)(*bcs[n][0]); bcr[n].hi = (C.c_int * 3)(*bcs[n][1])
    el = (C.c_double * 9)(*[v for row in edlo for v in row]); eh = (C.c_double * 9)(*[v for row in edhi for v in row])
    L.orc_fill_physbc_cc(cf.ref(), C.byref(g_c), bcr, el, eh)
    vlo, vhi = (0, 0, 8), (15, 15, 23)
    ff = orc.Fab(nf, orc.CELL, 0, ncomp, lo=tuple(v - ng for v in vlo), hi=tuple(v + ng for v in vhi))
    ff.a[...] = -99.0
    ff.a[ng:-ng, ng:-ng, ng:-ng, :] = Fnew[vlo[0]:vhi[0] + 1, vlo[1]:vhi[1] + 1, vlo[2]:vhi[2] + 1]
    flo = [vlo[d] - ng if per[d] else max(vlo[d] - ng, 0) for d in range(3)]
    fhi = [vhi[d] + ng if per[d] else min(vhi[d] + ng, nf[d] - 1) for d in range(3)]
    L.orc_fill_coarse_fine(ff.ref(), orc.i3(flo), orc.i3(fhi), orc.i3(vlo), orc.i3(vhi), cf.ref(), orc.i3((0, 0, 0)), orc.i3(tuple(v - 1 for v in nc)),
                           orc.i3(per), ratio, bcr)
    L.orc_fill_physbc_cc(ff.ref(), C.byref(g_f), bcr, el, eh)
    ref = il.fillpatch_ref(orc, fboxes, ng, time, (None, Fnew, time, time), fboxes, (Cold, Cnew, t_co, t_cn), nc, ratio, per, bcs, edlo, edhi)
    for a, lo in ref.boxes:
        sl = tuple(slice(lo[d] - ff.lo[d], lo[d] - ff.lo[d] + a.shape[d]) for d in range(3))
        assert np.abs(a).max() < 50.0
        assert np.array_equal(a, ff.a[sl])
    # the numpy restatement of the limiter (the source of the bookkeeping) gives the oracle's interpolated values, bit for bit
    own = il.cellconslin_numpy(ref.book, ratio, ref.ff_lo, tuple(ref.ff_lo[d] + ref.ff.shape[d] - 1 for d in range(3)))
    assert ref.interp.sum() > 1000
    assert np.array_equal(own[ref.interp], ref.ff[ref.interp])


@pytest.mark.parametrize("ratio", [2, 4])
@pytest.mark.parametrize("typ", [(0, 0, 0), (1, 0, 0), (1, 1, 1)], ids=["cell", "facex", "node"])
def test_average_down_ref_within_the_sequential_sum_bound(ratio, typ):
    """n = r^3 (cells), r^2 (faces), 1 (nodes) children: |ref - fsum(children) w| <= (n - 1) 2^-53 sum|x| w, the bound of a sequential
    sum of n terms (the product with w, a power of two, is exact); a node is injected: equal"""
    nc = (4, 4, 4)
    rng = np.random.default_rng(5)
    F = rng.standard_normal(tuple(ratio * nc[d] + typ[d] for d in range(3)) + (2,))
    Cin = np.zeros(tuple(nc[d] + typ[d] for d in range(3)) + (2,))
    cbox = ((1, 0, 2), (3, 2, 3))
    out = il.average_down_ref(F, Cin, typ, [cbox], ratio, 1, 1)
    nchild = [1 if typ[d] else ratio for d in range(3)]
    n = nchild[0] * nchild[1] * nchild[2]
    w = 1.0 / n
    seen = 0
    for i in range(cbox[0][0], cbox[1][0] + 1 + typ[0]):
        for j in range(cbox[0][1], cbox[1][1] + 1 + typ[1]):
            for k in range(cbox[0][2], cbox[1][2] + 1 + typ[2]):
                ch = [F[ratio * i + a, ratio * j + b, ratio * k + c, 1] for c in range(nchild[2]) for b in range(nchild[1]) for a in range(nchild[0])]
                exact = math.fsum(ch) * w
                assert abs(out[i, j, k, 1] - exact) <= (n - 1) * 2.0 ** -53 * sum(abs(v) for v in ch) * w
                if n == 1:
                    assert out[i, j, k, 1] == ch[0]
                seen += 1
    assert seen == np.count_nonzero(out[..., 1]) and not out[..., 0].any()


def test_flux_register_ref_matches_the_existing_direct_evaluation():
    """FluxRegRef on the configuration of test_gpu_amr.test_flux_register_reflux_matches_direct_evaluation against that test's loops"""
    nc, ratio, ncomp = (16, 12, 8), 2, 2
    cboxes = [((0, 2, 2), (3, 9, 5)), ((4, 2, 2), (7, 9, 5))]
    rng = np.random.default_rng(6)
    nf = tuple(2 * v for v in nc)
    dt_c, dt_f, vol = 0.1, 0.05, 0.25
    CF, FF1, FF2 = [], [], []
    for d in range(3):
        sc = list(nc); sc[d] += 1
        sf = list(nf); sf[d] += 1
        c = rng.standard_normal(tuple(sc) + (ncomp,))
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[d] = 0; hi[d] = nc[d]
        c[tuple(hi)] = c[tuple(lo)]
        CF.append(c); FF1.append(rng.standard_normal(tuple(sf) + (ncomp,))); FF2.append(rng.standard_normal(tuple(sf) + (ncomp,)))
    fr = il.FluxRegRef(cboxes, nc, (1, 1, 1), ratio, ncomp)
    for d in range(3):
        fr.crse_init(CF[d], d, 0, 0, ncomp, -dt_c)
        fr.fine_add(FF1[d], d, 0, 0, ncomp, dt_f)
        fr.fine_add(FF2[d], d, 0, 0, ncomp, dt_f)
    S = np.zeros(nc + (ncomp,))
    fr.reflux(S, vol, 1.0, 0, 0, ncomp)
    exp = np.zeros(nc + (ncomp,))
    for (lo, hi) in cboxes:
        for d in range(3):
            d1, d2 = [e for e in range(3) if e != d]
            for side in (0, 1):
                face = lo[d] if side == 0 else hi[d] + 1
                out = (lo[d] - 1) % nc[d] if side == 0 else (hi[d] + 1) % nc[d]
                for a in range(lo[d1], hi[d1] + 1):
                    for b in range(lo[d2], hi[d2] + 1):
                        ci = [0, 0, 0]; ci[d] = face; ci[d1] = a; ci[d2] = b
                        fsum = np.zeros(ncomp)
                        for ra in range(2):
                            for rb in range(2):
                                fi = [0, 0, 0]; fi[d] = 2 * face; fi[d1] = 2 * a + ra; fi[d2] = 2 * b + rb
                                fsum += FF1[d][tuple(fi)] + FF2[d][tuple(fi)]
                        reg = -dt_c * CF[d][tuple(ci)] + dt_f * fsum
                        oc = [0, 0, 0]; oc[d] = out; oc[d1] = a; oc[d2] = b
                        exp[tuple(oc)] += (-1.0 if side == 0 else 1.0) * reg / vol
    assert np.abs(exp).max() > 0.5
    assert np.abs(S - exp).max() <= 1e-13


# ---------------------------------------------------------------------------------------------------------------------------
# input conditions
def _shares(ref, n, interp=None):
    interp = ref.interp if interp is None else interp
    zero = [ref.fine_of(ref.book["zeroed"][..., n, d])[interp].mean() for d in range(3)]
    cent = [ref.fine_of(ref.book["dc_used"][..., n, d] & ~ref.book["one_sided"][..., n, d])[interp].mean() for d in range(3)]
    return zero, cent


def _all_fill_cases():
    for d, side, ratio in il.WALL_CASES:
        yield f"wall-{d}-{side}-r{ratio}", il.wall_case(d, side, ratio)
    yield "corner", il.corner_case()
    for name, ng, ratio in il.LAYOUT_CASES:
        yield f"{name}-ng{ng}-r{ratio}", il.layout_case(name, ng, ratio)


ALL_FILL_CASES = dict(_all_fill_cases())


@pytest.mark.parametrize("name", list(ALL_FILL_CASES))
def test_input_conditions_of_the_fill_patch_cases(orc, name):
    """G components: at most half of the interpolated cells have a zeroed slope, per direction, and at least a quarter take the
    unlimited central slope.  K components: at least 40 coarse cells of the level with alpha < 1 (8^3 levels; the 12 x 8 x 8 level has
    more) and at least 8 of them under the case's interpolated cells.  W components (ext_dir and hoextrap at the touched wall): the
    one-sided slope is what the limiter passes in at least half of the wall-adjacent coarse cells that feed interpolated cells.
    All of it over the cells the case's call interpolates (FillPatchRef.interp: the ghost cells of its boxes that no fine data cover).
    Shares of the chosen data there: ext_dir 48/48 (ratio 2) and 20/20 (ratio 4); hoextrap 27/48 to 33/48 (ratio 2) and 11/20, 14/20
    (ratio 4).  With hoextrap the ghost value is the extrapolation to the wall itself, |dc| and the limiter's bound 2 (u0 - u_wall) agree
    for a straight ramp, and the noise decides cell by cell (interlevel_numpy.data_W): a field of this form gives one half on average,
    so the noise seeds of the wall cases (interlevel_numpy.WALL_SEEDS) are ones for which the condition holds."""
    case = ALL_FILL_CASES[name]
    ref = il.case_ref(orc, case)
    nc = case["nc"]
    dom = tuple(slice(2, 2 + nc[d]) for d in range(3))
    feeding = ref.feeding()
    assert ref.interp.sum() >= 200
    assert not (ref.ff == il.SENTINEL).any()
    for n, kind in enumerate(case["kinds"]):
        if kind == "G":
            zero, cent = _shares(ref, n)
            print(name, "G zeroed", zero, "central", cent)
            assert max(zero) <= 0.5 and min(cent) >= 0.25, (zero, cent)
        elif kind == "K":
            lt1 = ref.book["alpha_lt1"][..., n]
            print(name, "K alpha<1 in the level", lt1[dom].sum(), "feeding", (lt1 & feeding).sum(), "alpha", np.unique(ref.book["alpha"][..., n][lt1 & feeding])[:4])
            assert lt1[dom].sum() >= 40
            assert (lt1 & feeding).sum() >= 8
        elif kind == "W" and case["bcs"][n][case["wall"][1]][case["wall"][0]] in (il.BC_EXT_DIR, il.BC_HOEXTRAP):
            d, side = case["wall"]
            sl = [slice(None)] * 3
            sl[d] = 2 if side == 0 else 2 + nc[d] - 1
            adj = feeding[tuple(sl)]
            used = (ref.book["dc_used"][..., n, d] & ref.book["one_sided"][..., n, d])[tuple(sl)]
            print(name, "W comp", n, "one-sided slope used in", (used & adj).sum(), "of", adj.sum())
            assert adj.sum() >= 16 and (used & adj).sum() >= 0.5 * adj.sum()


def test_kinked_ramp_alpha_values(orc):
    """the excursion limiter's factor in the cells of the kink plane away from the periodic seam: 2/3 at ratio 2, 4/9 at ratio 4"""
    for ratio, val in ((2, 2.0 / 3.0), (4, 4.0 / 9.0)):
        ref = il.case_ref(orc, il.layout_case("one", 3, ratio))
        a = ref.book["alpha"][2:10, 2:10, 2:10, 1]
        I, J, K = np.meshgrid(*[np.arange(8)] * 3, indexing="ij")
        m = ((I + J + K == 10) | (I + J + K == 11)) & (I > 0) & (J > 0) & (K > 0) & (I < 7) & (J < 7) & (K < 7)
        assert m.sum() >= 20 and np.abs(a[m] - val).max() <= 4 * 2.0 ** -53
