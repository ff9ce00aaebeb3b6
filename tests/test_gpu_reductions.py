"""GPU: the level-wide reductions (iamr_amd/csrc/k_basic.hip: norm0, norm0_comps, minmax, owner-weighted dot products and sums; launch.h:
the functor reduction reduce_max_f with its host and device finish) against plain numpy, at the layouts, index types, ghost widths and
positions where a tiled two-stage reduction goes wrong; the one rule of every max norm (a NaN anywhere in the region read gives +inf, +-inf
gives +inf, wherever it sits); and what the solvers make of a NaN right-hand side and of bottom_maxiter 0 / 1.

Maxima are exact and compared with ==.  Sums are compared with math.fsum of the same weighted terms within 2 n eps fsum(|terms|).  Every
point of a fab that a call does not count holds a poison value (NaN or -DBL_MAX), so a reduction that reads outside its region fails."""
import itertools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DMAX = np.finfo(np.float64).max
SUB = 5e-324                       # smallest subnormal
PER, DIR, NEU = 0, 101, 102        # LinOpBC codes

CELL, NODE = (0, 0, 0), (1, 1, 1)
TYPES = [CELL, NODE, (1, 0, 0), (0, 1, 0), (0, 0, 1)]


def _box(lo, hi):
    return (tuple(lo), tuple(hi))


# name -> (domain, boxes)
LAYOUTS = {
    "1x1x1": ((1, 1, 1), [_box((0, 0, 0), (0, 0, 0))]),
    "2x3x5": ((2, 3, 5), [_box((0, 0, 0), (1, 2, 4))]),
    "33x9x17": ((33, 9, 17), [_box((0, 0, 0), (32, 8, 16))]),
    "65x64x1": ((65, 64, 1), [_box((0, 0, 0), (64, 63, 0))]),
    "31x33x70": ((31, 33, 70), [_box((0, 0, 0), (30, 32, 69))]),
    # plain tiling: equal boxes
    "4equal": ((32, 32, 16), [_box((i, j, 0), (i + 15, j + 15, 15)) for j in (0, 16) for i in (0, 16)]),
    # unequal boxes, one-cell boxes among them: the flat tile list (launch.h level_tiling)
    "unequal": ((20, 12, 10), [_box((0, 0, 0), (15, 11, 9)), _box((16, 0, 0), (19, 5, 9)), _box((16, 6, 0), (19, 11, 8)),
                               _box((16, 6, 9), (16, 6, 9)), _box((16, 7, 9), (16, 11, 9)), _box((17, 6, 9), (19, 11, 9))]),
    # an L-shaped level that does not cover its domain
    "L": ((16, 16, 16), [_box((0, 0, 0), (7, 15, 7)), _box((8, 0, 0), (15, 7, 7))]),
}


class Field:
    """a global numpy field G (index origin glo) loaded into a MultiFab; points of a fab outside the region a call counts (its box converted
    to the type, grown by ng_count) hold `poison` instead"""

    def __init__(self, lib, lay, typ, nc, ng_alloc, ng_count, G, glo, poison):
        self.mf = lib.MultiFab(lay, typ, nc, ng_alloc)
        self.G, self.glo = G, glo
        self.fabs, self.host = [], []
        for li in range(self.mf.nlocal()):
            flo, fhi = self.mf.fab_box(li)
            blo, bhi, _ = lay.local_box(li)
            rlo = tuple(blo[d] - ng_count for d in range(3))
            rhi = tuple(bhi[d] + typ[d] + ng_count for d in range(3))
            a = np.array(G[tuple(slice(flo[d] - glo[d], fhi[d] - glo[d] + 1) for d in range(3))], order="F")
            keep = np.zeros(a.shape[:3], bool)
            keep[tuple(slice(rlo[d] - flo[d], rhi[d] - flo[d] + 1) for d in range(3))] = True
            a[~keep] = poison
            self.fabs.append((flo, rlo, rhi))
            self.host.append(a)
            self.mf.from_numpy(a, li)

    def regions(self):
        return [(rlo, rhi) for _, rlo, rhi in self.fabs]

    def counted(self):
        """values of every counted point (with repetitions where regions overlap), (npts, nc)"""
        v = [self.G[tuple(slice(rlo[d] - self.glo[d], rhi[d] - self.glo[d] + 1) for d in range(3))].reshape(-1, self.G.shape[3])
             for rlo, rhi in self.regions()]
        return np.concatenate(v)

    def poke(self, p, comp, val):
        """G[p, comp] = val at a counted point p, in every fab that counts p; returns the old value"""
        q = tuple(p[d] - self.glo[d] for d in range(3)) + (comp,)
        old = self.G[q]
        self.G[q] = val
        for li, (flo, rlo, rhi) in enumerate(self.fabs):
            if all(rlo[d] <= p[d] <= rhi[d] for d in range(3)):
                self.host[li][tuple(p[d] - flo[d] for d in range(3)) + (comp,)] = val
                self.mf.from_numpy(self.host[li], li)
        return old


def _global(n, typ, nc, ng, rng, neg=False):
    shape = tuple(n[d] + typ[d] + 2 * ng for d in range(3)) + (nc,)
    G = rng.uniform(-1.0, 1.0, shape)
    if neg:
        G = -1.0 - np.abs(G)
    return np.asfortranarray(G), (-ng, -ng, -ng)


def _ref_norm(vals):
    """the rule: |v| per point, NaN -> +inf"""
    a = np.abs(vals)
    a[np.isnan(a)] = np.inf
    return a.max(axis=0)


def _ref_minmax(v):
    if np.isnan(v).any():
        return -np.inf, np.inf
    return v.min(), v.max()


def _probe_points(f):
    """where an extreme is moved: two opposite corners and two more of every counted region (first / last tile in x and y, the last k of
    the last chunk, the hi+1 node plane, counted ghost points, the last box); in the first and the last region lane 63 and the first
    lanes of the next waves of a 64-wide row, and a middle point"""
    regs = f.regions()
    pts = []
    for r, (rlo, rhi) in enumerate(regs):
        pts += [rlo, rhi, (rhi[0], rlo[1], rlo[2]), (rlo[0], rhi[1], rhi[2])]
        if r in (0, len(regs) - 1):
            for off in ((63, 0, 0), (64, 0, 0), (0, 1, 0), (5, 2, 1)):
                pts.append(tuple(min(rlo[d] + off[d], rhi[d]) for d in range(3)))
            pts.append(tuple((rlo[d] + rhi[d]) // 2 for d in range(3)))
    return list(dict.fromkeys(pts))


def _layout(lib, name):
    n, boxes = LAYOUTS[name]
    return n, lib.Layout(boxes)


def _norms(f, comp, nc, ng):
    mf = f.mf
    got = {"norm0": [mf.norm0(comp, nc, ng)]}
    got["comps0"] = mf.norm0_comps(comp, nc, ng, form=0)
    if nc in (1, 3, 6):
        got["comps1"] = mf.norm0_comps(comp, nc, ng, form=1)
        got["comps2"] = mf.norm0_comps(comp, nc, ng, form=2)
    return got


def _check_norms(f, comp, nc, ng, tag):
    ref = _ref_norm(f.counted()[:, comp:comp + nc])
    got = _norms(f, comp, nc, ng)
    assert got["norm0"][0] == ref.max(), (tag, "norm0", got["norm0"], ref.max())
    for k in ("comps0", "comps1", "comps2"):
        if k in got:
            assert got[k] == list(ref), (tag, k, got[k], list(ref))


def _check_minmax(f, comp, ng, tag):
    mn, mx = f.mf.minmax(comp, ng)
    rmn, rmx = _ref_minmax(f.counted()[:, comp])
    assert (mn, mx) == (rmn, rmx), (tag, (mn, mx), (rmn, rmx))


def _mapped(val):
    return np.inf if np.isnan(val) else abs(val)


@pytest.mark.parametrize("name", list(LAYOUTS) + ["unequal-notilelist"])
def test_max_norms_and_minmax_against_numpy(gpu, name):
    """norm0, norm0_comps (three forms) and minmax on every index type and ghost width 0 ... 2, component offsets > 0; one extreme (-7.5,
    NaN, +-inf; the field lies in (-1, 1)) moved through the layout"""
    lib = gpu
    lname = "unequal" if name == "unequal-notilelist" else name
    n, lay = _layout(lib, lname)
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "unequal-notilelist":
        lib.tuning_set("TILE_LISTS", 0)
    try:
        for ti, typ in enumerate(TYPES):
            probe_ng = (1, 2, 0, 1, 2)[ti]
            for ng in (0, 1, 2):
                nc = 7
                G, glo = _global(n, typ, nc, ng + 1, rng)
                poison = np.nan if (ti + ng) % 2 == 0 else -DMAX
                f = Field(lib, lay, typ, nc, ng + 1, ng, G, glo, poison)
                tag = (name, typ, ng)
                for comp, ncomp in ((0, 1), (1, 6), (2, 3), (3, 4)):
                    _check_norms(f, comp, ncomp, ng, tag)
                _check_minmax(f, 2, ng, tag)
                if ng != probe_ng:
                    continue
                base = _ref_norm(f.counted())
                V2 = f.counted()[:, 2]
                for p in _probe_points(f):
                    # the extreme in component 4: (1, 6) sees it, (0, 1) must not
                    for val in (-7.5, np.nan, np.inf, -np.inf):
                        old = f.poke(p, 4, val)
                        want = list(base[1:7]); want[3] = _mapped(val)
                        got = _norms(f, 1, 6, ng)
                        assert got["norm0"] == [max(want)] and got["comps0"] == want and got["comps1"] == want and got["comps2"] == want, \
                            (tag, p, val, got, want)
                        assert f.mf.norm0_comps(0, 1, ng, form=1) == [base[0]], (tag, p, val)
                        f.poke(p, 4, old)
                    # the extreme in component 2: minmax and the (2, 3) norms
                    old = f.G[tuple(p[d] - glo[d] for d in range(3)) + (2,)]
                    rest = V2[V2 != old]
                    for val in (-7.5, 7.5, np.nan, -np.inf):
                        f.poke(p, 2, val)
                        want = list(base[2:5]); want[0] = _mapped(val)
                        got = _norms(f, 2, 3, ng)
                        assert got["comps0"] == want and got["comps1"] == want and got["comps2"] == want, (tag, p, val, got, want)
                        mm = f.mf.minmax(2, ng)
                        wmm = (-np.inf, np.inf) if np.isnan(val) else (min(val, rest.min()), max(val, rest.max()))
                        assert mm == wmm, (tag, p, val, mm, wmm)
                        f.poke(p, 2, old)
    finally:
        lib.tuning_set("TILE_LISTS", 1)


@pytest.mark.parametrize("name", ["2x3x5", "unequal", "L"])
def test_max_norms_at_the_ends_of_the_double_range(gpu, name):
    """-0.0, subnormals and values near +-DBL_MAX; an all-negative field for minmax"""
    lib = gpu
    n, lay = _layout(lib, name)
    rng = np.random.default_rng(7)
    for typ in (CELL, NODE, (0, 1, 0)):
        ng = 1
        G, glo = _global(n, typ, 3, ng + 1, rng)
        G[..., 0] *= SUB * 8                       # subnormal magnitudes
        G[..., 1] = -0.0
        G[..., 2] = np.sign(G[..., 2]) * DMAX * (1.0 - np.abs(G[..., 2]) * 1e-10)
        f = Field(lib, lay, typ, 3, ng + 1, ng, G, glo, np.nan)
        _check_norms(f, 0, 3, ng, (name, typ))
        _check_norms(f, 0, 1, ng, (name, typ))
        for c in range(3):
            _check_minmax(f, c, ng, (name, typ, c))
        p = f.regions()[-1][1]
        for val in (DMAX, -DMAX, SUB, -SUB):
            old = f.poke(p, 0, val)
            _check_norms(f, 0, 1, ng, (name, typ, val))
            _check_minmax(f, 0, ng, (name, typ, val))
            f.poke(p, 0, old)
        G2, _ = _global(n, typ, 1, ng + 1, rng, neg=True)
        G2[G2.shape[0] // 2, 0, 0, 0] = -DMAX
        f2 = Field(lib, lay, typ, 1, ng + 1, ng, G2, glo, np.nan)
        _check_minmax(f2, 0, ng, (name, typ, "negative"))
        _check_norms(f2, 0, 1, ng, (name, typ, "negative"))


# ---------------------------------------------------------------------------------------------------------------- owner-weighted sums
def _weights(n, boxes, typ, per, lobc, hibc):
    """the documented rule, restated: every point counted once; the hi+1 point of a box in a nodal direction belongs to its neighbour or
    periodic image (weight 0 here), except on a non-periodic domain face; a hi+1 point with no such neighbour (coarse/fine face of a level
    that does not cover the domain) counts nowhere; weight 1/2 per Neumann wall a node lies on"""
    W = np.zeros(tuple(n[d] + typ[d] for d in range(3)))
    for lo, hi in boxes:
        top = [hi[d] + (1 if (typ[d] and not per[d] and hi[d] == n[d] - 1) else 0) for d in range(3)]
        W[lo[0]:top[0] + 1, lo[1]:top[1] + 1, lo[2]:top[2] + 1] = 1.0
    for d in range(3):
        if not typ[d] or per[d]:
            continue
        sl = [slice(None)] * 3
        if lobc[d] == NEU:
            sl[d] = 0
            W[tuple(sl)] *= 0.5
        if hibc[d] == NEU:
            sl[d] = n[d]
            W[tuple(sl)] *= 0.5
    return W


def _check_sum(got, terms, tag):
    ref = math.fsum(terms)
    tol = 2 * max(len(terms), 1) * np.finfo(float).eps * math.fsum(np.abs(terms))
    assert abs(got - ref) <= tol, (tag, got, ref, tol)


def _valid_field(lib, lay, typ, nc, G):
    """valid points from G (consistent values where boxes share points), ghosts poisoned"""
    m = lib.MultiFab(lay, typ, nc, 1)
    for li in range(m.nlocal()):
        flo, fhi = m.fab_box(li)
        blo, bhi, _ = lay.local_box(li)
        a = np.full(tuple(fhi[d] - flo[d] + 1 for d in range(3)) + (nc,), np.nan, order="F")
        a[tuple(slice(blo[d] - flo[d], bhi[d] + typ[d] - flo[d] + 1) for d in range(3))] = \
            G[tuple(slice(blo[d], bhi[d] + typ[d] + 1) for d in range(3))]
        m.from_numpy(a, li)
    return m


BC_CHOICES = {"P": (1, PER, PER), "N": (0, NEU, NEU), "D": (0, DIR, DIR), "ND": (0, NEU, DIR), "DN": (0, DIR, NEU)}
T_JUNCTION = ((16, 16, 8), [_box((0, 0, 0), (7, 15, 7)), _box((8, 0, 0), (15, 7, 7)), _box((8, 8, 0), (15, 15, 7))])


def _sum_cases():
    """every choice per direction for node data; for face data every choice in the face's own direction; cell data twice"""
    for bcs in itertools.product(["P", "N", "D", "ND"], repeat=3):
        yield NODE, bcs
    for d in range(3):
        for c in BC_CHOICES:
            bcs = ["ND", "DN", "P"]
            bcs[d] = c
            yield tuple(int(q == d) for q in range(3)), tuple(bcs)
    yield CELL, ("P", "P", "P")
    yield CELL, ("N", "D", "ND")


@pytest.mark.parametrize("level", ["T", "L"])
def test_owner_weighted_dots_and_sums_against_numpy(gpu, level):
    """dot (one and two products, host and device finish) and sum_unique for every periodic / Neumann / Dirichlet choice per direction,
    node, face and cell data, on a 3-box layout with a T-junction and on an L-shaped level that does not cover the domain"""
    lib = gpu
    n, boxes = T_JUNCTION if level == "T" else LAYOUTS["L"]
    lay = lib.Layout(boxes)
    rng = np.random.default_rng(3)
    ncase = 0
    for typ in TYPES:
        nc = 2
        shape = tuple(n[d] + typ[d] for d in range(3)) + (nc,)
        X = [np.asfortranarray(rng.uniform(-1, 1, shape)) for _ in range(4)]
        mf = [_valid_field(lib, lay, typ, nc, x) for x in X]
        for t2, bcs in _sum_cases():
            if t2 != typ:
                continue
            per = tuple(BC_CHOICES[b][0] for b in bcs)
            lobc = tuple(BC_CHOICES[b][1] for b in bcs)
            hibc = tuple(BC_CHOICES[b][2] for b in bcs)
            g = lib.Geom.make(n, periodic=per)
            W = _weights(n, boxes, typ, per, lobc, hibc)[..., None]
            tag = (level, typ, bcs)
            for comp, ncomp in ((0, 2), (1, 1)):
                sl = slice(comp, comp + ncomp)
                t0 = (W * X[0][..., sl] * X[1][..., sl]).ravel()
                t1 = (W * X[2][..., sl] * X[3][..., sl]).ravel()
                for dev in (0, 1):
                    d1 = lib.dot(g, mf[0], mf[1], comp=comp, ncomp=ncomp, on_device=dev, lobc=lobc, hibc=hibc)
                    _check_sum(d1, t0, tag + ("dot1", comp, dev))
                    d2 = lib.dot(g, mf[0], mf[1], mf[2], mf[3], comp=comp, ncomp=ncomp, on_device=dev, lobc=lobc, hibc=hibc)
                    _check_sum(d2[0], t0, tag + ("dot2[0]", comp, dev))
                    _check_sum(d2[1], t1, tag + ("dot2[1]", comp, dev))
            for comp in (0, 1):
                s = lib.sum_unique(g, mf[0], comp, lobc=lobc, hibc=hibc)
                _check_sum(s, (W[..., 0] * X[0][..., comp]).ravel(), tag + ("sum_unique", comp))
            ncase += 1
    assert ncase == 64 + 3 * 5 + 2


@pytest.mark.parametrize("name", ["1x1x1", "33x9x17", "unequal", "unequal-notilelist"])
def test_sums_on_tile_edge_layouts(gpu, name):
    """dot and sum_unique where the tiles end: partial x / y tiles, k-chunk tails, one-cell boxes, the flat tile list and the plain grid"""
    lib = gpu
    lname = "unequal" if name == "unequal-notilelist" else name
    n, boxes = LAYOUTS[lname]
    lay = lib.Layout(boxes)
    rng = np.random.default_rng(5)
    if name == "unequal-notilelist":
        lib.tuning_set("TILE_LISTS", 0)
    try:
        for typ in TYPES:
            for per, bc in (((1, 1, 1), PER), ((0, 0, 0), NEU)):
                g = lib.Geom.make(n, periodic=per)
                shape = tuple(n[d] + typ[d] for d in range(3)) + (1,)
                X = [np.asfortranarray(rng.uniform(-1, 1, shape)) for _ in range(2)]
                mf = [_valid_field(lib, lay, typ, 1, x) for x in X]
                W = _weights(n, boxes, typ, per, (bc,) * 3, (bc,) * 3)
                tag = (name, typ, per)
                for dev in (0, 1):
                    _check_sum(lib.dot(g, mf[0], mf[1], on_device=dev, lobc=(bc,) * 3, hibc=(bc,) * 3),
                               (W * X[0][..., 0] * X[1][..., 0]).ravel(), tag + (dev,))
                _check_sum(lib.sum_unique(g, mf[0], 0, lobc=(bc,) * 3, hibc=(bc,) * 3), (W * X[0][..., 0]).ravel(), tag)
    finally:
        lib.tuning_set("TILE_LISTS", 1)


# ---------------------------------------------------------------------------------------------------------------- solver consequences
def _nodal_problem(lib, walls, rng):
    n = (16, 16, 16)
    per = (0, 0, 0) if walls else (1, 1, 1)
    bc = (NEU,) * 3 if walls else (PER,) * 3
    g = lib.Geom.make(n, periodic=per)
    lay = lib.Layout.single(n)
    sig = lib.MultiFab(lay, CELL, 1, 1); sig.setval(1.0)
    rhs = lib.MultiFab(lay, NODE, 1, 0)
    R = rng.uniform(-1, 1, (17, 17, 17, 1))
    if not walls:
        R[16, :, :] = R[0, :, :]; R[:, 16, :] = R[:, 0, :]; R[:, :, 16] = R[:, :, 0]
    rhs.set_from_global(np.asfortranarray(R), (0, 0, 0))
    phi = lib.MultiFab(lay, NODE, 1, 1); phi.setval(0.0)
    return g, lay, sig, rhs, phi, bc, R


def _accepts_nan(st, phi, tag):
    assert st.converged == 0, (tag, "a NaN right-hand side reported as converged", st.converged, st.resnorm0, st.resnorm)


@pytest.mark.parametrize("walls", [False, True])
def test_nodal_solve_does_not_converge_on_a_nan_rhs(gpu, walls):
    lib = gpu
    from iamr_amd import ns as N
    rng = np.random.default_rng(11)
    for dev_bottom, krylov_dev in itertools.product((0, 1), (0, 1)):
        g, lay, sig, rhs, phi, bc, R = _nodal_problem(lib, walls, rng)
        R[5, 6, 7, 0] = np.nan
        rhs.set_from_global(np.asfortranarray(R), (0, 0, 0))
        lib.tuning_set("KRYLOV_DEVICE", krylov_dev)
        try:
            st = N.nodal_solve(g, phi, rhs, sig, 0, bc, bc, 1e-10, 0.0, lib.mg_opts(device_bottom=dev_bottom, max_iters=8))
        except lib.IamrxError:
            continue
        finally:
            lib.tuning_set("KRYLOV_DEVICE", 1)
        _accepts_nan(st, phi, (walls, dev_bottom, krylov_dev))


def test_mac_solve_does_not_converge_on_a_nan_rhs(gpu):
    lib = gpu
    n = (16, 16, 16)
    g = lib.Geom.make(n)
    lay = lib.Layout.single(n)
    um = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 1); m.setval(0.0)
        um.append(m)
    rho = lib.MultiFab(lay, CELL, 1, 1); rho.setval(1.0)
    S = lib.MultiFab(lay, CELL, 1, 0)
    A = np.random.default_rng(2).uniform(-1, 1, n + (1,))
    A -= A.mean()
    A[3, 9, 15, 0] = np.nan
    S.set_from_global(np.asfortranarray(A), (0, 0, 0))
    phi = lib.MultiFab(lay, CELL, 1, 1); phi.setval(0.0)
    for db in (0, 1):
        try:
            st = lib.mlmg_mac_solve(g, um, rho, 0, S, phi, 1.0, opts=lib.mg_opts(maxorder=4, device_bottom=db, max_iters=8))
        except lib.IamrxError:
            continue
        _accepts_nan(st, phi, ("mac", db))


@pytest.mark.parametrize("maxiter", [0, 1])
def test_bottom_maxiter_device_and_host_driven_krylov_agree(gpu, maxiter):
    """bottom_maxiter 0 and 1: the device-resident BiCGStab (krylov.h) gives the MGStats and the phi of the host-driven loop, cell-centred
    and nodal (device_bottom = 0: the hierarchies end in BiCGStab)"""
    lib = gpu
    from iamr_amd import ns as N
    n = (16, 16, 16)
    rng = np.random.default_rng(13)
    g = lib.Geom.make(n)
    lay = lib.Layout.single(n)
    b = []
    for d in range(3):
        m = lib.MultiFab(lay, lib.face(d), 1, 0); m.setval(1.0)
        b.append(m)
    rhs_c = rng.uniform(-1, 1, n + (1,)); rhs_c -= rhs_c.mean()
    rhs_d = lib.MultiFab(lay, CELL, 1, 0); rhs_d.set_from_global(np.asfortranarray(rhs_c), (0, 0, 0))
    out = {}
    for dev in (1, 0):
        lib.tuning_set("KRYLOV_DEVICE", dev)
        try:
            o = lib.mg_opts(device_bottom=0, min_width=8, bottom_maxiter=maxiter, fixed_iters=3)
            phi = lib.MultiFab(lay, CELL, 1, 1); phi.setval(0.0)
            st = lib.abec_solve(g, 0.0, 1.0, None, b, phi, rhs_d, rtol=1e-11, atol=0.0, opts=o)
            cell = ((st.iters, st.bottom_iters_total, st.converged, st.resnorm0, st.resnorm), phi.gather_valid(n)[..., 0])
            gn, _, sig, rhs, phin, bc, _ = _nodal_problem(lib, False, np.random.default_rng(17))
            o = lib.mg_opts(device_bottom=0, bottom_maxiter=maxiter, fixed_iters=3)
            stn = N.nodal_solve(gn, phin, rhs, sig, 0, bc, bc, 1e-11, 0.0, o)
            nodal = ((stn.iters, stn.bottom_iters_total, stn.converged, stn.resnorm0, stn.resnorm), phin.gather_valid(n)[..., 0])
        finally:
            lib.tuning_set("KRYLOV_DEVICE", 1)
        out[dev] = (cell, nodal)
    # (the same operations on the same doubles; the compiler may order a kernel's independent loads differently: test_gpu_krylov.py)
    for q, what in enumerate(("cell", "nodal")):
        s0, p0 = out[0][q]
        s1, p1 = out[1][q]
        assert s0[:4] == s1[:4], (what, maxiter, s0, s1)
        assert abs(s0[4] - s1[4]) <= 1e-12 * s0[3], (what, maxiter, s0, s1)
        assert np.abs(p0 - p1).max() <= 1e-13 * np.abs(p0).max(), (what, maxiter, float(np.abs(p0 - p1).max()))
