"""References of the inter-level transfer operators (iamr_amd/csrc/amr.hip: fillpatch_two_levels, FluxRegister, average_down,
create_umac_grown) for tests/test_cpu_interlevel_ref.py and tests/test_gpu_interlevel.py.  A plain helper module, no fixtures.

Every reference restates the product's expressions in the product's order (amr.hip is built with -ffp-contract=off), so the tests
can ask for bit equality.  Data come as GLOBAL numpy arrays over a level's index space ((nx, ny, nz, ncomp), cells / faces / nodes
of the whole domain); a level's boxes say which part of a fine array exists.  Boxes are ((lo), (hi)) cell boxes, inclusive.

  fillpatch_ref      : the cell-conservative-linear fill of any fine layout, built from the CPU oracle's orc_fill_periodic,
                       orc_fill_physbc_cc and orc_fill_coarse_fine; + the limiter's bookkeeping recomputed in numpy (limiter_book)
  FluxRegRef         : CrseInit / FineAdd / Reflux evaluated directly per fine box
  average_down_ref   : mean of the children (cell-like directions), injection (nodal directions)
  umac_grown_ref     : FaceLinear ghost faces + sibling / image overlay + level mask + divergence fix, per box
"""
import ctypes as C
import itertools
import numpy as np

SENTINEL = -7.0e30
BC_REFLECT_ODD, BC_INT_DIR, BC_REFLECT_EVEN, BC_FOEXTRAP, BC_EXT_DIR, BC_HOEXTRAP = -1, 0, 1, 2, 3, 4


def shifts(per, n):
    """index shifts of the periodic images of a domain of n cells (the zero shift included)"""
    rng = [(-n[d], 0, n[d]) if per[d] else (0,) for d in range(3)]
    return list(itertools.product(*rng))


def box_slices(lo, hi, origin):
    return tuple(slice(lo[d] - origin[d], hi[d] - origin[d] + 1) for d in range(3))


def intersect(alo, ahi, blo, bhi):
    lo = tuple(max(alo[d], blo[d]) for d in range(3))
    hi = tuple(min(ahi[d], bhi[d]) for d in range(3))
    return (lo, hi) if all(lo[d] <= hi[d] for d in range(3)) else None


def time_interp(td, time):
    """StateData time interpolation of amr.hip (time_interp): td = (old or None, new, t_old, t_new) of numpy arrays"""
    old, new, t_old, t_new = td
    if old is None or old is new:
        return new
    eps = 1.e-3 * abs(t_new - t_old)
    if abs(time - t_new) <= eps:
        return new
    if abs(time - t_old) <= eps:
        return old
    a = (t_new - time) / (t_new - t_old)
    b = (time - t_old) / (t_new - t_old)
    return a * old + b * new


# ---------------------------------------------------------------------------------------------------------------------------
# fill-patch
def coarse_fab(orc, crse, nc, per, bcs, edlo, edhi):
    """the coarse data (nc + (ncomp,)) with 4 ghost cells: periodic images, then the physical BC of the coarse domain"""
    L = orc.lib()
    ncomp = crse.shape[3]
    cf = orc.Fab(nc, orc.CELL, 4, ncomp)
    cf.a[4:-4, 4:-4, 4:-4, :] = crse
    g_c = orc.geom(nc, periodic=per)
    L.orc_fill_periodic(cf.ref(), C.byref(g_c), orc.i3(orc.CELL))
    bcr, el, eh = _bc_args(orc, ncomp, bcs, edlo, edhi)
    L.orc_fill_physbc_cc(cf.ref(), C.byref(g_c), bcr, el, eh)
    return cf


def _bc_args(orc, ncomp, bcs, edlo, edhi):
    bcr = (orc.CBCRec * ncomp)()
    for n in range(ncomp):
        lo, hi = bcs[n] if bcs is not None else ((0, 0, 0), (0, 0, 0))
        bcr[n].lo = (C.c_int * 3)(*lo)
        bcr[n].hi = (C.c_int * 3)(*hi)
    flat = lambda e: (C.c_double * (3 * ncomp))(*([float(v) for row in e for v in row] if e is not None else [0.0] * (3 * ncomp)))
    return bcr, flat(edlo), flat(edhi)


class FillPatchRef:
    """result of fillpatch_ref: .boxes[i] = (array over dst box i grown by ng, lo), .ff / .ff_lo the global fine array (domain grown by
    ng in the periodic directions), .interp the cells of it that the call interpolates (inside a destination box grown by ng, and
    covered by no fine box or image), .book the limiter's
    bookkeeping on the coarse cells (limiter_book), .ratio"""

    def fine_of(self, carr):
        """a coarse-cell array of the bookkeeping (origin -2) expanded to the cells of .ff"""
        r = self.ratio
        idx = [np.arange(self.ff_lo[d], self.ff_lo[d] + self.ff.shape[d]) // r + 2 for d in range(3)]
        return carr[np.ix_(*idx)]

    def feeding(self):
        """coarse cells (origin -2, shape of the bookkeeping) that hold at least one interpolated fine cell"""
        out = np.zeros(self.book["alpha_lt1"].shape[:3], bool)
        w = np.argwhere(self.interp)
        c = (w + np.array(self.ff_lo)) // self.ratio + 2
        out[c[:, 0], c[:, 1], c[:, 2]] = True
        return out


def fillpatch_ref(orc, dst_boxes, ng, time, fine_td, fine_boxes, crse_td, nc, ratio, per, bcs=None, edlo=None, edhi=None):
    """fine_td / crse_td: (old or None, new, t_old, t_new) of global arrays that hold exactly the components to fill"""
    L = orc.lib()
    nf = tuple(ratio * v for v in nc)
    crse = time_interp(crse_td, time)
    ncomp = crse.shape[3]
    cf = coarse_fab(orc, crse, nc, per, bcs, edlo, edhi)
    bcr, el, eh = _bc_args(orc, ncomp, bcs, edlo, edhi)
    if bcs is None:
        bcs = [((0, 0, 0), (0, 0, 0))] * ncomp
    flo = tuple(-ng if per[d] else 0 for d in range(3))
    fhi = tuple(nf[d] - 1 + (ng if per[d] else 0) for d in range(3))
    ff = orc.Fab(nf, orc.CELL, 0, ncomp, lo=flo, hi=fhi)
    ff.a[...] = SENTINEL
    L.orc_fill_coarse_fine(ff.ref(), orc.i3(flo), orc.i3(fhi), orc.i3((0, 0, 0)), orc.i3((-1, -1, -1)), cf.ref(), orc.i3((0, 0, 0)),
                           orc.i3(tuple(v - 1 for v in nc)), orc.i3(per), ratio, bcr)
    interp = np.ones(ff.a.shape[:3], bool)
    if fine_boxes:
        fine = time_interp(fine_td, time)
        for blo, bhi in fine_boxes:
            for sh in shifts(per, nf):
                q = intersect(tuple(blo[d] + sh[d] for d in range(3)), tuple(bhi[d] + sh[d] for d in range(3)), flo, fhi)
                if q is None:
                    continue
                src = box_slices(tuple(q[0][d] - sh[d] for d in range(3)), tuple(q[1][d] - sh[d] for d in range(3)), (0, 0, 0))
                ff.a[box_slices(q[0], q[1], flo)] = fine[src]
                interp[box_slices(q[0], q[1], flo)] = False
    g_f = orc.geom(nf, periodic=per)
    out = FillPatchRef()
    out.boxes = []
    for blo, bhi in dst_boxes:
        lo = tuple(v - ng for v in blo)
        hi = tuple(v + ng for v in bhi)
        fab = orc.Fab(nf, orc.CELL, 0, ncomp, lo=lo, hi=hi)
        fab.a[...] = SENTINEL
        q = intersect(lo, hi, flo, fhi)
        fab.a[box_slices(q[0], q[1], lo)] = ff.a[box_slices(q[0], q[1], flo)]
        L.orc_fill_physbc_cc(fab.ref(), C.byref(g_f), bcr, el, eh)
        out.boxes.append((fab.a, lo))
    # the cells a call interpolates: inside a destination box grown by ng (and inside the periodically extended domain), not covered
    wanted = np.zeros(interp.shape, bool)
    for blo, bhi in dst_boxes:
        q = intersect(tuple(v - ng for v in blo), tuple(v + ng for v in bhi), flo, fhi)
        wanted[box_slices(q[0], q[1], flo)] = True
    interp &= wanted
    out.ff, out.ff_lo, out.interp, out.ratio = ff.a, flo, interp, ratio
    out.book = limiter_book(cf.a, nc, per, bcs, ratio)
    return out


def limiter_book(ca, nc, per, bcs, ratio):
    """amrex::CellConservativeLinear (per-component limiter) on the coarse cells [-2, n+1]^3 of a coarse fab with 4 ghost cells
    (origin -4), in the order of k_cellconslin / orc_fill_coarse_fine.  Returns arrays of shape (n+4, n+4, n+4, ncomp[, 3]), origin -2:
      zeroed[..., d]   the limited slope of direction d is zero
      dc_used[..., d]  |dc| <= the limiter's bound and the slope is not zero: dc itself is the slope
      one_sided[..., d] dc is the four-point one-sided formula (cell next to an ext_dir / hoextrap face)
      alpha_lt1        the excursion limiter fired,  alpha  its factor,  slope[..., d]  the limited slope, u0  the coarse value"""
    ncomp = ca.shape[3]
    core = tuple(slice(2, ca.shape[d] - 2) for d in range(3))
    shape = tuple(ca.shape[d] - 4 for d in range(3))

    def sh(off):
        return ca[tuple(slice(2 + off[d], ca.shape[d] - 2 + off[d]) for d in range(3))]
    u0 = ca[core]
    sl = np.zeros(shape + (ncomp, 3))
    dcs = np.zeros(shape + (ncomp, 3))
    sms = np.zeros(shape + (ncomp, 3))
    one = np.zeros(shape + (ncomp, 3), bool)
    for d in range(3):
        e = lambda m: tuple(m if q == d else 0 for q in range(3))
        um, up, umm, upp = sh(e(-1)), sh(e(1)), sh(e(-2)), sh(e(2))
        dc = 0.5 * (up - um)
        idx = np.arange(-2, nc[d] + 2).reshape([-1 if q == d else 1 for q in range(3)] + [1])
        lo_f = -16. / 15. * um + 0.5 * u0 + 2. / 3. * up - 0.1 * upp
        hi_f = 16. / 15. * up - 0.5 * u0 - 2. / 3. * um + 0.1 * umm
        for n in range(ncomp):
            blo, bhi = (BC_INT_DIR, BC_INT_DIR) if per[d] else (bcs[n][0][d], bcs[n][1][d])
            if blo in (BC_EXT_DIR, BC_HOEXTRAP):
                m = np.broadcast_to(idx == 0, shape + (1,))[..., 0]
                dc[..., n] = np.where(m, lo_f[..., n], dc[..., n]); one[..., n, d] |= m
            if bhi in (BC_EXT_DIR, BC_HOEXTRAP):
                m = np.broadcast_to(idx == nc[d] - 1, shape + (1,))[..., 0]
                dc[..., n] = np.where(m, hi_f[..., n], dc[..., n]); one[..., n, d] |= m
        df, db = 2.0 * (up - u0), 2.0 * (u0 - um)
        sm = np.where(df * db >= 0.0, np.minimum(np.abs(df), np.abs(db)), 0.0)
        sl[..., d] = np.copysign(1.0, dc) * np.minimum(sm, np.abs(dc))
        dcs[..., d], sms[..., d] = dc, sm
    exc = float(ratio - 1) / float(2 * ratio)
    dumax = np.abs(sl[..., 0]) * exc + np.abs(sl[..., 1]) * exc + np.abs(sl[..., 2]) * exc
    umax, umin = u0.copy(), u0.copy()
    for ko in (-1, 0, 1):
        for jo in (-1, 0, 1):
            for io in (-1, 0, 1):
                v = sh((io, jo, ko))
                umin = np.minimum(umin, v); umax = np.maximum(umax, v)
    alpha = np.ones(shape + (ncomp,))
    any_sl = (sl != 0.0).any(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(any_sl & (dumax * alpha > (umax - u0)), (umax - u0) / dumax, alpha)
        alpha = np.where(any_sl & (dumax * alpha > (u0 - umin)), (u0 - umin) / dumax, alpha)
    return dict(zeroed=sl == 0.0, dc_used=(np.abs(dcs) <= sms) & (sl != 0.0), one_sided=one, alpha_lt1=alpha < 1.0, alpha=alpha,
                slope=sl, u0=u0)


def cellconslin_numpy(book, ratio, flo, fhi):
    """the interpolated fine values on the cells [flo, fhi] from the bookkeeping: crse + sum_d off_d (slope_d alpha)"""
    idx = [np.arange(flo[d], fhi[d] + 1) for d in range(3)]
    cix = [v // ratio + 2 for v in idx]
    g = np.ix_(*cix)
    out = book["u0"][g].copy()
    terms = []
    for d in range(3):
        off = ((idx[d] - (idx[d] // ratio) * ratio).astype(float) + 0.5) / float(ratio) - 0.5
        off = off.reshape([-1 if q == d else 1 for q in range(3)] + [1])
        terms.append(off * (book["slope"][..., d] * book["alpha"])[g])
    return out + terms[0] + terms[1] + terms[2]


# ---------------------------------------------------------------------------------------------------------------------------
# flux register
class FluxRegRef:
    """FluxRegister of amr.hip evaluated directly: one register plane per (fine box, direction, side) on the coarse faces of the
    coarsened box; Reflux adds to the coarse cell outside that face, through the periodic images of the coarse domain and not at all
    outside a wall.  Like the product it also corrects coarse cells that lie under a neighbouring fine box."""

    def __init__(self, cboxes, nc, per, ratio, ncomp):
        self.cboxes, self.nc, self.per, self.r, self.ncomp = cboxes, nc, per, ratio, ncomp
        self.reg = {}
        for b, (lo, hi) in enumerate(cboxes):
            for d in range(3):
                shape = tuple(1 if e == d else hi[e] - lo[e] + 1 for e in range(3)) + (ncomp,)
                for side in (0, 1):
                    self.reg[b, d, side] = np.zeros(shape)

    def set_val(self, v):
        for a in self.reg.values():
            a[...] = v

    def _plane(self, b, d, side, mul=1):
        lo, hi = self.cboxes[b]
        face = lo[d] if side == 0 else hi[d] + 1
        return tuple(slice(mul * face, mul * face + 1) if e == d else slice(mul * lo[e], mul * (hi[e] + 1)) for e in range(3))

    def crse_init(self, flux, d, scomp, dcomp, nc, mult, add=False):
        for b in range(len(self.cboxes)):
            for side in (0, 1):
                v = mult * flux[self._plane(b, d, side)][..., scomp:scomp + nc]
                if add:
                    self.reg[b, d, side][..., dcomp:dcomp + nc] += v
                else:
                    self.reg[b, d, side][..., dcomp:dcomp + nc] = v

    def fine_add(self, flux, d, scomp, dcomp, nc, mult):
        r = self.r
        d1 = 1 if d == 0 else 0
        d2 = 1 if d == 2 else 2
        for b in range(len(self.cboxes)):
            for side in (0, 1):
                pl = flux[self._plane(b, d, side, r)][..., scomp:scomp + nc]
                s = 0.0
                for bb in range(r):            # the kernel's order: a (direction d1) fastest
                    for aa in range(r):
                        sl = [slice(None)] * 3
                        sl[d1] = slice(aa, None, r); sl[d2] = slice(bb, None, r)
                        s = s + pl[tuple(sl)]
                self.reg[b, d, side][..., dcomp:dcomp + nc] += mult * s

    def reflux(self, S, volume, scale, scomp, dcomp, nc):
        for d in range(3):
            for side in (0, 1):
                m = (-scale if side == 0 else scale) / volume
                for b, (lo, hi) in enumerate(self.cboxes):
                    c = lo[d] - 1 if side == 0 else hi[d] + 1
                    if c < 0 or c >= self.nc[d]:
                        if not self.per[d]:
                            continue
                        c %= self.nc[d]
                    sl = tuple(slice(c, c + 1) if e == d else slice(lo[e], hi[e] + 1) for e in range(3))
                    S[sl + (slice(dcomp, dcomp + nc),)] += m * self.reg[b, d, side][..., scomp:scomp + nc]


# ---------------------------------------------------------------------------------------------------------------------------
# average down
def average_down_ref(F, Cin, typ, cboxes, ratio, scomp, ncomp):
    """coarse array after average_down of the fine array F (global, index type typ) on the coarsened fine boxes cboxes: the sum of the
    children in the kernel's order (ir fastest, then jr, kr) times w = 1 / (number of children)"""
    r = ratio
    n = [1 if typ[d] else r for d in range(3)]
    w = 1.0 / float(n[0] * n[1] * n[2])
    out = Cin.copy()
    for lo, hi in cboxes:
        hi = tuple(hi[d] + typ[d] for d in range(3))
        s = 0.0
        for kr in range(n[2]):
            for jr in range(n[1]):
                for ir in range(n[0]):
                    o = (ir, jr, kr)
                    sl = tuple(slice(r * lo[d] + o[d], r * hi[d] + o[d] + 1, r) for d in range(3))
                    s = s + F[sl][..., scomp:scomp + ncomp]
        out[box_slices(lo, hi, (0, 0, 0)) + (slice(scomp, scomp + ncomp),)] = s * w
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# create_umac_grown
def umac_grown_ref(UC, UF, fboxes, nc, ratio, per, divu=None, fdx=None):
    """per fine box: (u, v, w) over the box grown by one cell (face arrays, origin box lo - 1), the same before the divergence fix
    (`lin`), and the level mask over the box grown by two cells (origin lo - 2).  UC[d] / UF[d]: global coarse / fine face arrays
    ((n + e_d)); divu: fine cell array over the domain grown by one cell (origin -1) or None; fdx: fine mesh widths."""
    r = ratio
    nf = tuple(r * v for v in nc)
    rinv = 1.0 / float(r)
    if fdx is None:
        fdx = tuple(1.0 / nf[d] for d in range(3))
    dxi = tuple(1.0 / v for v in fdx)
    images = [(tuple(lo[e] + s[e] for e in range(3)), tuple(hi[e] + s[e] for e in range(3)), s) for lo, hi in fboxes for s in shifts(per, nf)]
    out = []
    for blo, bhi in fboxes:
        U, glo = [], tuple(v - 1 for v in blo)
        for d in range(3):
            ghi = tuple(bhi[e] + 1 + (e == d) for e in range(3))
            fi = [np.arange(glo[e], ghi[e] + 1) for e in range(3)]
            c = [v // r for v in fi]

            def crse(cidx):
                """the periodically extended coarse faces; 0 outside a non-periodic domain (the product's coarse patch starts from 0)"""
                ok = np.ones([len(v) for v in cidx], bool)
                ii = []
                for e in range(3):
                    n_e = nc[e] + (e == d)
                    v = cidx[e]
                    if per[e]:
                        v = np.where(v == nc[e], v, v % nc[e]) if e == d else v % nc[e]
                    good = (v >= 0) & (v < n_e)
                    ok &= good.reshape([-1 if q == e else 1 for q in range(3)])
                    ii.append(np.clip(v, 0, n_e - 1))
                return np.where(ok, UC[d][np.ix_(*ii)], 0.0)
            rem = (fi[d] - c[d] * r).reshape([-1 if q == d else 1 for q in range(3)])
            wgt = rem.astype(float) * rinv
            cp = list(c); cp[d] = c[d] + 1
            a = np.where(rem == 0, crse(c), (1.0 - wgt) * crse(c) + wgt * crse(cp))
            # fine data: the box's own valid faces, and what sibling boxes and periodic images cover (FillBoundary)
            for ilo, ihi, s in images:
                q = intersect(ilo, tuple(ihi[e] + (e == d) for e in range(3)), glo, ghi)
                if q is None:
                    continue
                src = box_slices(tuple(q[0][e] - s[e] for e in range(3)), tuple(q[1][e] - s[e] for e in range(3)), (0, 0, 0))
                a[box_slices(q[0], q[1], glo)] = UF[d][src]
            U.append(a)
        # level mask on the box grown by two cells
        mlo, mhi = tuple(v - 2 for v in blo), tuple(v + 2 for v in bhi)
        mask = np.full(tuple(mhi[e] - mlo[e] + 1 for e in range(3)), 2)
        for e in range(3):
            if not per[e]:
                ix = np.arange(mlo[e], mhi[e] + 1)
                sl = [slice(None)] * 3
                sl[e] = (ix < 0) | (ix > nf[e] - 1)
                mask[tuple(sl)] = 3
        for ilo, ihi, s in images:
            q = intersect(ilo, ihi, mlo, mhi)
            if q is not None:
                mask[box_slices(q[0], q[1], mlo)] = 1
        mask[box_slices(blo, bhi, mlo)] = 0
        lin = [a.copy() for a in U]
        u0, v0, w0 = lin
        u, v, w = U
        M = lambda i, j, k: mask[i - mlo[0], j - mlo[1], k - mlo[2]]
        inl = lambda m: int(m == 0 or m == 1)              # (int: numpy's bool + bool is a logical or)
        count1 = []
        for k in range(glo[2], bhi[2] + 2):
            for j in range(glo[1], bhi[1] + 2):
                for i in range(glo[0], bhi[0] + 2):
                    if blo[0] <= i <= bhi[0] and blo[1] <= j <= bhi[1] and blo[2] <= k <= bhi[2]:
                        continue
                    if M(i, j, k) != 2:
                        continue
                    cnt = (inl(M(i - 1, j, k)) + inl(M(i + 1, j, k)) + inl(M(i, j - 1, k)) + inl(M(i, j + 1, k)) + inl(M(i, j, k - 1)) + inl(M(i, j, k + 1)))
                    if cnt != 1:
                        continue
                    count1.append((i, j, k))
                    a, b, c_ = i - glo[0], j - glo[1], k - glo[2]
                    div = float(divu[i + 1, j + 1, k + 1]) if divu is not None else 0.0
                    dux = dxi[0] * (u0[a + 1, b, c_] - u0[a, b, c_])
                    duy = dxi[1] * (v0[a, b + 1, c_] - v0[a, b, c_])
                    duz = dxi[2] * (w0[a, b, c_ + 1] - w0[a, b, c_])
                    if i < blo[0] and M(i + 1, j, k) != 2:
                        u[a, b, c_] = u0[a + 1, b, c_] + fdx[0] * (duy + duz - div)
                    elif i > bhi[0] and M(i - 1, j, k) != 2:
                        u[a + 1, b, c_] = u0[a, b, c_] - fdx[0] * (duy + duz - div)
                    if j < blo[1] and M(i, j + 1, k) != 2:
                        v[a, b, c_] = v0[a, b + 1, c_] + fdx[1] * (dux + duz - div)
                    elif j > bhi[1] and M(i, j - 1, k) != 2:
                        v[a, b + 1, c_] = v0[a, b, c_] - fdx[1] * (dux + duz - div)
                    if k < blo[2] and M(i, j, k + 1) != 2:
                        w[a, b, c_] = w0[a, b, c_ + 1] + fdx[2] * (dux + duy - div)
                    elif k > bhi[2] and M(i, j, k - 1) != 2:
                        w[a, b, c_ + 1] = w0[a, b, c_] - fdx[2] * (dux + duy - div)
        out.append(dict(u=U, lin=lin, lo=glo, mask=mask, mask_lo=mlo, count1=count1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# input data of the fill-patch cases, chosen so that the limiter's branches are all taken (test_cpu_interlevel_ref.py asserts it)
def _centres(nc):
    return np.meshgrid(*[(np.arange(nc[d]) + 0.5) / nc[d] for d in range(3)], indexing="ij")


def sine_product(nc, seed, phases=None):
    X, Y, Z = _centres(nc)
    a, b, c = np.random.default_rng(seed).random(3) if phases is None else phases
    return np.sin(2 * np.pi * (X + a)) * np.sin(2 * np.pi * (Y + b)) * np.sin(2 * np.pi * (Z + c))


def data_G(nc, seed):
    """general: a ramp in all three directions + a smooth part + a little noise (few extrema, mostly the central slope)"""
    X, Y, Z = _centres(nc)
    return 2.0 * X - 3.0 * Y + 0.5 * Z + 0.5 * sine_product(nc, seed) + 0.05 * np.random.default_rng(seed + 1000).standard_normal(nc)


def data_W(nc, d, side, seed):
    """wall-normal: a ramp along direction d only, so that the one-sided slope at the (d, side) wall is what the limiter passes.
    With ext_dir the wall value W_EXT_* does it.  With hoextrap the ghost cell holds the quadratic extrapolation to the wall and for
    a parabola s x + c x^2 / 2 the one-sided slope s h + c h^2 / 2 is within the limiter's bound 2 (u0 - u_wall) = s h + c h^2 / 4
    only if c and s have opposite signs: the phases put the sine product's lobe of that curvature on the wall, under the patch (the
    noise, 0.012 in that difference against 0.008 of the curvature, still decides many cells)."""
    ph = [-0.25, -0.25, -0.25]
    ph[d] = 0.75 if side == 0 else 0.25
    return -3.0 * _centres(nc)[d] + 0.05 * sine_product(nc, 0, ph) + 0.02 * np.random.default_rng(seed + 1000).standard_normal(nc)


W_EXT_LO, W_EXT_HI = 0.2, -3.2          # ext_dir wall values of data_W: 0.2 beyond the ramp's value at the wall (0 and -3)


def data_K(nc, T):
    """kinked ramp f(i + j + k): f(t) = 3 t on T - 2 <= t <= T - 1, the plateau 3 (T - 1) + 1 above and the plateau 3 (T - 2) - 1
    below.  In the cells of the plane t = T - 1 the limited slopes (2 in each direction, excursion 1.5 at ratio 2) overshoot the
    largest of the 27 neighbours, u0 + 1, and the excursion limiter fires: alpha = 2/3 at ratio 2 and 4/9 at ratio 4; in the plane
    t = T - 2 the same happens against the smallest neighbour.  (With the upper plateau alone only the 27 cells of one plane that lie
    away from the faces of a periodic 8^3 level fire: across the seam one slope is zero, and two slopes do not overshoot.  Hence the
    lower plateau, which adds the second plane.)"""
    I, J, K = np.meshgrid(*[np.arange(nc[d]) for d in range(3)], indexing="ij")
    t = I + J + K
    return np.where(t < T - 2, 3.0 * (T - 2) - 1.0, np.where(t <= T - 1, 3.0 * t, 3.0 * (T - 1) + 1.0)).astype(float)


def refine_box(b, r):
    return (tuple(r * v for v in b[0]), tuple(r * v + r - 1 for v in b[1]))


WALL_BCS = (BC_REFLECT_ODD, BC_REFLECT_EVEN, BC_FOEXTRAP, BC_EXT_DIR, BC_HOEXTRAP)
WALL_CASES = [(d, side, 2) for d in range(3) for side in (0, 1)] + [(1, 0, 4), (2, 1, 4)]


# seeds of the noise of the W components and of the G component, per wall case (see data_W: with hoextrap the noise decides, and a
# seed is kept only if the input conditions of test_cpu_interlevel_ref.py hold)
WALL_SEEDS = {(0, 0, 2): (10, 101), (0, 1, 2): (10, 101), (1, 0, 2): (5, 2), (1, 1, 2): (30, 2), (2, 0, 2): (25, 10), (2, 1, 2): (25, 10),
              (1, 0, 4): (5, 2), (2, 1, 4): (25, 10)}


def _bc(types_lo, types_hi):
    return (tuple(types_lo), tuple(types_hi))


def wall_case(d, side, ratio):
    """a fine patch, ratio * 4 cells thick, on the (d, side) face of a domain that is walled in d, periodic in d + 1 and walled (and
    not touched) in d + 2; components 0-4: W data with reflect_odd, reflect_even, foextrap, ext_dir, hoextrap on the touched face,
    5: G, 6: K (foextrap)"""
    nc = (8, 8, 8)
    per = [0, 0, 0]; per[(d + 1) % 3] = 1
    clo, chi = [2, 2, 2], [5, 5, 5]
    clo[d], chi[d] = (0, 3) if side == 0 else (4, 7)
    half = list(chi); half[(d + 1) % 3] = 3
    half2 = list(clo); half2[(d + 1) % 3] = 4
    cboxes = [(tuple(clo), tuple(half)), (tuple(half2), tuple(chi))]
    bcs, edlo, edhi = [], [], []
    for n in range(7):
        lo, hi = [BC_FOEXTRAP] * 3, [BC_FOEXTRAP] * 3
        for e in range(3):
            if per[e]:
                lo[e] = hi[e] = BC_INT_DIR
        if n < 5:
            (lo if side == 0 else hi)[d] = WALL_BCS[n]
        bcs.append(_bc(lo, hi))
        el, eh = [0.0] * 3, [0.0] * 3
        el[d], eh[d] = W_EXT_LO, W_EXT_HI
        edlo.append(el); edhi.append(eh)
    ws, gs = WALL_SEEDS[d, side, ratio]
    crse = np.stack([data_W(nc, d, side, ws + n) for n in range(5)] + [data_G(nc, gs), data_K(nc, 12)], axis=-1)
    return dict(nc=nc, ratio=ratio, per=tuple(per), cboxes=cboxes, ng=3, bcs=bcs, edlo=edlo, edhi=edhi, crse=crse, kinds="WWWWWGK", wall=(d, side))


CORNER_SEEDS = (12, 0, 1)


def corner_case():
    """a patch in the (lo, lo, hi) corner of a domain with six walls, a different BC type on each of the three touched faces and a
    different assignment per component: the ghost cells outside two and three faces take the composition of the rules"""
    nc = (8, 8, 8)
    trip = [(BC_EXT_DIR, BC_HOEXTRAP, BC_REFLECT_EVEN), (BC_HOEXTRAP, BC_FOEXTRAP, BC_EXT_DIR), (BC_REFLECT_ODD, BC_EXT_DIR, BC_HOEXTRAP),
            (BC_FOEXTRAP, BC_REFLECT_EVEN, BC_REFLECT_ODD)]
    bcs = [_bc((t[0], t[1], BC_FOEXTRAP), (BC_FOEXTRAP, BC_FOEXTRAP, t[2])) for t in trip]
    edlo = [[0.3, -0.4, 0.0]] * 4
    edhi = [[0.0, 0.0, 0.7]] * 4
    crse = np.stack([data_G(nc, CORNER_SEEDS[0]), data_G(nc, CORNER_SEEDS[1]), data_G(nc, CORNER_SEEDS[2]), data_K(nc, 12)], axis=-1)
    return dict(nc=nc, ratio=2, per=(0, 0, 0), cboxes=[((0, 0, 4), (3, 3, 7))], ng=3, bcs=bcs, edlo=edlo, edhi=edhi, crse=crse, kinds="GGGK")


LAYOUTS = {
    # name: (coarse domain, coarse boxes of the fine patch, T of the K data)
    "span_x": ((8, 8, 8), [((0, 2, 2), (7, 5, 5))], 12),                      # its own image covers the x ghost cells
    "neg_yz": ((12, 8, 8), [((3, 0, 4), (8, 3, 7))], 12),                     # periodic y-lo and z-hi: coarse indices -1, -2 and 8, 9
    "ell": ((12, 8, 8), [((1, 1, 2), (6, 2, 5)), ((1, 3, 2), (2, 5, 5)), ((1, 6, 2), (2, 6, 5))], 12),   # re-entrant corner at (3, 3)
    "one": ((8, 8, 8), [((2, 2, 2), (5, 5, 5))], 12),
    "two": ((8, 8, 8), [((2, 2, 2), (3, 5, 5)), ((4, 2, 2), (5, 5, 5))], 12),
    "eight": ((8, 8, 8), [((2 + 2 * a, 2 + 2 * b, 2 + 2 * c), (3 + 2 * a, 3 + 2 * b, 3 + 2 * c)) for c in (0, 1) for b in (0, 1) for a in (0, 1)], 12),
}
LAYOUT_CASES = [("span_x", 3, 2), ("neg_yz", 3, 2), ("neg_yz", 1, 2), ("ell", 3, 2), ("ell", 1, 2), ("one", 3, 2), ("two", 3, 2), ("eight", 3, 2),
                ("eight", 1, 2), ("neg_yz", 3, 4)]


def layout_case(name, ng, ratio):
    """fully periodic; components G and K"""
    nc, cboxes, T = LAYOUTS[name]
    crse = np.stack([data_G(nc, 2), data_K(nc, T)], axis=-1)
    return dict(nc=nc, ratio=ratio, per=(1, 1, 1), cboxes=cboxes, ng=ng, bcs=None, edlo=None, edhi=None, crse=crse, kinds="GK")


def case_fine_boxes(case):
    return [refine_box(b, case["ratio"]) for b in case["cboxes"]]


def case_fine_data(case, seed=3):
    nf = tuple(case["ratio"] * v for v in case["nc"])
    return np.random.default_rng(seed).standard_normal(nf + (case["crse"].shape[3],))


def case_ref(orc, case):
    fb = case_fine_boxes(case)
    return fillpatch_ref(orc, fb, case["ng"], 0.0, (None, case_fine_data(case), 0.0, 0.0), fb, (None, case["crse"], 0.0, 0.0), case["nc"],
                         case["ratio"], case["per"], case["bcs"], case["edlo"], case["edhi"])
