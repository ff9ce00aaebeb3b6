"""ctypes binding of libiamrx.so (C-ABI declared in include/iamrx.h).

The HIP library is the product; there is no CPU fallback: importing works without a GPU (so that the
build / symbol checks can run), but `init()` raises if no gfx950 device is present.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libiamrx.so")
_lib = None


class IamrxError(RuntimeError):
    pass


class Geom(C.Structure):
    _fields_ = [("dom_lo", C.c_int * 3), ("dom_hi", C.c_int * 3), ("prob_lo", C.c_double * 3),
                ("prob_hi", C.c_double * 3), ("periodic", C.c_int * 3)]

    @staticmethod
    def make(n, prob_lo=(0.0, 0.0, 0.0), prob_hi=(1.0, 1.0, 1.0), periodic=(1, 1, 1)):
        g = Geom()
        g.dom_lo = (C.c_int * 3)(0, 0, 0)
        g.dom_hi = (C.c_int * 3)(*[int(n[d]) - 1 for d in range(3)])
        g.prob_lo = (C.c_double * 3)(*prob_lo)
        g.prob_hi = (C.c_double * 3)(*prob_hi)
        g.periodic = (C.c_int * 3)(*periodic)
        return g

    @property
    def n(self):
        return tuple(self.dom_hi[d] - self.dom_lo[d] + 1 for d in range(3))

    @property
    def dx(self):
        return tuple((self.prob_hi[d] - self.prob_lo[d]) / self.n[d] for d in range(3))


class MgOpts(C.Structure):
    _fields_ = [("nu1", C.c_int), ("nu2", C.c_int), ("nuf", C.c_int), ("nub", C.c_int), ("max_iters", C.c_int),
                ("bottom_maxiter", C.c_int), ("bottom_reltol", C.c_double), ("omega", C.c_double),
                ("maxorder", C.c_int), ("max_coarsening_level", C.c_int), ("min_width", C.c_int),
                ("nodal_sweeps", C.c_int), ("nodal_smoother", C.c_int), ("verbose", C.c_int),
                ("bottom_smoother_only", C.c_int), ("fixed_iters", C.c_int), ("nodal_nu1", C.c_int), ("nodal_nu2", C.c_int),
                ("device_bottom", C.c_int), ("slab", C.c_int)]


class MgStats(C.Structure):
    _fields_ = [("iters", C.c_int), ("resnorm0", C.c_double), ("rhsnorm0", C.c_double), ("resnorm", C.c_double),
                ("bottom_iters_total", C.c_int), ("converged", C.c_int), ("vcycle_ms", C.c_double), ("nlevels", C.c_int)]


def lib():
    """load libiamrx.so (fails loudly if it has not been built)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IamrxError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for the product path)")
        _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _lib.iamrx_last_error.restype = C.c_char_p
        _lib.iamrx_stream.restype = C.c_void_p
    return _lib


def check(rc):
    if rc != 0:
        raise IamrxError(lib().iamrx_last_error().decode())


_initialized = False


def init(device=0):
    global _initialized
    check(lib().iamrx_init(int(device)))
    _initialized = True


def tuning_set(key, value):
    """run-time switch of the library (include/iamrx.h: iamrx_tuning_set); key without the IAMRX_ prefix"""
    check(lib().iamrx_tuning_set(key.encode(), C.c_double(float(value))))


def tuning_get(key, default):
    v = C.c_double()
    check(lib().iamrx_tuning_get(key.encode(), C.c_double(float(default)), C.byref(v)))
    return v.value


def sync():
    check(lib().iamrx_sync())


def comm_rank():
    """(rank, number of ranks) of the installed communicator; (0, 1) without one"""
    r, n = C.c_int(), C.c_int()
    check(lib().iamrx_comm_rank(C.byref(r), C.byref(n)))
    return r.value, n.value


def comm_allreduce(a, op=0):
    """in-place all-reduce of a float64 numpy array over the ranks (include/iamrx.h: iamrx_comm_allreduce); op 0 sum, 1 max, 2 min.
    Collective; one rank: `a` stays as it is."""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
        raise TypeError("comm_allreduce: a C-contiguous float64 numpy array is reduced in place")
    L = lib()
    if L.iamrx_comm_allreduce(a.ctypes.data_as(C.POINTER(C.c_double)), int(a.size), int(op)) != 0:
        L.iamrx_comm_last_error.restype = C.c_char_p
        raise IamrxError(L.iamrx_comm_last_error().decode())
    return a


def comm_barrier():
    """every rank has arrived (a one-element sum through comm_allreduce)"""
    comm_allreduce(np.zeros(1), 0)


def mg_opts(**kw):
    o = MgOpts()
    lib().iamrx_mg_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def i3(v):
    return (C.c_int * 3)(*[int(x) for x in v])


CELL = (0, 0, 0)
NODE = (1, 1, 1)


def face(d):
    t = [0, 0, 0]
    t[d] = 1
    return tuple(t)


class Layout:
    """BoxArray + DistributionMapping of one level."""

    def __init__(self, boxes, owners=None):
        nb = len(boxes)
        arr = (C.c_int * (6 * nb))()
        for i, (lo, hi) in enumerate(boxes):
            for d in range(3):
                arr[6 * i + d] = int(lo[d])
                arr[6 * i + 3 + d] = int(hi[d])
        own = (C.c_int * nb)(*([0] * nb if owners is None else [int(o) for o in owners]))
        self.h = C.c_void_p()
        check(lib().iamrx_layout_create(nb, arr, own, C.byref(self.h)))
        self.boxes = [(tuple(lo), tuple(hi)) for lo, hi in boxes]
        self.owners = [0] * nb if owners is None else list(owners)

    @staticmethod
    def from_handle(h, boxes, owners=None):
        """wrap a layout handle obtained from the library (e.g. iamrx_amr_level_layout)"""
        self = Layout.__new__(Layout)
        self.h = h
        self.boxes = [(tuple(lo), tuple(hi)) for lo, hi in boxes]
        self.owners = [0] * len(boxes) if owners is None else list(owners)
        return self

    @staticmethod
    def single(n):
        return Layout([((0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1))])

    @staticmethod
    def decompose(n, max_grid_size, nranks=1):
        """chop the domain [0,n-1]^3 into boxes of at most max_grid_size, round-robin over ranks"""
        boxes = []
        mg = max_grid_size if hasattr(max_grid_size, "__len__") else (max_grid_size,) * 3
        for k0 in range(0, n[2], mg[2]):
            for j0 in range(0, n[1], mg[1]):
                for i0 in range(0, n[0], mg[0]):
                    boxes.append(((i0, j0, k0), (min(i0 + mg[0], n[0]) - 1, min(j0 + mg[1], n[1]) - 1, min(k0 + mg[2], n[2]) - 1)))
        per = (len(boxes) + nranks - 1) // nranks
        owners = [min(i // per, nranks - 1) for i in range(len(boxes))]
        return Layout(boxes, owners)

    def nlocal(self):
        n = C.c_int()
        check(lib().iamrx_layout_nlocal(self.h, C.byref(n)))
        return n.value

    def local_box(self, li):
        a = (C.c_int * 6)()
        gi = C.c_int()
        check(lib().iamrx_layout_local_box(self.h, li, a, C.byref(gi)))
        return tuple(a[0:3]), tuple(a[3:6]), gi.value

    def __del__(self):
        try:
            if self.h:
                lib().iamrx_layout_destroy(self.h)
        except Exception:
            pass


def local_indices(lay):
    """global indices (in lay.boxes) of the boxes this rank owns, in the order of its local fabs (increasing)"""
    return [lay.local_box(li)[2] for li in range(lay.nlocal())]


class MultiFab:
    """device-resident multi-component array over the boxes of a Layout"""

    def __init__(self, layout, typ=CELL, ncomp=1, ngrow=0, _handle=None, _owned=True):
        self.layout = layout
        self.typ = tuple(typ)
        self.ncomp = ncomp
        self.ngrow = ngrow
        self._owned = _owned
        if _handle is not None:
            self.h = _handle
        else:
            self.h = C.c_void_p()
            check(lib().iamrx_mf_create(layout.h, i3(typ), ncomp, ngrow, C.byref(self.h)))

    def nlocal(self):
        n = C.c_int()
        check(lib().iamrx_mf_info(self.h, None, None, None, C.byref(n)))
        return n.value

    def fab_box(self, li=0):
        a = (C.c_int * 6)()
        check(lib().iamrx_mf_fab_box(self.h, li, a))
        return tuple(a[0:3]), tuple(a[3:6])

    def to_numpy(self, li=0):
        """(nx,ny,nz,nc) Fortran-ordered copy of local fab li, ghost cells included; returns (array, lo)"""
        lo, hi = self.fab_box(li)
        shape = tuple(hi[d] - lo[d] + 1 for d in range(3)) + (self.ncomp,)
        a = np.empty(shape, dtype=np.float64, order="F")
        check(lib().iamrx_mf_to_host(self.h, li, a.ctypes.data_as(C.POINTER(C.c_double))))
        return a, lo

    def from_numpy(self, a, li=0):
        lo, hi = self.fab_box(li)
        shape = tuple(hi[d] - lo[d] + 1 for d in range(3)) + (self.ncomp,)
        a = np.asfortranarray(a, dtype=np.float64).reshape(shape, order="F")
        check(lib().iamrx_mf_from_host(self.h, li, a.ctypes.data_as(C.POINTER(C.c_double))))

    def set_from_global(self, G, glo):
        """fill every local fab (valid + ghosts) from a global numpy array G whose index origin is glo"""
        for li in range(self.nlocal()):
            lo, hi = self.fab_box(li)
            sl = tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))
            self.from_numpy(G[sl], li)

    def gather_valid(self, n):
        """assemble the valid regions of all LOCAL fabs into a global array over cells [0,n-1] (+type)"""
        shape = tuple(n[d] + self.typ[d] for d in range(3)) + (self.ncomp,)
        G = np.zeros(shape, order="F")
        for li in range(self.nlocal()):
            a, lo = self.to_numpy(li)
            blo, bhi, _ = self.layout.local_box(li)
            vlo = blo
            vhi = tuple(bhi[d] + self.typ[d] for d in range(3))
            src = tuple(slice(vlo[d] - lo[d], vhi[d] - lo[d] + 1) for d in range(3))
            dst = tuple(slice(vlo[d], vhi[d] + 1) for d in range(3))
            G[dst] = a[src]
        return G

    def setval(self, v):
        check(lib().iamrx_mf_setval(self.h, C.c_double(v)))

    def fill_boundary(self, geom):
        check(lib().iamrx_mf_fill_boundary(self.h, C.byref(geom)))

    def fill_physbc(self, geom, bc, extdir_lo=None, extdir_hi=None, scomp=0, ncomp=None):
        """physical BC fill outside the domain; bc: list of (lo[3], hi[3]) BCType codes per component"""
        nc = self.ncomp if ncomp is None else ncomp
        el = None if extdir_lo is None else (C.c_double * (3 * nc))(*[float(x) for row in extdir_lo for x in row])
        eh = None if extdir_hi is None else (C.c_double * (3 * nc))(*[float(x) for row in extdir_hi for x in row])
        check(lib().iamrx_mf_fill_physbc(self.h, C.byref(geom), scomp, nc, _bcrec(nc, bc), el, eh))

    def norm0(self, comp=0, ncomp=None, ngrow=0):
        out = C.c_double()
        check(lib().iamrx_mf_norm0(self.h, comp, self.ncomp if ncomp is None else ncomp, ngrow, C.byref(out)))
        return out.value

    def norm0_comps(self, comp=0, ncomp=None, ngrow=0, form=0):
        """per-component max norms; form 0 MultiFab::norm0_comps, 1 / 2 the functor reduction with the host / device finish (ncomp 1, 3, 6)"""
        nc = self.ncomp - comp if ncomp is None else ncomp
        out = (C.c_double * nc)()
        check(lib().iamrx_mf_norm0_comps(self.h, comp, nc, ngrow, form, out))
        return list(out)

    def minmax(self, comp=0, ngrow=0):
        """(smallest, largest) value of one component over the valid region grown by ngrow"""
        mn, mx = C.c_double(), C.c_double()
        check(lib().iamrx_mf_minmax(self.h, comp, ngrow, C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    def dev_ptr(self, li=0):
        p = C.POINTER(C.c_double)()
        check(lib().iamrx_mf_dev_ptr(self.h, li, C.byref(p)))
        return C.cast(p, C.c_void_p).value

    def __del__(self):
        try:
            if self._owned and self.h:
                lib().iamrx_mf_destroy(self.h)
        except Exception:
            pass


def _h(m):
    return m.h if m is not None else None


def dot(geom, x0, y0, x1=None, y1=None, comp=0, ncomp=1, on_device=0, lobc=(0, 0, 0), hibc=(0, 0, 0)):
    """owner-weighted dot products x0.y0 (and x1.y1); lobc / hibc: the nodal solver's LinOpBC codes (Neumann walls weigh 1/2)"""
    out = (C.c_double * 2)()
    check(lib().iamrx_mf_dot(C.byref(geom), i3(lobc), i3(hibc), x0.h, y0.h, _h(x1), _h(y1), comp, ncomp, int(on_device), out))
    return list(out) if x1 is not None else out[0]


def sum_unique(geom, m, comp=0, lobc=(0, 0, 0), hibc=(0, 0, 0)):
    """owner-weighted sum of one component (MultiFab::sum_unique), the weights of dot()"""
    out = C.c_double()
    check(lib().iamrx_mf_sum_unique(C.byref(geom), i3(lobc), i3(hibc), m.h, comp, C.byref(out)))
    return out.value


def abec_gsrb(geom, alpha, beta, a, b, phi, rhs, redblack, omega=1.15, lobc=(0, 0, 0), hibc=(0, 0, 0), maxorder=3):
    check(lib().iamrx_abec_gsrb(C.byref(geom), C.c_double(alpha), C.c_double(beta), _h(a), b[0].h, b[1].h, b[2].h,
                                phi.h, rhs.h, redblack, C.c_double(omega), i3(lobc), i3(hibc), maxorder))


def parallel_copy(dst, src, scomp=0, dcomp=0, ncomp=None, src_ng=0, dst_ng=0, periodic_geom=None):
    nc = src.ncomp if ncomp is None else ncomp
    check(lib().iamrx_parallel_copy(dst.h, src.h, scomp, dcomp, nc, src_ng, dst_ng, C.byref(periodic_geom) if periodic_geom is not None else None))


def fillpatch_two_levels(dst, time, fine, crse, cgeom, fgeom, scomp=0, ncomp=None, dcomp=0, ratio=2, bc=None, extdir_lo=None, extdir_hi=None):
    """fine / crse: (old MultiFab or None, new MultiFab, t_old, t_new)"""
    nc = dst.ncomp if ncomp is None else ncomp
    el = None if extdir_lo is None else (C.c_double * (3 * nc))(*[float(x) for row in extdir_lo for x in row])
    eh = None if extdir_hi is None else (C.c_double * (3 * nc))(*[float(x) for row in extdir_hi for x in row])
    bcs = bc if bc is not None else [((0, 0, 0), (0, 0, 0))] * nc
    check(lib().iamrx_fillpatch_two_levels(dst.h, dcomp, C.c_double(time), _h(fine[0]), fine[1].h, C.c_double(fine[2]), C.c_double(fine[3]),
                                           _h(crse[0]), crse[1].h, C.c_double(crse[2]), C.c_double(crse[3]), scomp, nc,
                                           C.byref(cgeom), C.byref(fgeom), ratio, _bcrec(nc, bcs), el, eh))


def create_umac_grown(umac_fine, umac_crse, cgeom, fgeom, ratio=2, divu=None):
    check(lib().iamrx_create_umac_grown(umac_fine[0].h, umac_fine[1].h, umac_fine[2].h, umac_crse[0].h, umac_crse[1].h, umac_crse[2].h,
                                        _h(divu), C.byref(cgeom), C.byref(fgeom), ratio))


class FluxRegister:
    """amrex::FluxRegister role (names as in the reference: CrseInit, FineAdd, Reflux)"""

    def __init__(self, fine_layout, crse_layout, cgeom, ratio, ncomp):
        self.h = C.c_void_p()
        self._keep = (fine_layout, crse_layout)
        check(lib().iamrx_fluxreg_create(fine_layout.h, crse_layout.h, C.byref(cgeom), ratio, ncomp, C.byref(self.h)))

    def setVal(self, v):
        check(lib().iamrx_fluxreg_setval(self.h, C.c_double(v)))

    def CrseInit(self, flux, dir, scomp, dcomp, ncomp, mult, add=False):
        check(lib().iamrx_fluxreg_crse_init(self.h, flux.h, dir, scomp, dcomp, ncomp, C.c_double(mult), int(add)))

    def FineAdd(self, flux, dir, scomp, dcomp, ncomp, mult):
        check(lib().iamrx_fluxreg_fine_add(self.h, flux.h, dir, scomp, dcomp, ncomp, C.c_double(mult)))

    def Reflux(self, S, volume, scale, scomp, dcomp, ncomp):
        check(lib().iamrx_fluxreg_reflux(self.h, S.h, C.c_double(volume), C.c_double(scale), scomp, dcomp, ncomp))

    def __del__(self):
        try:
            if self.h:
                lib().iamrx_fluxreg_destroy(self.h)
                self.h = None
        except Exception:
            pass


class SyncRegister:
    """IAMR's SyncRegister (Source/SyncRegister.H:10-66; names as in the reference: CrseInit, FineAdd, InitRHS) of one coarse/fine interface"""

    def __init__(self, fine_layout, crse_layout, cgeom, fgeom, ratio=2, phys_lo=(0, 0, 0), phys_hi=(0, 0, 0)):
        self.h = C.c_void_p()
        self._keep = (fine_layout, crse_layout)
        check(lib().iamrx_syncreg_create(fine_layout.h, crse_layout.h, C.byref(cgeom), C.byref(fgeom), int(ratio), i3(phys_lo), i3(phys_hi), C.byref(self.h)))

    def CrseInit(self, sync_resid_crse, mult):
        check(lib().iamrx_syncreg_crse_init(self.h, sync_resid_crse.h, C.c_double(mult)))

    def FineAdd(self, sync_resid_fine, mult):
        check(lib().iamrx_syncreg_fine_add(self.h, sync_resid_fine.h, C.c_double(mult)))

    def CompAdd(self, sync_resid_fine, fgeom, finer_layout, finer_ratio, mult):
        """Source/SyncRegister.cpp:302-348: zero the residual on the nodes of the next finer level's boxes, then FineAdd (modifies the residual)"""
        check(lib().iamrx_syncreg_comp_add(self.h, sync_resid_fine.h, C.byref(fgeom), finer_layout.h, int(finer_ratio), C.c_double(mult)))

    def InitRHS(self, rhs):
        check(lib().iamrx_syncreg_init_rhs(self.h, rhs.h))

    def __del__(self):
        try:
            if self.h:
                lib().iamrx_syncreg_destroy(self.h)
                self.h = None
        except Exception:
            pass


def average_down(fine, crse, scomp=0, ncomp=None, ratio=2):
    check(lib().iamrx_average_down(fine.h, crse.h, scomp, crse.ncomp if ncomp is None else ncomp, ratio))


SMOOTHER_PATHS = ("COLOUR", "RB_BOX", "RB_CF", "RB_NBR", "FUSED_SHELL")
SMOOTHER_KERNELS = ("general", "gsrb1", "gsrb2", "gsrb2_per_comp")


def host_abec_smoother_plan(geom, boxes, ncomp=1, coef=1, has_a=False, has_cf=False, finest=True, ngrow=(1, 0, 1, 0), lobc=(0, 0, 0), hibc=(0, 0, 0),
                            maxorder=3):
    """host-only: the smoother path of a cell-centred multigrid level (include/iamrx.h: iamrx_host_abec_smoother_plan) as a dict;
    boxes: [(lo, hi), ...], the level's global box list"""
    arr = (C.c_int * (6 * len(boxes)))(*[int(v) for lo, hi in boxes for v in tuple(lo) + tuple(hi)])
    out = (C.c_int * 12)()
    check(lib().iamrx_host_abec_smoother_plan(len(boxes), arr, C.byref(geom), i3(lobc), i3(hibc), int(maxorder), int(ncomp), int(coef), int(has_a),
                                              int(has_cf), int(finest), (C.c_int * 4)(*[int(v) for v in ngrow]), out))
    keys = ("path", "nw", "nbr_splits", "zero_first", "kernel", "mode", "np", "maintain", "allcf", "wrap", "walls_inkernel", "zero_ok")
    d = dict(zip(keys, out[:]))
    d["path"], d["kernel"] = SMOOTHER_PATHS[d["path"]], SMOOTHER_KERNELS[d["kernel"]]
    return d


def host_abec_leg_plan(geom, boxes, level, nu1=2, nu2=2, ncomp=1, coef=0, has_a=False, has_cf=False, ngrow=(1, 0, 0, 0), lobc=(0, 0, 0), hibc=(0, 0, 0),
                       maxorder=3, slab_transition=False, agg_transition=False):
    """host-only: whether a coarse level of the cell-centred V-cycle runs its down leg and its up leg as one launch each
    (include/iamrx.h: iamrx_host_abec_leg_plan) as a dict; boxes: [(lo, hi), ...], the level's global box list"""
    arr = (C.c_int * (6 * len(boxes)))(*[int(v) for lo, hi in boxes for v in tuple(lo) + tuple(hi)])
    out = (C.c_int * 9)()
    check(lib().iamrx_host_abec_leg_plan(len(boxes), arr, C.byref(geom), i3(lobc), i3(hibc), int(maxorder), int(ncomp), int(coef), int(has_a),
                                         int(has_cf), int(level == 0), (C.c_int * 4)(*[int(v) for v in ngrow]), int(level), int(nu1), int(nu2),
                                         int(slab_transition), int(agg_transition), out))
    v = out[:]
    return dict(legs=bool(v[0]), tile_down=tuple(v[1:4]), tile_up=tuple(v[4:7]), halo_down=v[7], halo_up=v[8])


NODAL_SMOOTHER_PATHS = ("JACOBI", "COLOUR8", "SMALL", "GS4", "GSR")
NODAL_BOTTOM_KINDS = ("NONE", "SMOOTHER_ONLY", "DEVICE_PERIODIC", "DEVICE_GENERAL", "HOST_KRYLOV")


def host_nodal_smoother_plan(geom, boxes, has_mask=False, nodal_smoother=0, bottom_smoother_only=False, device_bottom=True, nodal_sweeps=2,
                             coarsest=False, ngrow=(4, 4), lobc=(0, 0, 0), hibc=(0, 0, 0)):
    """host-only: the smoother and bottom path of a nodal multigrid level (include/iamrx.h: iamrx_host_nodal_smoother_plan) as a dict;
    boxes: [(lo, hi), ...], the level's global box list; ngrow: ghost widths of correction and right-hand side"""
    arr = (C.c_int * (6 * len(boxes)))(*[int(v) for lo, hi in boxes for v in tuple(lo) + tuple(hi)])
    out = (C.c_int * 11)()
    check(lib().iamrx_host_nodal_smoother_plan(len(boxes), arr, C.byref(geom), i3(lobc), i3(hibc), int(has_mask), int(nodal_smoother),
                                               int(bottom_smoother_only), int(device_bottom), int(nodal_sweeps), int(coarsest),
                                               (C.c_int * 2)(*[int(v) for v in ngrow]), out))
    keys = ("path", "ngrow", "wrap", "refl", "images", "written_first", "zero_start", "par_fill", "splits", "bottom", "sweeps")
    d = dict(zip(keys, out[:]))
    d["path"], d["bottom"] = NODAL_SMOOTHER_PATHS[d["path"]], NODAL_BOTTOM_KINDS[d["bottom"]]
    return d


def host_godunov_plan(geom, boxes, pred=False, scheme=0, has_force=True, fit=False, has_divu=False, edge_out=False, flux_out=False, iconserv=(0, 0, 0)):
    """host-only: the launches one call of the fused Godunov kernels issues on a level and the tiles of its classes (include/iamrx.h:
    iamrx_host_godunov_plan) as a dict; boxes: [(lo, hi), ...]; iconserv: one entry per component (prediction: the three velocities).
    launches: dicts in issue order; chunks: [(first plane, last plane)] relative to a box; tiles: (class, box, tile x, tile y, chunk) in
    list order, box -1 = padding"""
    arr = (C.c_int * (6 * len(boxes)))(*[int(v) for lo, hi in boxes for v in tuple(lo) + tuple(hi)])
    ncomp = 3 if pred else len(iconserv)
    ic = (C.c_int * max(1, ncomp))(*([0, 0, 0] if pred else [int(v) for v in iconserv]))
    head, la, st, nt = (C.c_int * 5)(), (C.c_int * 64)(), (C.c_int * 20)(), C.c_int()
    args = (int(pred), len(boxes), arr, C.byref(geom), int(scheme), int(has_force), int(fit), int(has_divu), int(edge_out), int(flux_out), ncomp, ic, head, la, st)
    check(lib().iamrx_host_godunov_plan(*args, None, 0, C.byref(nt)))
    ti = (C.c_int * max(1, 5 * nt.value))()
    check(lib().iamrx_host_godunov_plan(*args, ti, nt.value, C.byref(nt)))
    launches = []
    for i in range(head[3]):
        v = la[16 * i:16 * i + 16]
        launches.append(dict(sel=v[0], bcs=bool(v[1]), frc=v[2], dvu=v[3], out=v[4], cns=v[5], comps=tuple(v[8:8 + v[6]])))
    return dict(tile=(head[0], head[1]), kc=head[2], launches=launches, chunks=[(st[c], st[c + 1] - 1) for c in range(head[4])],
                tiles=[tuple(ti[5 * i:5 * i + 5]) for i in range(nt.value)])


# the 17 values of a forcing mode, in the order of upstream's arrays (Tutorials/HIT/NS_getForce.cpp:249-281)
TURB_FIELDS = ("FTX", "TAT", "FPX", "FPY", "FPZ", "FAX", "FAY", "FAZ", "FPXX", "FPXY", "FPXZ", "FPYX", "FPYY", "FPYZ", "FPZX", "FPZY", "FPZZ")


def host_turb_modes(prob_lo, prob_hi, nmodes=4, mode_start=0, div_free=1):
    """host-only: the mode table of the turbulent forcing for a domain (include/iamrx.h: iamrx_host_turb_modes) -> (kxyz (M, 3) int32,
    data (M, 17) float64, columns TURB_FIELDS)"""
    lo, hi = (C.c_double * 3)(*[float(v) for v in prob_lo]), (C.c_double * 3)(*[float(v) for v in prob_hi])
    M = C.c_int()
    check(lib().iamrx_host_turb_modes(lo, hi, int(nmodes), int(mode_start), int(div_free), 0, C.byref(M), None, None))
    k = np.zeros((M.value, 3), dtype=np.int32)
    d = np.zeros((M.value, 17))
    check(lib().iamrx_host_turb_modes(lo, hi, int(nmodes), int(mode_start), int(div_free), M.value, C.byref(M), k.ctypes.data_as(C.POINTER(C.c_int)),
                                      d.ctypes.data_as(C.POINTER(C.c_double))))
    return k, d


def _turb_table(kxyz, data):
    k = np.ascontiguousarray(kxyz, dtype=np.int32).reshape(-1, 3)
    d = np.ascontiguousarray(data, dtype=np.float64).reshape(-1, 17)
    if len(k) != len(d):
        raise ValueError("turbulent forcing table: kxyz (M, 3) and data (M, 17) must have the same number of modes")
    _turb_table.keep = (k, d)              # the pointers below are read during the call only
    return len(k), k.ctypes.data_as(C.POINTER(C.c_int)), d.ctypes.data_as(C.POINTER(C.c_double))


def turb_force(geom, kxyz, data, div_free, time, out, ocomp=0):
    """k_turb_force alone: out(ocomp .. ocomp + 2) = the forcing's acceleration f(x, time) on the cells and every ghost cell of out
    (include/iamrx.h: iamrx_turb_force)"""
    M, k, d = _turb_table(kxyz, data)
    check(lib().iamrx_turb_force(C.byref(geom), M, k, d, int(div_free), C.c_double(float(time)), out.h, int(ocomp)))


def mf_spectrum(geom, mf, comp=0, ncomp=1):
    """shell-summed power spectra of components comp .. comp + ncomp - 1 of a cell-centred MultiFab whose boxes tile the fully periodic
    domain of geom (include/iamrx.h: iamrx_mf_spectrum) -> (P (ncomp, nbins), count (nbins,) int64)"""
    from . import spectrum as _s
    return _s.mf_spectrum(geom, mf, comp, ncomp)


def mf_plane_spectrum(geom, mf, dir, comp=0, ncomp=1):
    """ring-summed plane spectra of components comp .. comp + ncomp - 1 of a cell-centred MultiFab along the normal axis dir; only the
    two directions in the plane must be periodic (include/iamrx.h: iamrx_mf_plane_spectrum) -> (P (ncomp, nplanes, nrings), count
    (nrings,) int64)"""
    from . import planespec as _p
    return _p.mf_plane_spectrum(geom, mf, dir, comp, ncomp)


def mf_plane_cospectrum(geom, a, b, dir, acomp=0, bcomp=0):
    """plane co-spectrum of component acomp of a and bcomp of b along the normal axis dir (include/iamrx.h: iamrx_mf_plane_cospectrum;
    one packed transform) -> (C_ab, P_a, P_b, each (nplanes, nrings), count (nrings,))"""
    from . import planespec as _p
    return _p.mf_plane_cospectrum(geom, a, b, dir, acomp, bcomp)


def host_spectrum_slab_plan(geom, boxes, owners, rank, nranks):
    """host only: eligibility and the scatter plan of the slab-decomposed transform (include/iamrx.h: iamrx_host_spectrum_slab_plan)
    -> (eligible, reason, rows (n, 10) int64: spectrum.SLAB_ROW)"""
    from . import spectrum as _s
    return _s.host_slab_plan(geom, boxes, owners, rank, nranks)


def spectrum_slab_info():
    """the path, the sizes and the traffic of the last shell-sum call on this rank (include/iamrx.h: iamrx_spectrum_slab_info) -> dict
    with the keys spectrum.SLAB_INFO"""
    from . import spectrum as _s
    return _s.slab_info()


def spectrum_slab_bench(geom, nranks, reps=1):
    """milliseconds (reps, 10) of the kernels one rank of nranks runs for one transform (include/iamrx.h: iamrx_spectrum_slab_bench)"""
    from . import spectrum as _s
    return _s.slab_bench(geom, nranks, reps)


def mf_cospectrum(geom, a, b, acomp=0, bcomp=0):
    """co-spectrum of component acomp of a and bcomp of b, cell-centred MultiFabs that each tile the fully periodic domain of geom
    (include/iamrx.h: iamrx_mf_cospectrum; one packed transform) -> (C_ab, P_a, P_b, count), each (nbins,)"""
    from . import budget as _b
    return _b.mf_cospectrum(geom, a, b, acomp, bcomp)


def mf_noise(geom, mf, seed, comp=0, ncomp=1):
    """white noise of (seed, component, global cell index) in the valid cells (include/iamrx.h: iamrx_mf_noise; spectral.py)"""
    from . import spectral as _s
    return _s.mf_noise(geom, mf, seed, comp, ncomp)


def mf_filter(geom, dst, src, kind, kc, dcomp=0, scomp=0, ncomp=1):
    """dst(dcomp + q) = the low-pass filtered src(scomp + q): kind identity / sharp / gaussian / box (or 0 .. 3), cut-off kc in units of
    2 pi / L_max (include/iamrx.h: iamrx_mf_filter; spectral.py)"""
    from . import spectral as _s
    return _s.mf_filter(geom, dst, src, kind, kc, dcomp, scomp, ncomp)


def mf_sgs(geom, vel, kind, kc, fields=(), vcomp=0, layout=None):
    """a-priori LES analysis of vel(vcomp .. vcomp + 2) under the filter (kind, kc): subgrid stress, inter-scale flux, backscatter and the
    Smagorinsky constants that reproduce them (include/iamrx.h: iamrx_mf_sgs) -> the dict of sgs.as_dict"""
    from . import sgs as _s
    return _s.mf_sgs(geom, vel, kind, kc, fields, vcomp, layout)


def mf_solenoidal(geom, dst, src, wavenumber="centred", dcomp=0, scomp=0):
    """dst(dcomp .. dcomp + 2) = the solenoidal part of src(scomp .. scomp + 2) for the exact or the centred wavenumber
    (include/iamrx.h: iamrx_mf_solenoidal; spectral.py)"""
    from . import spectral as _s
    return _s.mf_solenoidal(geom, dst, src, wavenumber, dcomp, scomp)


def mf_synthesize(geom, dst, E_target, seed=42, wavenumber="centred", comp=0):
    """dst(comp .. comp + 2) = a random solenoidal field with the shell spectrum E_target (include/iamrx.h: iamrx_mf_synthesize;
    spectral.py)"""
    from . import spectral as _s
    return _s.mf_synthesize(geom, dst, E_target, seed, wavenumber, comp)


def mf_spectrum_k2(geom, mf, comp=0, ncomp=1):
    """k^2-weighted power W (ncomp, nbins) of components comp .. comp + ncomp - 1: the spectral |grad f|^2 per shell
    (include/iamrx.h: iamrx_mf_spectrum_k2)"""
    from . import budget as _b
    return _b.mf_spectrum_k2(geom, mf, comp, ncomp)


def convective_term(geom, out, vel, ocomp=0, vcomp=0):
    """out(ocomp .. ocomp + 2) = the skew-symmetric centred nonlinear term N_i = 0.5 sum_d [u_d delta_d u_i + delta_d(u_d u_i)] of
    vel(vcomp .. vcomp + 2), vel with 1 filled ghost layer (include/iamrx.h: iamrx_convective_term)"""
    check(lib().iamrx_convective_term(C.byref(geom), _h(out), int(ocomp), _h(vel), int(vcomp)))


def mf_structure(geom, mf, comp=0, ncomp=1, pmax=4, rmax=None):
    """structure functions and two-point correlations along the axes of components comp .. comp + ncomp - 1 of a cell-centred MultiFab
    whose boxes tile the domain of geom (include/iamrx.h: iamrx_mf_strfn) -> the raw dict of strfn.raw_dict: "avg" (3, ncomp, ncol,
    rcap), "count" (3, rcap) int64, "mean" (ncomp,), "r", "dx", "n", "L", "periodic", "pmax", "rmax".  Collective."""
    from . import strfn as _s
    return _s.mf_structure(geom, mf, comp, ncomp, pmax, rmax)


def mf_histogram(mf, comp=0, ncomp=1, nbins=64, range=None, cov=None, weight=1):
    """exact histograms of components comp .. comp + ncomp - 1 of a cell-centred MultiFab over the valid cells where cov (a cell array
    on the same layout, or None) is zero (include/iamrx.h: iamrx_mf_histogram) -> int64 (ncomp, nbins + 3): the bins, then below,
    above, nan.  range: one (lo, hi) pair for all columns or one per column.  Collective."""
    from . import pdf as _p
    return _p.mf_histogram(mf, comp, ncomp, nbins, range, cov, weight)


def mf_histogram2(mf, compx, compy, nbins=(32, 32), range=None, cov=None, weight=1):
    """exact joint histogram of two components (include/iamrx.h: iamrx_mf_histogram2) -> (int64 (nbx, nby), outside)"""
    from . import pdf as _p
    return _p.mf_histogram2(mf, compx, compy, nbins, range, cov, weight)


def abec_form(geom, coef, op, phi, rhs, out=None, rho=None, rho_comp=0, scale=1.0, bu=(1.0, 1.0, 1.0), beta=1.0, omega=1.15, lobc=(0, 0, 0), hibc=(0, 0, 0),
              maxorder=3):
    """one operation of the multigrid's finest-level kernel forms (include/iamrx.h: iamrx_abec_form)"""
    check(lib().iamrx_abec_form(C.byref(geom), int(coef), _h(rho), int(rho_comp), C.c_double(scale), (C.c_double * 3)(*[float(v) for v in bu]),
                                C.c_double(beta), int(op), phi.h, rhs.h, _h(out), C.c_double(omega), i3(lobc), i3(hibc), int(maxorder)))


def abec_gsrb_sweep(geom, alpha, beta, a, b, phi, rhs, omega=1.15, lobc=(0, 0, 0), hibc=(0, 0, 0), maxorder=2, fused=1):
    check(lib().iamrx_abec_gsrb_sweep(C.byref(geom), C.c_double(alpha), C.c_double(beta), _h(a), b[0].h, b[1].h, b[2].h,
                                      phi.h, rhs.h, C.c_double(omega), i3(lobc), i3(hibc), maxorder, int(fused)))


def abec_residual(geom, alpha, beta, a, b, out, phi, rhs=None, tensor=0):
    check(lib().iamrx_abec_residual(C.byref(geom), C.c_double(alpha), C.c_double(beta), _h(a), b[0].h, b[1].h, b[2].h,
                                    out.h, phi.h, _h(rhs), tensor))


def abec_solve(geom, alpha, beta, a, b, phi, rhs, lobc=(0, 0, 0), hibc=(0, 0, 0), rtol=1e-12, atol=1e-16, opts=None, tensor=0):
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    check(lib().iamrx_abec_solve(C.byref(geom), C.c_double(alpha), C.c_double(beta), _h(a), b[0].h, b[1].h, b[2].h,
                                 phi.h, rhs.h, i3(lobc), i3(hibc), C.c_double(rtol), C.c_double(atol), C.byref(o), tensor, C.byref(st)))
    return st


def abec_solve_cf(geom, alpha, beta, a, b, phi, rhs, crse_phi, cgeom, ratio=2, lobc=(0, 0, 0), hibc=(0, 0, 0), rtol=1e-12, atol=1e-16, opts=None):
    """abec_solve on an AMR level that does not cover the domain: coarse/fine faces take Dirichlet data from crse_phi"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    check(lib().iamrx_abec_solve_cf(C.byref(geom), C.c_double(alpha), C.c_double(beta), _h(a) if a is not None else None, _h(b[0]), _h(b[1]), _h(b[2]),
                                    _h(phi), _h(rhs), i3(lobc), i3(hibc), _h(crse_phi) if crse_phi is not None else None, C.byref(cgeom), ratio,
                                    C.c_double(rtol), C.c_double(atol), C.byref(o), C.byref(st)))
    return st


def mlmg_mac_solve(geom, umac, rho, rho_comp, S, mac_phi, rhs_scale, lobc=(0, 0, 0), hibc=(0, 0, 0),
                   mac_tol=1e-12, mac_abs_tol=1e-16, opts=None):
    """MacProj::mlmg_mac_solve (reference Source/MacProj.cpp:1084-1184)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts(maxorder=4)
    check(lib().iamrx_mlmg_mac_solve(C.byref(geom), umac[0].h, umac[1].h, umac[2].h, rho.h, rho_comp, _h(S), mac_phi.h,
                                     C.c_double(rhs_scale), i3(lobc), i3(hibc), C.c_double(mac_tol), C.c_double(mac_abs_tol),
                                     C.byref(o), C.byref(st)))
    return st


def mlmg_mac_solve_cf(geom, umac, rho, rho_comp, S, mac_phi, rhs_scale, crse_phi, cgeom, ratio=2, lobc=(0, 0, 0), hibc=(0, 0, 0),
                      mac_tol=1e-12, mac_abs_tol=1e-16, opts=None):
    """MAC solve on an AMR level > 0: coarse/fine Dirichlet data from the coarse level's MAC phi (MacProj.cpp:1166-1170)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts(maxorder=4)
    check(lib().iamrx_mlmg_mac_solve_cf(C.byref(geom), umac[0].h, umac[1].h, umac[2].h, rho.h, rho_comp, _h(S), mac_phi.h,
                                        C.c_double(rhs_scale), i3(lobc), i3(hibc), _h(crse_phi), C.byref(cgeom), ratio,
                                        C.c_double(mac_tol), C.c_double(mac_abs_tol), C.byref(o), C.byref(st)))
    return st


def derive_velgrad(geom, out, vel, which, ocomp=0, vcomp=0, mu=0.0, path=0):
    """derived fields of the velocity-gradient tensor (include/iamrx.h: iamrx_derive_velgrad): out(ocomp + q) = quantity which[q] -- ids or
    names of pdf.VELGRAD_NAMES -- of the centred gradient of vel(vcomp .. vcomp + 2), vel with 1 filled ghost layer; mu: the viscosity of
    "dissipation"; path 0: the form the layout asks for, 1 marching, 2 plain"""
    from .pdf import VELGRAD_NAMES
    ids = [VELGRAD_NAMES.index(w) if isinstance(w, str) else int(w) for w in ([which] if isinstance(which, (str, int)) else which)]
    check(lib().iamrx_derive_velgrad(C.byref(geom), _h(out), int(ocomp), len(ids), (C.c_int * max(len(ids), 1))(*ids), _h(vel), int(vcomp),
                                     C.c_double(mu), int(path)))


def velgrad_path(vel, path=0):
    """the form derive_velgrad takes on the layout of vel: 1 marching, 2 plain (path 1 raises where no box holds a full tile)"""
    form = C.c_int()
    check(lib().iamrx_velgrad_path(_h(vel), int(path), C.byref(form)))
    return form.value


def derive_mag_vort(geom, out, vel, ocomp=0, vcomp=0):
    """|curl u| (dermgvort, NS_derive.cpp:86-264); vel with 1 filled ghost cell"""
    check(lib().iamrx_derive_mag_vort(C.byref(geom), _h(out), ocomp, _h(vel), vcomp))


TAG_GREATER, TAG_LESS, TAG_VORT, TAG_GRAD = 0, 1, 2, 3


def error_tag(geom, tags, field, mode, value, comp=0, level=0, realbox=None):
    """one amr.refinement_indicators entry (NS_error.cpp:10-145); tagged cells of `tags` are set to 1"""
    lo = hi = None
    if realbox is not None:
        lo = (C.c_double * 3)(*realbox[0]); hi = (C.c_double * 3)(*realbox[1])
    check(lib().iamrx_error_tag(C.byref(geom), _h(tags), _h(field), comp, mode, C.c_double(value), level, lo, hi))


def cluster_tags(geom, tags, blocking_factor=8, max_grid_size=32, grid_eff=0.7, n_error_buf=1, capacity=4096):
    """Berger-Rigoutsos grid generation from the tags of a level -> [(lo, hi), ...] in the index space of the tags"""
    buf = (C.c_int * (6 * capacity))()
    nb = C.c_int(capacity)
    check(lib().iamrx_cluster_tags(C.byref(geom), _h(tags), blocking_factor, max_grid_size, C.c_double(grid_eff), n_error_buf, buf, C.byref(nb)))
    return [(tuple(buf[6 * q:6 * q + 3]), tuple(buf[6 * q + 3:6 * q + 6])) for q in range(nb.value)]


def mac_sync_solve(geom, mac_reg, rho_half, dt, fine_layout, ucorr, mac_sync_phi, ratio=2, lobc=(0, 0, 0), hibc=(0, 0, 0),
                   tol=1e-10, abs_tol=1e-16, opts=None):
    """MacProj::mac_sync_solve (Source/MacProj.cpp:359-470)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts(maxorder=4)
    check(lib().iamrx_mac_sync_solve(C.byref(geom), mac_reg.h, _h(rho_half), C.c_double(dt), fine_layout.h, ratio, _h(ucorr[0]), _h(ucorr[1]),
                                     _h(ucorr[2]), _h(mac_sync_phi), i3(lobc), i3(hibc), C.c_double(tol), C.c_double(abs_tol), C.byref(o),
                                     C.byref(st)))
    return st


def mac_divergence(geom, div, umac):
    check(lib().iamrx_mac_divergence(C.byref(geom), div.h, umac[0].h, umac[1].h, umac[2].h))


def _bcrec(ncomp, bc=None):
    arr = (C.c_int * (6 * ncomp))()
    if bc is not None:
        for n in range(ncomp):
            lo, hi = bc[n]
            for d in range(3):
                arr[6 * n + d] = int(lo[d])
                arr[6 * n + 3 + d] = int(hi[d])
    return arr


def godunov_extrap_vel_to_faces(geom, vel, force, umac, dt, bc=None, use_forces_in_trans=0, scheme=0):
    """Godunov::ExtrapVelToFaces (reference call site Source/NavierStokesBase.cpp:4487-4491)"""
    check(lib().iamrx_godunov_extrap_vel_to_faces(C.byref(geom), vel.h, _h(force), umac[0].h, umac[1].h, umac[2].h,
                                                  C.c_double(dt), _bcrec(3, bc), use_forces_in_trans, int(scheme)))


def godunov_compute_aofs(geom, aofs, acomp, S, ncomp, force, divu, umac, iconserv, dt, bc=None, is_velocity=0,
                         use_forces_in_trans=0, edge=None, flux=None, scheme=0):
    """kernel chain of NavierStokesBase::ComputeAofs (reference Source/NavierStokesBase.cpp:4594-4845)"""
    ic = (C.c_int * ncomp)(*[int(x) for x in iconserv])
    e = [None] * 3 if edge is None else edge
    f = [None] * 3 if flux is None else flux
    check(lib().iamrx_godunov_compute_aofs(C.byref(geom), aofs.h, acomp, S.h, ncomp, _h(force), _h(divu), umac[0].h, umac[1].h,
                                           umac[2].h, ic, C.c_double(dt), _bcrec(ncomp, bc), is_velocity, use_forces_in_trans,
                                           _h(e[0]), _h(e[1]), _h(e[2]), _h(f[0]), _h(f[1]), _h(f[2]), int(scheme)))


def godunov_compute_aofs_sync(geom, sync, acomp, S, ncomp, force, divu, umac, ucorr, iconserv, dt, bc=None, is_velocity=0,
                              use_forces_in_trans=0, flux=None, scheme=0):
    """NavierStokesBase::ComputeAofs with is_sync = true (reference Source/MacProj.cpp:700-731): edge states traced with umac, fluxes
    formed with ucorr, sync(acomp..) -= -div(F)/vol; flux: all three face arrays or None"""
    ic = (C.c_int * ncomp)(*[int(x) for x in iconserv])
    f = [None] * 3 if flux is None else flux
    check(lib().iamrx_godunov_compute_aofs_sync(C.byref(geom), sync.h, acomp, S.h, ncomp, _h(force), _h(divu), umac[0].h, umac[1].h,
                                                umac[2].h, ucorr[0].h, ucorr[1].h, ucorr[2].h, ic, C.c_double(dt), _bcrec(ncomp, bc),
                                                is_velocity, use_forces_in_trans, _h(f[0]), _h(f[1]), _h(f[2]), int(scheme)))


# ---- Diffusion operator entries on caller-owned data (include/iamrx.h; reference Source/Diffusion.H:53-225) ----------------------------
class DiffusionCrse(C.Structure):
    _fields_ = [("crse_old", C.c_void_p), ("crse_new", C.c_void_p), ("cgeom", C.c_void_p), ("ratio", C.c_int)]


def _mf3(v):
    return (C.c_void_p * 3)(*[m.h for m in v]) if v is not None else None


def _crse(crse):
    """crse = (crse_old or None, crse_new or None, cgeom, ratio) or None"""
    if crse is None:
        return None, None
    co, cn, cg, r = crse
    d = DiffusionCrse(_h(co) if co is not None else None, _h(cn) if cn is not None else None, C.cast(C.pointer(cg), C.c_void_p), int(r))
    return C.byref(d), d


def diffuse_scalar(geom, S_old, S_new, sigma, rho_comp, dt, theta, rho_half, rho_flag, betanp1, betan=None, fluxn=None, fluxnp1=None, delta_rhs=None,
                   rhs_comp=0, lobc=(0, 0, 0), hibc=(0, 0, 0), crse=None, add_old_time_divFlux=True, visc_tol=1e-10, opts=None, Rho_old=None, Rho_new=None):
    """Diffusion::diffuse_scalar (Source/Diffusion.cpp:207-599) on caller-owned MultiFabs"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    cp, keep = _crse(crse)
    check(lib().iamrx_diffuse_scalar(C.byref(geom), _h(S_old), _h(Rho_old), S_new.h, _h(Rho_new), int(sigma), int(rho_comp), C.c_double(dt), C.c_double(theta),
                                     rho_half.h, int(rho_flag), _mf3(fluxn), _mf3(fluxnp1), _h(delta_rhs), int(rhs_comp), _mf3(betan), _mf3(betanp1),
                                     i3(lobc), i3(hibc), cp, int(bool(add_old_time_divFlux)), C.c_double(visc_tol), C.byref(o), C.byref(st)))
    return st


def diffuse_tensor_velocity(geom, U_old, U_new, rho_comp, dt, theta, rho_half, rho_flag, eta_np1, eta_n=None, visc_old_term=None, lobc=(0,) * 9, hibc=(0,) * 9,
                            crse=None, tflux=None, visc_tol=1e-10, opts=None, fill_new=None):
    """Diffusion::diffuse_tensor_velocity (Source/Diffusion.cpp:617-957); fill_new(): refill the ghost cells of U_new once it holds rho u*"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    cp, keep = _crse(crse)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
    cb = CB(lambda ctx, h: fill_new()) if fill_new is not None else C.cast(None, CB)
    check(lib().iamrx_diffuse_tensor_velocity(C.byref(geom), _h(U_old), U_new.h, int(rho_comp), C.c_double(dt), C.c_double(theta), rho_half.h, int(rho_flag),
                                              _h(visc_old_term), _mf3(eta_n), _mf3(eta_np1), (C.c_int * 9)(*lobc), (C.c_int * 9)(*hibc), cp, _mf3(tflux),
                                              C.c_double(visc_tol), C.byref(o), C.byref(st), cb, None))
    return st


def diffuse_tensor_vsync(geom, Vsync, dt, theta, rho_half, rho_flag, eta, bcrec_vel, Rho_old=None, Rho_new=None, rho_comp=3, lobc=(0,) * 9, hibc=(0,) * 9,
                         cgeom=None, ratio=2, tflux=None, visc_tol=1e-10, opts=None):
    """Diffusion::diffuse_tensor_Vsync (Source/Diffusion.cpp:1010-1178)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    check(lib().iamrx_diffuse_tensor_vsync(C.byref(geom), Vsync.h, C.c_double(dt), C.c_double(theta), rho_half.h, int(rho_flag), _h(Rho_old), _h(Rho_new), int(rho_comp),
                                           _mf3(eta), (C.c_int * 9)(*lobc), (C.c_int * 9)(*hibc), (C.c_int * 18)(*bcrec_vel),
                                           C.byref(cgeom) if cgeom is not None else None, int(ratio), _mf3(tflux), C.c_double(visc_tol), C.byref(o), C.byref(st)))
    return st


def diffuse_ssync(geom, Ssync, comp, dt, theta, rho_half, rho_flag, Rho_new, rho_comp, beta, lobc=(0, 0, 0), hibc=(0, 0, 0), cgeom=None, ratio=2, flux=None,
                  visc_tol=1e-10, opts=None):
    """Diffusion::diffuse_Ssync as NavierStokes::mac_sync calls it (Source/NavierStokes.cpp:1590-1640)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    check(lib().iamrx_diffuse_ssync(C.byref(geom), Ssync.h, int(comp), C.c_double(dt), C.c_double(theta), rho_half.h, int(rho_flag), Rho_new.h, int(rho_comp),
                                    _mf3(beta), i3(lobc), i3(hibc), C.byref(cgeom) if cgeom is not None else None, int(ratio), _mf3(flux), C.c_double(visc_tol),
                                    C.byref(o), C.byref(st)))
    return st


class ProjLevel(C.Structure):
    """iamrx_proj_level: a level of a multi-level nodal projection on caller-owned data"""
    _fields_ = [("geom", C.c_void_p), ("layout", C.c_void_p), ("lobc", C.c_int * 3), ("hibc", C.c_int * 3), ("ratio", C.c_int), ("gp", C.c_void_p)]


def mlsync_project(crse, fine, pres_crse, vel_crse, pres_fine, vel_fine, rho_crse, rho_fine, Vsync, V_corr, phi_crse, phi_fine, rhs_sync_reg, dt,
                   crse_sync_reg=None, crse_iteration=1, crse_dt_ratio=1, vcomp_crse=0, vcomp_fine=0, sync_tol=1e-10, abs_tol=1e-16, opts=None):
    """Projection::MLsyncProject (Source/Projection.cpp:457-607) on caller-owned arrays; crse / fine: (geom, layout, lobc, hibc, ratio, gp or None)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    keep = []

    def mk(lv):
        g, lay, lo, hi, r, gp = lv
        keep.append(g)
        return ProjLevel(C.cast(C.pointer(g), C.c_void_p), lay.h, i3(lo), i3(hi), int(r), _h(gp) if gp is not None else None)
    pc, pf = mk(crse), mk(fine)
    check(lib().iamrx_mlsync_project(C.byref(pc), C.byref(pf), pres_crse.h, vel_crse.h, int(vcomp_crse), pres_fine.h, vel_fine.h, int(vcomp_fine), rho_crse.h,
                                     rho_fine.h, Vsync.h, V_corr.h, phi_crse.h, phi_fine.h, rhs_sync_reg.h, crse_sync_reg.h if crse_sync_reg is not None else None,
                                     C.c_double(dt), int(crse_iteration), int(crse_dt_ratio), C.c_double(sync_tol), C.c_double(abs_tol), C.byref(o), C.byref(st)))
    return st


# ---- round 6: MacProj::mac_sync_compute, SyncRegister::CompAdd, Projection::initial*Project on caller-owned data ----------------------
def mac_sync_compute(geom, ucorr, Vsync, Ssync, S_vel, S_scal, nscal, gradp, umac, iconserv_scal, dt, visc_vel=None, tforce_scal=None, divu=None,
                     do_mom_diff=0, gravity=0.0, bc_vel=None, bc_scal=None, use_forces_in_trans=0, scheme=0, flux_vel=None, flux_scal=None):
    """MacProj::mac_sync_compute as NavierStokes::mac_sync calls it (Source/MacProj.cpp:488-731)"""
    ic = (C.c_int * nscal)(*[int(x) for x in iconserv_scal])
    fv = [None] * 3 if flux_vel is None else flux_vel
    fs = [None] * 3 if flux_scal is None else flux_scal
    check(lib().iamrx_mac_sync_compute(C.byref(geom), ucorr[0].h, ucorr[1].h, ucorr[2].h, Vsync.h, Ssync.h, S_vel.h, S_scal.h, int(nscal), _h(visc_vel),
                                       _h(tforce_scal), gradp.h, _h(divu), umac[0].h, umac[1].h, umac[2].h, ic, int(do_mom_diff), C.c_double(gravity),
                                       C.c_double(dt), _bcrec(3, bc_vel), _bcrec(nscal, bc_scal), int(use_forces_in_trans), int(scheme),
                                       _h(fv[0]), _h(fv[1]), _h(fv[2]), _h(fs[0]), _h(fs[1]), _h(fs[2])))


def mac_sync_compute_edge(geom, ucorr, Sync, sync_indx, edge, edge_comp, flux=None):
    """MacProj::mac_sync_compute with known edge states (Source/MacProj.cpp:733-786)"""
    f = [None] * 3 if flux is None else flux
    check(lib().iamrx_mac_sync_compute_edge(C.byref(geom), ucorr[0].h, ucorr[1].h, ucorr[2].h, Sync.h, int(sync_indx), edge[0].h, edge[1].h, edge[2].h,
                                            int(edge_comp), _h(f[0]), _h(f[1]), _h(f[2])))


def _proj_levels(levels, keep):
    arr = (ProjLevel * len(levels))()
    for q, (g, lay, lo, hi, r, gp) in enumerate(levels):
        keep.append(g)
        arr[q] = ProjLevel(C.cast(C.pointer(g), C.c_void_p), lay.h, i3(lo), i3(hi), int(r), _h(gp) if gp is not None else None)
    return arr


def _hv(mfs, n):
    a = (C.c_void_p * n)()
    for q in range(n):
        a[q] = None if (mfs is None or mfs[q] is None) else mfs[q].h
    return a


def initial_velocity_project(levels, vel, vcomp, pres, rho=None, rho_comp=None, divu=None, divu_comp=None, proj_tol=1e-12, proj_abs_tol=1e-16, opts=None):
    """Projection::initialVelocityProject (Source/Projection.cpp:615-838); levels: [(geom, layout, lobc, hibc, ratio, gp or None)], coarsest first"""
    n = len(levels)
    st = MgStats(); o = opts if opts is not None else mg_opts(); keep = []
    pl = _proj_levels(levels, keep)
    vc = (C.c_int * n)(*[int(v) for v in vcomp])
    rc = (C.c_int * n)(*[int(v) for v in (rho_comp or [0] * n)])
    dc = (C.c_int * n)(*[int(v) for v in (divu_comp or [0] * n)])
    check(lib().iamrx_initial_velocity_project(n, pl, _hv(vel, n), vc, _hv(pres, n), _hv(rho, n) if rho is not None else None, rc,
                                               _hv(divu, n) if divu is not None else None, dc, C.c_double(proj_tol), C.c_double(proj_abs_tol), C.byref(o), C.byref(st)))
    return st


def initial_sync_project(levels, vel_new, vcomp, vel_old, phi, rho_half, dt, pres_new=None, divu_new=None, divu_old=None, divu_comp=None, proj_tol=1e-12,
                         proj_abs_tol=1e-16, opts=None):
    """Projection::initialSyncProject (Source/Projection.cpp:970-1185)"""
    n = len(levels)
    st = MgStats(); o = opts if opts is not None else mg_opts(); keep = []
    pl = _proj_levels(levels, keep)
    vc = (C.c_int * n)(*[int(v) for v in vcomp])
    dc = (C.c_int * n)(*[int(v) for v in (divu_comp or [0] * n)])
    check(lib().iamrx_initial_sync_project(n, pl, _hv(vel_new, n), vc, _hv(vel_old, n), _hv(phi, n), _hv(pres_new, n) if pres_new is not None else None,
                                           _hv(rho_half, n), _hv(divu_new, n) if divu_new is not None else None,
                                           _hv(divu_old, n) if divu_old is not None else None, dc, C.c_double(dt), C.c_double(proj_tol),
                                           C.c_double(proj_abs_tol), C.byref(o), C.byref(st)))
    return st
