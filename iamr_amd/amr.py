"""Hierarchy of NavierStokes levels (ctypes view of iamrx_amr_*; include/iamrx.h): Amr::coarseTimeStep with subcycling,
NavierStokesBase::post_timestep (reflux, avgDown, mac_sync, level_sync) and the multi-level NavierStokes::post_init.  What the run driver,
the checkpoint writer and the particle container read of a run -- levels, layouts, nlev, level_geom, ratio, time, dts, particles,
plane_profile, spectrum, structure_functions -- a single NavierStokes level offers under the same names (ns.py)."""
import ctypes as C
from .lib import lib, check, mg_opts, MgStats
from .ns import NavierStokes, ns_params


class TagRule(C.Structure):
    _fields_ = [("comp", C.c_int), ("mode", C.c_int), ("nvalue", C.c_int), ("max_level", C.c_int), ("has_box", C.c_int),
                ("value", C.c_double * 8), ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3)]


class _Level(NavierStokes):
    """a level borrowed from an Amr hierarchy (never destroyed on its own)"""

    def __init__(self, handle, geom, layout, params, opts):
        self.geom = geom
        self.layout = layout
        self.params = params
        self.opts = opts
        self.h = handle

    def __del__(self):
        pass


class Amr:
    def __init__(self, geom0, layouts, params=None, opts=None, ratio=2):
        self.geom0 = geom0
        self.layouts = list(layouts)
        self.ratio = ratio
        self.params = params if params is not None else ns_params()
        self.opts = opts if opts is not None else mg_opts()
        self.h = C.c_void_p()
        arr = (C.c_void_p * len(self.layouts))(*[l.h for l in self.layouts])
        check(lib().iamrx_amr_create(C.byref(geom0), len(self.layouts), arr, int(ratio), C.byref(self.params), C.byref(self.opts), C.byref(self.h)))
        self.levels = []
        self._refresh(keep_layouts=True)
        if getattr(self.params, "turb_forcing", 0):
            self.set_turb_forcing(self.params.turb_nmodes, self.params.turb_mode_start, self.params.turb_div_free)

    def set_turb_forcing(self, nmodes=4, mode_start=0, div_free=1, on=1):
        """switch the turbulent forcing on for every level, with upstream's mode table for the level-0 domain (iamrx_amr_set_turb_forcing)"""
        check(lib().iamrx_amr_set_turb_forcing(self.h, int(on), int(nmodes), int(mode_start), int(div_free)))

    def set_particles(self, pc):
        """attach ONE tracer-particle container to the hierarchy (particles.Particles; None: detach): it is rebound to the levels' boxes,
        now and after every regrid; every level moves its particles at the end of its advance, post_timestep and post_regrid redistribute
        (NavierStokes::advance, post_timestep_particle, post_regrid; include/iamrx.h: iamrx_amr_set_particles)"""
        check(lib().iamrx_amr_set_particles(self.h, None if pc is None else pc.h))
        self._particles = pc

    @property
    def particles(self):
        return getattr(self, "_particles", None)

    def _refresh(self, keep_layouts=False):
        """(re)build the Python views of the levels; after a regrid the layouts are re-created from the hierarchy's box lists"""
        from .lib import Layout
        n = C.c_int()
        check(lib().iamrx_amr_nlevels(self.h, C.byref(n)))
        if not keep_layouts:
            lays = [self.layouts[0]]
            for l in range(1, n.value):
                nb = C.c_int(0)
                check(lib().iamrx_amr_level_boxes(self.h, l, C.byref(nb), None))
                arr = (C.c_int * (6 * nb.value))()
                check(lib().iamrx_amr_level_boxes(self.h, l, C.byref(nb), arr))
                hl = C.c_void_p()
                check(lib().iamrx_amr_level_layout(self.h, l, C.byref(hl)))
                own = (C.c_int * max(1, nb.value))()
                check(lib().iamrx_layout_owners(hl, own))            # who the regrid's knapsack gave every box to
                lays.append(Layout.from_handle(hl, [(tuple(arr[6 * q:6 * q + 3]), tuple(arr[6 * q + 3:6 * q + 6])) for q in range(nb.value)], list(own[:nb.value])))
            self.layouts = lays
        self.levels = []
        for l in range(n.value):
            hl = C.c_void_p()
            check(lib().iamrx_amr_level(self.h, l, C.byref(hl)))
            self.levels.append(_Level(hl, self.level_geom(l), self.layouts[l], self.params, self.opts))

    def set_turb_modes(self, kxyz, data, div_free=1):
        """switch the turbulent forcing on for every level with the caller's table (NavierStokes.set_turb_modes for the hierarchy)"""
        from .lib import _turb_table
        M, k, d = _turb_table(kxyz, data)
        check(lib().iamrx_amr_set_turb_modes(self.h, M, k, d, int(div_free)))

    def set_regrid(self, max_level, regrid_int, rules, blocking_factor=8, max_grid_size=32, grid_eff=0.7, n_error_buf=1, compute_new_dt_on_regrid=0,
                   do_refine_outflow=0, do_derefine_outflow=1, nbuf_outflow=1):
        """rules: list of dicts(comp (0..4, -1 = mag_vort), mode (0 greater, 1 less, 2 vorticity, 3 adjacent difference), value (list per level),
        max_level (optional), box_lo / box_hi (optional)) -- amr.refinement_indicators of NS_error.cpp"""
        arr = (TagRule * max(1, len(rules)))()
        for q, r in enumerate(rules):
            arr[q].comp, arr[q].mode = int(r.get("comp", 4)), int(r.get("mode", 0))
            vals = list(r["value"]) if hasattr(r["value"], "__len__") else [r["value"]]
            arr[q].nvalue = len(vals)
            for i, v in enumerate(vals[:8]):
                arr[q].value[i] = float(v)
            arr[q].max_level = int(r.get("max_level", 1000))
            arr[q].has_box = 1 if "box_lo" in r else 0
            for d in range(3):
                arr[q].box_lo[d] = float(r.get("box_lo", (0, 0, 0))[d])
                arr[q].box_hi[d] = float(r.get("box_hi", (0, 0, 0))[d])
        check(lib().iamrx_amr_set_regrid(self.h, int(max_level), int(regrid_int), int(blocking_factor), int(max_grid_size), C.c_double(grid_eff),
                                         int(n_error_buf), len(rules), arr))
        check(lib().iamrx_amr_set_compute_new_dt_on_regrid(self.h, int(compute_new_dt_on_regrid)))
        check(lib().iamrx_amr_set_outflow_tagging(self.h, int(do_refine_outflow), int(do_derefine_outflow), int(nbuf_outflow)))

    def regrid_log(self):
        """[(lbase, time, [boxes of level lbase + 1, boxes of level lbase + 2, ...]), ...] of the last coarse step"""
        n = C.c_int()
        check(lib().iamrx_amr_regrid_log_count(self.h, C.byref(n)))
        out = []
        for e in range(n.value):
            lb, tm, nl = C.c_int(), C.c_double(), C.c_int()
            nb = (C.c_int * 8)()
            check(lib().iamrx_amr_regrid_log_event(self.h, e, C.byref(lb), C.byref(tm), C.byref(nl), nb, None))
            tot = sum(nb[q] for q in range(nl.value))
            arr = (C.c_int * (6 * max(tot, 1)))()
            check(lib().iamrx_amr_regrid_log_event(self.h, e, C.byref(lb), C.byref(tm), C.byref(nl), nb, arr))
            grids, q = [], 0
            for l in range(nl.value):
                grids.append([(tuple(arr[6 * (q + b):6 * (q + b) + 3]), tuple(arr[6 * (q + b) + 3:6 * (q + b) + 6])) for b in range(nb[l])])
                q += nb[l]
            out.append((lb.value, tm.value, grids))
        return out

    def regrid(self):
        ch = C.c_int()
        check(lib().iamrx_amr_regrid(self.h, C.byref(ch)))
        if ch.value:
            self._refresh()
        return bool(ch.value)

    def install_grids(self, grids):
        """grids: per refined level the list of (lo, hi) boxes in that level's index space"""
        nb = (C.c_int * max(1, len(grids)))(*[len(g) for g in grids])
        flat = [v for g in grids for lo, hi in g for v in (*lo, *hi)]
        arr = (C.c_int * max(1, len(flat)))(*flat)
        ch = C.c_int()
        check(lib().iamrx_amr_install_grids(self.h, len(grids), nb, arr, C.byref(ch)))
        if ch.value:
            self._refresh()
        return bool(ch.value)

    def level_geom(self, l):
        from .lib import Geom
        n = [self.geom0.n[d] * self.ratio ** l for d in range(3)]
        return Geom.make(n, tuple(self.geom0.prob_lo), tuple(self.geom0.prob_hi), tuple(self.geom0.periodic))

    @property
    def nlev(self):
        return len(self.layouts)

    def post_init(self, stop_time=-1.0):
        check(lib().iamrx_amr_post_init(self.h, C.c_double(stop_time)))

    def coarse_step(self):
        dt = C.c_double()
        check(lib().iamrx_amr_coarse_step(self.h, C.byref(dt)))
        n = C.c_int()
        check(lib().iamrx_amr_nlevels(self.h, C.byref(n)))
        if n.value != len(self.levels) or self._grids_changed():
            self._refresh()
        return dt.value

    def _grids_changed(self):
        for l in range(1, len(self.levels)):
            nb = C.c_int(0)
            check(lib().iamrx_amr_level_boxes(self.h, l, C.byref(nb), None))
            arr = (C.c_int * (6 * max(1, nb.value)))()
            check(lib().iamrx_amr_level_boxes(self.h, l, C.byref(nb), arr))
            now = [(tuple(arr[6 * q:6 * q + 3]), tuple(arr[6 * q + 3:6 * q + 6])) for q in range(nb.value)]
            if now != self.layouts[l].boxes:
                return True
        return False

    @property
    def time(self):
        t = C.c_double()
        check(lib().iamrx_amr_time(self.h, C.byref(t), None))
        return t.value

    def dts(self):
        arr = (C.c_double * self.nlev)()
        check(lib().iamrx_amr_time(self.h, None, arr))
        return list(arr)

    def sum_integrated(self):
        """(mass, tracer, kinetic energy) of the composite grid now (NavierStokes::sum_integrated_quantities, NavierStokes.cpp:1046-1079)"""
        v = (C.c_double * 3)()
        check(lib().iamrx_amr_sum_integrated(self.h, v))
        return tuple(v)

    def integrate(self, names):
        """composite volume-weighted sums of named fields (include/iamrx.h: iamrx_amr_integrate; the names of histogram): every level
        over the cells the next finer one does not cover -> float64 array, one per name.  Collective; the same on every rank."""
        import numpy as np
        names = [names] if isinstance(names, str) else list(names)
        out = np.zeros(max(len(names), 1))
        check(lib().iamrx_amr_integrate(self.h, len(names), (C.c_char_p * max(len(names), 1))(*[nm.encode() for nm in names]),
                                        out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:len(names)]

    def last_sum(self):
        """(level-0 step, time, (mass, tracer, kinetic energy)) the hierarchy last computed by itself (ns.sum_interval > 0: after post_init and
        in level 0's post_timestep), or None"""
        st, tm, v = C.c_int(), C.c_double(), (C.c_double * 3)()
        check(lib().iamrx_amr_last_sum(self.h, C.byref(st), C.byref(tm), v))
        return None if st.value < 0 else (st.value, tm.value, tuple(v))

    def plane_profile(self, dir, bin_level=0):
        """plane-averaged profile of the composite state along dir (0, 1, 2) in the slabs of level bin_level (0 .. finest), over the cells
        no finer level covers (include/iamrx.h: iamrx_amr_plane_profile) -> dict name -> array of nbins for the 14 names of
        profile.NAMES, plus "coord" (bin centres in physical units) and "names"; the same on every rank.  (`profile` is the section timer.)"""
        import numpy as np
        from . import profile as _p
        ok = 0 <= int(dir) <= 2 and 0 <= int(bin_level) < 30
        cap = int(self.geom0.n[dir]) * self.ratio ** int(bin_level) if ok else 1
        out, n = np.zeros(len(_p.NAMES) * cap), C.c_int()
        check(lib().iamrx_amr_plane_profile(self.h, int(dir), int(bin_level), cap, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return _p.as_dict(out, n.value, self.geom0.prob_lo[dir], self.geom0.prob_hi[dir], dir, bin_level)

    def spectrum(self):
        """shell-summed spectra of LEVEL 0 of the hierarchy (after avgDown its covered cells hold the average of the finer data;
        include/iamrx.h: iamrx_amr_spectrum) -> the dict of NavierStokes.spectrum; the same bits on every rank.  Collective."""
        from . import spectrum as _s
        return _s.level_spectrum(lib().iamrx_amr_spectrum, self.h, self.geom0)

    def plane_spectrum(self, dir):
        """ring-summed plane spectra of LEVEL 0 of the hierarchy (as spectrum takes its level; include/iamrx.h:
        iamrx_amr_plane_spectrum) -> the dict of NavierStokes.plane_spectrum; the same bits on every rank.  Collective."""
        from . import planespec as _p
        return _p.level_plane_spectrum(lib().iamrx_amr_plane_spectrum, self.h, self.geom0, dir)

    def filtered(self, names, kind, kc):
        """the named fields of LEVEL 0 of the hierarchy (as spectrum takes its level) low-pass filtered into a new MultiFab on that
        level's layout -> NavierStokes.filtered of level 0.  Collective."""
        return self.levels[0].filtered(names, kind, kc)

    def sgs(self, kind, kc, fields=()):
        """a-priori LES analysis of LEVEL 0 of the hierarchy (as spectrum takes its level; include/iamrx.h: iamrx_amr_sgs) -> the dict of
        NavierStokes.sgs, the fields on the layout of level 0; the same bits on every rank.  Collective."""
        from . import sgs as _g
        return _g.level_sgs(lib().iamrx_amr_sgs, self.h, self.geom0, self.layouts[0], kind, kc, fields)

    def spectral_budget(self):
        """spectral kinetic-energy budget of LEVEL 0 of the hierarchy (as spectrum takes its level; include/iamrx.h:
        iamrx_amr_spectral_budget) -> the dict of NavierStokes.spectral_budget; the same bits on every rank.  Collective."""
        from . import budget as _b
        return _b.level_budget(lib().iamrx_amr_spectral_budget, self.h, self.geom0, self.params.visc_coef)

    def structure_functions(self, pmax=4, rmax=None):
        """structure functions and two-point correlations of LEVEL 0 of the hierarchy (as spectrum takes its level; include/iamrx.h:
        iamrx_amr_strfn) -> the dict of NavierStokes.structure_functions; the same bits on every rank.  Collective."""
        from . import strfn as _s
        return _s.level_structure(lib().iamrx_amr_strfn, self.h, self.geom0, pmax, rmax)

    def histogram(self, names, nbins=64, range=None):
        """composite histograms and PDFs of named fields (include/iamrx.h: iamrx_amr_histogram; pdf.py): level l counts the cells level
        l + 1 does not cover with the weight 8^(finest - l), so the counts are in finest-level cell volumes -> the dict of
        NavierStokes.histogram.  range None: each field's minimum and maximum over the valid cells of all levels.  Collective."""
        from . import pdf as _p
        return _p.histogram(self, lib().iamrx_amr_histogram, names, nbins, range)

    def histogram2(self, namex, namey, nbins=(32, 32), range=None):
        """composite joint histogram of two named fields (include/iamrx.h: iamrx_amr_histogram2) -> the dict of NavierStokes.histogram2"""
        from . import pdf as _p
        return _p.histogram2(self, lib().iamrx_amr_histogram2, namex, namey, nbins, range)

    def profile(self, enable):
        """-> (hierarchy sections [16], per-level sections [nlev][8]) accumulated so far; then enable: 1 reset + start, 0 stop, -1 keep"""
        sec = (C.c_double * 16)()
        lv = (C.c_double * (8 * self.nlev))()
        check(lib().iamrx_amr_profile(self.h, int(enable), sec, lv))
        return list(sec), [list(lv[8 * l:8 * l + 8]) for l in range(self.nlev)]

    def sync_stats(self):
        a, b = MgStats(), MgStats()
        check(lib().iamrx_amr_sync_stats(self.h, C.byref(a), C.byref(b)))
        return a, b

    def __del__(self):
        try:
            if self.h:
                self.levels = []
                lib().iamrx_amr_destroy(self.h)
        except Exception:
            pass
