"""Python mirror of the operator layer for tests / bench: nodal projection, tensor diffusion and the
NavierStokes level object, all thin wrappers over the C-ABI (include/iamrx.h)."""
import ctypes as C
from .lib import lib, check, i3, mg_opts, MgStats, MultiFab, _h


class NsParams(C.Structure):
    _fields_ = [("cfl", C.c_double), ("visc_coef", C.c_double), ("be_cn_theta", C.c_double), ("gravity", C.c_double),
                ("mac_tol", C.c_double), ("mac_abs_tol", C.c_double), ("proj_tol", C.c_double),
                ("proj_abs_tol", C.c_double), ("visc_tol", C.c_double),
                ("use_forces_in_trans", C.c_int), ("do_mom_diff", C.c_int), ("init_iter", C.c_int),
                ("init_vel_iter", C.c_int), ("init_shrink", C.c_double), ("change_max", C.c_double),
                ("fixed_dt", C.c_double), ("nscal", C.c_int), ("verbose", C.c_int),
                ("init_dt", C.c_double), ("tracer_diff_coef", C.c_double), ("phys_lo", C.c_int * 3), ("phys_hi", C.c_int * 3),
                ("wall_vel_lo", C.c_double * 9), ("wall_vel_hi", C.c_double * 9),
                ("scal_bc_lo", C.c_double * 12), ("scal_bc_hi", C.c_double * 12), ("do_cons_trac", C.c_int), ("do_denminmax", C.c_int), ("do_scalminmax", C.c_int),
                ("do_trac2", C.c_int), ("do_cons_trac2", C.c_int), ("tracer2_diff_coef", C.c_double), ("do_temp", C.c_int), ("temp_cond_coef", C.c_double), ("use_ppm", C.c_int),
                ("avg_interval", C.c_int), ("compute_fluctuations", C.c_int), ("sum_interval", C.c_int),
                ("do_LES", C.c_int), ("LES_model", C.c_int), ("smago_Cs_cst", C.c_double), ("sigma_Cs_cst", C.c_double)]


def ns_params(**kw):
    p = NsParams()
    lib().iamrx_ns_default_params(C.byref(p))
    # ns.avg_in_checkpoint (NavierStokesBase.cpp:539) only steers amr.restart (checkpoint.restart): it travels with the parameters as a
    # plain attribute, the library's struct does not hold it
    p.avg_in_checkpoint = int(kw.pop("avg_in_checkpoint", 1))
    # the turbulent forcing (Tutorials/HIT) is set on the level or the hierarchy after its creation (iamrx_ns_set_turb_forcing /
    # iamrx_amr_set_turb_forcing; the library's struct keeps its layout): the four values travel the same way and NavierStokes / Amr apply them
    p.turb_forcing, p.turb_nmodes = int(kw.pop("turb_forcing", 0)), int(kw.pop("turb_nmodes", 4))
    p.turb_mode_start, p.turb_div_free = int(kw.pop("turb_mode_start", 0)), int(kw.pop("turb_div_free", 1))
    for k, v in kw.items():
        if k in ("phys_lo", "phys_hi"):
            setattr(p, k, (C.c_int * 3)(*[int(x) for x in v]))
        elif k in ("wall_vel_lo", "wall_vel_hi"):
            setattr(p, k, (C.c_double * 9)(*[float(x) for x in v]))
        elif k in ("scal_bc_lo", "scal_bc_hi"):        # [d*4+n]; a 6-entry list is the two-scalar layout [d*2+n]
            v = [float(x) for x in v]
            if len(v) == 6:
                v = [v[2 * d + n] if n < 2 else 0.0 for d in range(3) for n in range(4)]
            setattr(p, k, (C.c_double * 12)(*v))
        else:
            setattr(p, k, v)
    return p


def nodal_residual(geom, out, phi, sig, rhs=None):
    check(lib().iamrx_nodal_residual(C.byref(geom), out.h, phi.h, sig.h, _h(rhs)))


def nodal_residual_images(geom, out, phi, sig, rhs=None, lobc=(0, 0, 0), hibc=(0, 0, 0)):
    """nodal_residual with image reads instead of phi's ghost nodes (one box spanning a periodic / Neumann-walled domain); returns max |out|"""
    norm = C.c_double()
    check(lib().iamrx_nodal_residual_images(C.byref(geom), out.h, phi.h, sig.h, _h(rhs), i3(lobc), i3(hibc), C.byref(norm)))
    return norm.value


def nodal_gs_color(geom, phi, rhs, sig, color):
    check(lib().iamrx_nodal_gs_color(C.byref(geom), phi.h, rhs.h, sig.h, color))


def nodal_gs_sweep(geom, phi, rhs, sig, fused=1):
    """one 8-colour Gauss-Seidel sweep incl. ghost fills (fused: plane-fused two-pass variant, same arithmetic)"""
    check(lib().iamrx_nodal_gs_sweep(C.byref(geom), phi.h, rhs.h, sig.h, int(fused)))


def nodal_restrict(crse, fine):
    check(lib().iamrx_nodal_restrict(crse.h, fine.h))


def nodal_restrict_images(geom, crse, fine, lobc=(0, 0, 0), hibc=(0, 0, 0)):
    """nodal_restrict with image reads instead of fine's ghost nodes; geom: the fine level's"""
    check(lib().iamrx_nodal_restrict_images(C.byref(geom), crse.h, fine.h, i3(lobc), i3(hibc)))


def nodal_interp_add(fine, crse, sig_fine):
    check(lib().iamrx_nodal_interp_add(fine.h, crse.h, sig_fine.h))


def nodal_divu(geom, rhs, vel, vcomp=0, lobc=None, hibc=None):
    """lobc / hibc: LinOp codes of the non-periodic faces (Neumann wall, inflow); None: every non-periodic face is a wall"""
    if lobc is None and hibc is None:
        check(lib().iamrx_nodal_divu(C.byref(geom), rhs.h, vel.h, vcomp))
    else:
        check(lib().iamrx_nodal_divu_bc(C.byref(geom), rhs.h, vel.h, vcomp, i3(lobc), i3(hibc)))


def nodal_compgrad(geom, gp, phi):
    """MLNodeLaplacian::compGrad (NavierStokesBase::computeGradP, reference Source/NavierStokesBase.cpp:4102-4122)"""
    check(lib().iamrx_nodal_compgrad(C.byref(geom), gp.h, phi.h))


def nodal_solve(geom, phi, rhs, sig, sig_comp=0, lobc=(0, 0, 0), hibc=(0, 0, 0), rel_tol=1e-12, abs_tol=1e-16, opts=None):
    """div(sig grad phi) = rhs; Dirichlet nodes (outflow faces, boundary of a level that does not cover the domain) keep phi"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    check(lib().iamrx_nodal_solve(C.byref(geom), _h(phi), _h(rhs), _h(sig), sig_comp, i3(lobc), i3(hibc),
                                      C.c_double(rel_tol), C.c_double(abs_tol), C.byref(o), C.byref(st)))
    return st


def nodal_projection(geom, vel, vcomp, phi, sig, sig_comp=0, lobc=(0, 0, 0), hibc=(0, 0, 0), rel_tol=1e-12, abs_tol=1e-16,
                     opts=None, gp=None, increment_gp=False):
    """Projection::doMLMGNodalProjection on one level (reference Source/Projection.cpp:2385-2567)"""
    st = MgStats()
    o = opts if opts is not None else mg_opts()
    check(lib().iamrx_nodal_projection(C.byref(geom), vel.h, vcomp, phi.h, sig.h, sig_comp, i3(lobc), i3(hibc),
                                       C.c_double(rel_tol), C.c_double(abs_tol), C.byref(o), _h(gp), int(increment_gp), C.byref(st)))
    return st


def _bcn(lobc, hibc):
    """(lo, hi, nbc): lobc/hibc are 3 codes, or 3 x 3 codes (one triple per velocity component)"""
    if hasattr(lobc[0], "__len__"):
        flat_lo = [int(v) for c in lobc for v in c]
        flat_hi = [int(v) for c in hibc for v in c]
        return (C.c_int * 9)(*flat_lo), (C.c_int * 9)(*flat_hi), 3
    return i3(lobc), i3(hibc), 1


def tensor_apply(geom, out, vel, a, b, acoef, eta, lobc=(0, 0, 0), hibc=(0, 0, 0), maxorder=2):
    lo, hi, nbc = _bcn(lobc, hibc)
    check(lib().iamrx_tensor_apply(C.byref(geom), out.h, vel.h, C.c_double(a), C.c_double(b), _h(acoef), eta[0].h, eta[1].h,
                                   eta[2].h, lo, hi, nbc, maxorder))


def tensor_solve(geom, soln, rhs, a, b, acoef, eta, lobc=(0, 0, 0), hibc=(0, 0, 0), tol_rel=1e-10, tol_abs=0.0, opts=None):
    st = MgStats()
    o = opts if opts is not None else mg_opts(maxorder=2)
    lo, hi, nbc = _bcn(lobc, hibc)
    check(lib().iamrx_tensor_solve(C.byref(geom), soln.h, rhs.h, C.c_double(a), C.c_double(b), _h(acoef), eta[0].h, eta[1].h,
                                   eta[2].h, lo, hi, nbc, C.c_double(tol_rel), C.c_double(tol_abs), C.byref(o), C.byref(st)))
    return st


def tensor_extensive_flux(geom, vel, eta, flux, fac, add=False):
    """Diffusion::computeExtensiveFluxes on the tensor operator (include/iamrx.h: iamrx_tensor_extensive_flux): flux[d] (3 comps on the
    d-faces) = or += fac * area_d * (-eta_d (4/3 if n == d) du_n/dx_d + cross terms); vel as tensor_apply / tensor_solve left it"""
    check(lib().iamrx_tensor_extensive_flux(C.byref(geom), vel.h, eta[0].h, eta[1].h, eta[2].h, flux[0].h, flux[1].h, flux[2].h,
                                            C.c_double(fac), int(bool(add))))


def tensor_apply_cf(geom, out, vel, a, b, acoef, eta, crse_vel, cgeom, ratio=2, lobc=(0, 0, 0), hibc=(0, 0, 0), maxorder=2):
    """tensor operator on a refined level (tensorop.setCoarseFineBC(&crsedata, ratio), Source/Diffusion.cpp:1725-1736); crse_vel None: homogeneous"""
    lo, hi, nbc = _bcn(lobc, hibc)
    check(lib().iamrx_tensor_apply_cf(C.byref(geom), out.h, vel.h, C.c_double(a), C.c_double(b), _h(acoef), eta[0].h, eta[1].h,
                                      eta[2].h, lo, hi, nbc, maxorder, _h(crse_vel), C.byref(cgeom), int(ratio)))


def tensor_solve_cf(geom, soln, rhs, a, b, acoef, eta, crse_vel, cgeom, ratio=2, lobc=(0, 0, 0), hibc=(0, 0, 0), tol_rel=1e-10, tol_abs=0.0,
                    opts=None):
    st = MgStats()
    o = opts if opts is not None else mg_opts(maxorder=2)
    lo, hi, nbc = _bcn(lobc, hibc)
    check(lib().iamrx_tensor_solve_cf(C.byref(geom), soln.h, rhs.h, C.c_double(a), C.c_double(b), _h(acoef), eta[0].h, eta[1].h,
                                      eta[2].h, lo, hi, nbc, _h(crse_vel), C.byref(cgeom), int(ratio), C.c_double(tol_rel), C.c_double(tol_abs),
                                      C.byref(o), C.byref(st)))
    return st


SMAGORINSKY, SIGMA = 0, 1        # ns.LES_model


def les_mut(geom, vel, mu, model, Cs, base=0.0, vcomp=0):
    """k_les_mut alone: mu[d] = base + mu_t from vel(vcomp..vcomp+2) and its ghost cells as they are (the model loops of
    NavierStokesBase::calc_mut_LES, Source/NS_LES.cpp:105-222)"""
    check(lib().iamrx_les_mut(C.byref(geom), vel.h, int(vcomp), int(model), C.c_double(Cs), C.c_double(base), mu[0].h, mu[1].h, mu[2].h))


def calc_mut_les(geom, vel, mu, model, Cs, lobc=((0, 0, 0),) * 3, hibc=((0, 0, 0),) * 3, maxorder=3, crse_vel=None, cgeom=None, ratio=2):
    """NavierStokesBase::calc_mut_LES (Source/NS_LES.cpp:22-225) on caller data: the tensor operator's boundary step on vel (3 comps, 1 ghost),
    then the kernel; cgeom given: a refined level (crse_vel None: homogeneous coarse/fine data)"""
    lo, hi, nbc = _bcn(lobc, hibc)
    assert nbc == 3
    if cgeom is None:
        check(lib().iamrx_calc_mut_les(C.byref(geom), vel.h, lo, hi, int(maxorder), int(model), C.c_double(Cs), mu[0].h, mu[1].h, mu[2].h))
    else:
        check(lib().iamrx_calc_mut_les_cf(C.byref(geom), vel.h, lo, hi, int(maxorder), int(model), C.c_double(Cs), mu[0].h, mu[1].h, mu[2].h,
                                          _h(crse_vel), C.byref(cgeom), int(ratio)))


class NavierStokes:
    """level object with the reference's method names (NavierStokes::advance, post_init, ...)"""
    S_NEW, S_OLD, P_NEW, P_OLD, GP_NEW, GP_OLD, UMAC_X, UMAC_Y, UMAC_Z, AOFS = range(10)
    ETA_N, ETA_NP1 = 13, 16   # + direction: the face viscosities visc_coef + mu_t of the last velocity_diffusion_update (do_LES = 1)
    AVERAGE = 12          # the time-average accumulators (Average_Type, NS_setup.cpp:389-405): 6 components, no ghost cells
    VEL_AVG_NAMES = ["x_vel_average", "y_vel_average", "z_vel_average", "x_vel_rms", "y_vel_rms", "z_vel_rms"]   # NS_setup.cpp:417-427
    _types = {0: ((0, 0, 0), 5, 1), 1: ((0, 0, 0), 5, 1), 2: ((1, 1, 1), 1, 1), 3: ((1, 1, 1), 1, 1), 4: ((0, 0, 0), 3, 1),
              5: ((0, 0, 0), 3, 1), 6: ((1, 0, 0), 1, 1), 7: ((0, 1, 0), 1, 1), 8: ((0, 0, 1), 1, 1), 9: ((0, 0, 0), 5, 0),
              12: ((0, 0, 0), 6, 0), 13: ((1, 0, 0), 1, 0), 14: ((0, 1, 0), 1, 0), 15: ((0, 0, 1), 1, 0), 16: ((1, 0, 0), 1, 0),
              17: ((0, 1, 0), 1, 0), 18: ((0, 0, 1), 1, 0)}

    def __init__(self, geom, layout, params=None, opts=None):
        self.geom = geom
        self.layout = layout
        self.params = params if params is not None else ns_params()
        self.opts = opts if opts is not None else mg_opts()
        self.h = C.c_void_p()
        check(lib().iamrx_ns_create(C.byref(geom), layout.h, C.byref(self.params), C.byref(self.opts), C.byref(self.h)))
        if getattr(self.params, "turb_forcing", 0):
            self.set_turb_forcing(self.params.turb_nmodes, self.params.turb_mode_start, self.params.turb_div_free)

    def set_turb_forcing(self, nmodes=4, mode_start=0, div_free=1, on=1):
        """switch the turbulent forcing on with upstream's mode table for the level's domain (include/iamrx.h: iamrx_ns_set_turb_forcing)"""
        check(lib().iamrx_ns_set_turb_forcing(self.h, int(on), int(nmodes), int(mode_start), int(div_free)))

    def init_rayleightaylor(self, rho_1, rho_2, tra_1=0.0, tra_2=0.0, pertamp=0.0, interface_width=1.0):
        check(lib().iamrx_ns_init_rayleightaylor(self.h, C.c_double(rho_1), C.c_double(rho_2), C.c_double(tra_1), C.c_double(tra_2),
                                                 C.c_double(pertamp), C.c_double(interface_width)))

    def init_taylorgreen(self, vfac=1.0, a=1.0, b=1.0, c=0.0, rho0=1.0):
        check(lib().iamrx_ns_init_taylorgreen(self.h, C.c_double(vfac), C.c_double(a), C.c_double(b), C.c_double(c), C.c_double(rho0)))

    def init_rest(self, rho0=1.0):
        check(lib().iamrx_ns_init_rest(self.h, C.c_double(rho0)))

    def set_turb_modes(self, kxyz, data, div_free=1):
        """switch the turbulent forcing on with the caller's table of modes: kxyz (M, 3) integer wavevectors, data (M, 17) in
        the order of lib.TURB_FIELDS (include/iamrx.h: iamrx_ns_set_turb_modes)"""
        from .lib import _turb_table
        M, k, d = _turb_table(kxyz, data)
        check(lib().iamrx_ns_set_turb_modes(self.h, M, k, d, int(div_free)))

    def set_particles(self, pc):
        """attach a tracer-particle container (particles.Particles; None: detach).  The container is rebound to this level's boxes; the
        level moves its particles at the end of every advance but the initial one and redistributes them in step().  derive() knows
        "particle_count" and "total_particle_count" while one is attached (include/iamrx.h: iamrx_ns_set_particles)."""
        check(lib().iamrx_ns_set_particles(self.h, None if pc is None else pc.h))
        self._particles = pc

    @property
    def particles(self):
        return getattr(self, "_particles", None)

    # a level is a hierarchy of one: the read-only members amr.Amr offers the run driver, the checkpoint writer and the particle container
    nlev, ratio = 1, 2

    @property
    def levels(self):
        return [self]

    @property
    def layouts(self):
        return [self.layout]

    def level_geom(self, l):
        return self.geom

    def dts(self):
        return [self.dt]

    def set_data(self, which, mf):
        check(lib().iamrx_ns_set_data(self.h, int(which), mf.h))

    def post_init(self, stop_time=-1.0):
        check(lib().iamrx_ns_post_init(self.h, C.c_double(stop_time)))

    def step(self):
        dt = C.c_double()
        check(lib().iamrx_ns_step(self.h, C.byref(dt)))
        return dt.value

    def advance(self, dt):
        est = C.c_double()
        check(lib().iamrx_ns_advance(self.h, C.c_double(dt), C.byref(est)))
        return est.value

    @property
    def time(self):
        t = C.c_double()
        check(lib().iamrx_ns_time(self.h, C.byref(t), None, None))
        return t.value

    @property
    def dt(self):
        t = C.c_double()
        check(lib().iamrx_ns_time(self.h, None, C.byref(t), None))
        return t.value

    def data(self, which):
        h = C.c_void_p()
        check(lib().iamrx_ns_data(self.h, which, C.byref(h)))
        typ, nc, ng = self._types[which]
        if nc == 5:
            nc = self.nalloc if which in (0, 1) else self.nstate
        return MultiFab(self.layout, typ, nc, ng, _handle=h, _owned=True)

    def derive(self, name):
        """derived quantity of the plotfile ("energy", "mag_vort", "avg_pressure": NavierStokes::derive) or one of the velocity-gradient
        fields of pdf.VELGRAD_NAMES as a one-component cell MultiFab; a list of names: derive_fields, one multi-component array;
        "velocity_average" (only with avg_interval > 0; der_vel_avg, NS_derive.cpp:11-45) has the six components VEL_AVG_NAMES"""
        from .lib import MultiFab, CELL
        if not isinstance(name, str):
            return self.derive_fields(name)
        out = MultiFab(self.layout, CELL, 6 if name == "velocity_average" else 1, 0)
        check(lib().iamrx_ns_derive(self.h, name.encode(), out.h, 0))
        return out

    def derive_fields(self, names):
        """one cell MultiFab with component q = field names[q]: any mix of state names (pdf.STATE_NAMES), single-component derived names
        and the velocity-gradient names of pdf.VELGRAD_NAMES, which all share one ghost fill and one kernel launch
        (include/iamrx.h: iamrx_ns_derive_fields).  Collective."""
        from .lib import MultiFab, CELL
        names = list(names)
        out = MultiFab(self.layout, CELL, max(len(names), 1), 0)
        check(lib().iamrx_ns_derive_fields(self.h, len(names), (C.c_char_p * max(len(names), 1))(*[nm.encode() for nm in names]), out.h, 0))
        return out

    def integrate(self, names):
        """volume-weighted sums of named fields over ALL cells of this level (include/iamrx.h: iamrx_ns_integrate; the names of
        histogram) -> float64 array, one per name.  Collective; the same on every rank."""
        import numpy as np
        names = [names] if isinstance(names, str) else list(names)
        out = np.zeros(max(len(names), 1))
        check(lib().iamrx_ns_integrate(self.h, len(names), (C.c_char_p * max(len(names), 1))(*[nm.encode() for nm in names]),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:len(names)]

    def time_average(self, dt_level, level0_steps):
        """NavierStokesBase::time_average (NS_average.cpp:19-69); a hierarchy calls it itself, the driver of a single level after post_init
        and after every step"""
        check(lib().iamrx_ns_time_average(self.h, C.c_double(dt_level), int(level0_steps)))

    @property
    def average_state(self):
        """(time_avg, time_avg_fluct, dt_avg) of the level"""
        v = (C.c_double * 3)()
        check(lib().iamrx_ns_average_state(self.h, 0, v))
        return tuple(v)

    @average_state.setter
    def average_state(self, v):
        check(lib().iamrx_ns_average_state(self.h, 1, (C.c_double * 3)(*[float(x) for x in v])))

    def sum_integrated(self):
        """(mass, tracer, kinetic energy) integrated over ALL cells of this level (NavierStokes::sum_integrated_quantities, one level)"""
        v = (C.c_double * 3)()
        check(lib().iamrx_ns_sum_integrated(self.h, v))
        return tuple(v)

    @property
    def nstate(self):
        """NUM_STATE (NavierStokes.cpp:43-48): u v w density tracer [tracer2] [temp]"""
        return 5 + (1 if self.params.do_trac2 else 0) + (1 if self.params.do_temp else 0)

    @property
    def nalloc(self):
        """components of the S arrays: the state, plus divu and dsdt (Divu_Type, Dsdt_Type) in a temperature run"""
        return self.nstate + (2 if self.params.do_temp else 0)

    def stats(self):
        a, b, c = MgStats(), MgStats(), MgStats()
        check(lib().iamrx_ns_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a, b, c

    def plane_profile(self, dir, bin_level=0):
        """plane-averaged profile of this level along dir (0, 1, 2), nothing masked (include/iamrx.h: iamrx_ns_plane_profile) -> dict
        name -> array of nbins for the 14 names of profile.NAMES, plus "coord" (bin centres in physical units) and "names"; the same
        on every rank.  bin_level: Amr.plane_profile's argument; a level bins in its own cells.  (`profile` is the section timer.)"""
        import numpy as np
        from . import profile as _p
        if bin_level != 0:
            raise ValueError(f"NavierStokes.plane_profile: bin_level {bin_level} on a single level")
        cap = int(self.geom.n[dir]) if 0 <= int(dir) <= 2 else 1
        out, n = np.zeros(len(_p.NAMES) * cap), C.c_int()
        check(lib().iamrx_ns_plane_profile(self.h, int(dir), cap, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return _p.as_dict(out, n.value, self.geom.prob_lo[dir], self.geom.prob_hi[dir], dir, 0)

    def spectrum(self):
        """shell-summed spectra of the new-time state on a fully periodic level (include/iamrx.h: iamrx_ns_spectrum) -> dict with "k"
        (s 2 pi / L_max), "count" (modes per shell), "E" = (P_u + P_v + P_w) / 2, "Euu", "Evv", "Eww", "Ecc" (c: the first tracer), "n",
        "L"; the same bits on every rank.  Collective."""
        from . import spectrum as _s
        return _s.level_spectrum(lib().iamrx_ns_spectrum, self.h, self.geom)

    def cospectrum(self, a, b):
        """co-spectrum of two named fields of this level -- any names derive_fields knows: the state components by plotfile name, "energy",
        "mag_vort", "avg_pressure" and the velocity-gradient names (include/iamrx.h: iamrx_mf_cospectrum) -> dict with "k", "count",
        "C" = C_ab, "Pa", "Pb", "n", "L"; the same bits on every rank.  Collective."""
        from . import budget as _b
        from . import spectrum as _s
        import math
        import numpy as np
        f = self.derive_fields([a, b])
        Cab, Pa, Pb, cnt = _b.mf_cospectrum(self.geom, f, f, 0, 1)
        n, L = _s._geom_nL(self.geom)
        return dict(k=np.arange(len(Cab)) * (2.0 * math.pi / max(L)), count=cnt, C=Cab, Pa=Pa, Pb=Pb, n=n, L=L)

    def plane_spectrum(self, dir):
        """ring-summed 2-D spectra of the new-time state in the planes normal to dir (0, 1, 2), E(k_h; z); only the two directions in the
        plane must be periodic (include/iamrx.h: iamrx_ns_plane_spectrum) -> dict with "k" (s 2 pi / L2), "count" (modes per ring),
        "coord" (plane centres), "dir", "n", "L" and the arrays (nplanes, nrings) "E" = (P_u + P_v + P_w) / 2, "Euu", "Evv", "Eww", "Err"
        (density), "Ecc" (the first tracer); the same bits on every rank.  Collective."""
        from . import planespec as _p
        return _p.level_plane_spectrum(lib().iamrx_ns_plane_spectrum, self.h, self.geom, dir)

    def plane_cospectrum(self, a, b, dir):
        """plane co-spectrum of two named fields of this level, any names cospectrum accepts, in the planes normal to dir (include/iamrx.h:
        iamrx_mf_plane_cospectrum) -> dict with "k", "count", "coord", "dir", "n", "L" and the arrays (nplanes, nrings) "C" = C_ab, "Pa",
        "Pb"; the same bits on every rank.  Collective."""
        from . import planespec as _p
        from . import spectrum as _s
        import math
        import numpy as np
        f = self.derive_fields([a, b])
        Cab, Pa, Pb, cnt = _p.mf_plane_cospectrum(self.geom, f, f, dir, 0, 1)
        n, L = _s._geom_nL(self.geom)
        ia, ib = _p.axes_of(dir)
        return dict(k=np.arange(Cab.shape[1]) * (2.0 * math.pi / max(L[ia], L[ib])), count=cnt, coord=_p.coord_of(self.geom, int(dir), Cab.shape[0]),
                    dir=int(dir), C=Cab, Pa=Pa, Pb=Pb, n=n, L=L)

    def filtered(self, names, kind, kc):
        """the named fields of this level -- any names derive_fields knows -- low-pass filtered in mode space into a new MultiFab on the
        level's layout, component q = names[q] (include/iamrx.h: iamrx_mf_filter; spectral.py).  kind: "sharp", "gaussian", "box" (or
        "identity"); kc: the cut-off in units of 2 pi / L_max.  Needs what spectrum needs.  Collective."""
        from . import spectral as _s
        return _s.level_filtered(self, names, kind, kc)

    def sgs(self, kind, kc, fields=()):
        """a-priori LES analysis of the new-time velocity on a fully periodic level (include/iamrx.h: iamrx_ns_sgs; sgs.py) -> dict with
        the 16 named statistics, "N", "negative_cells", "delta", the derived ratios per model ("strain", "gradient") and "fields": a new
        MultiFab on the level's layout holding the requested fields (names or ids of sgs.FIELD_NAMES), or None.  Collective."""
        from . import sgs as _g
        return _g.level_sgs(lib().iamrx_ns_sgs, self.h, self.geom, self.layout, kind, kc, fields)

    def spectral_budget(self):
        """spectral kinetic-energy budget of the new-time state on a fully periodic level (include/iamrx.h: iamrx_ns_spectral_budget) ->
        dict with "k", "count", "E", "T" (nonlinear transfer, skew-symmetric centred form), "Pi" (the flux -cumsum(T)), "D" (molecular
        dissipation spectrum), "F" (injection by the turbulent forcing; zero when it is off), "n", "L", "visc_coef"; the same bits on every
        rank.  Collective."""
        from . import budget as _b
        return _b.level_budget(lib().iamrx_ns_spectral_budget, self.h, self.geom, self.params.visc_coef)

    def structure_functions(self, pmax=4, rmax=None):
        """structure functions and two-point correlations of u, v, w and the first tracer of the new-time state along the axes, with or
        without walls (include/iamrx.h: iamrx_ns_strfn) -> the dict of strfn.derive: the raw "avg" (3, 4, ncol, rcap), "count", "mean",
        "r", "dx", "n", "L", "periodic", and per axis "SL", "ST", "Sc" (and "...abs"), "RL", "RT", "f", "g", "integral_scale",
        "taylor_scale".  rmax: None the largest separation of every axis, one integer or three (0 skips an axis).  The same bits on every
        rank.  Collective."""
        from . import strfn as _s
        return _s.level_structure(lib().iamrx_ns_strfn, self.h, self.geom, pmax, rmax)

    def histogram(self, names, nbins=64, range=None):
        """histograms and PDFs of named fields of this level (include/iamrx.h: iamrx_ns_histogram; pdf.py: the names, the binning rule)
        -> dict with "names", "range", "edges", "counts" (int64), "below", "above", "nan", "total", "pdf", one row per name.  range: one
        (lo, hi) pair per name, or None for each field's minimum and maximum.  Collective; the same on every rank."""
        from . import pdf as _p
        return _p.histogram(self, lib().iamrx_ns_histogram, names, nbins, range)

    def histogram2(self, namex, namey, nbins=(32, 32), range=None):
        """joint histogram of two named fields (include/iamrx.h: iamrx_ns_histogram2) -> dict with "xedges", "yedges", "counts"
        (nbx, nby) int64, "outside", "total", "pdf".  Collective."""
        from . import pdf as _p
        return _p.histogram2(self, lib().iamrx_ns_histogram2, namex, namey, nbins, range)

    def profile(self, enable):
        arr = (C.c_double * 8)()
        check(lib().iamrx_ns_profile(self.h, int(enable), arr))
        return list(arr)

    def __del__(self):
        try:
            if self.h:
                lib().iamrx_ns_destroy(self.h)
        except Exception:
            pass
