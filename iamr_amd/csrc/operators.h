// iamr_amd/csrc/operators.h -- host-side operator layer keeping IAMR's operator API surface
// (MacProj / Projection / Diffusion / NavierStokesBase::advance), SURVEY 8(b).
#pragma once
#include <string>
#include "mf.h"
#include "mlmg.h"
#include "kernels.h"
#include <memory>
#include <functional>

namespace iamrx {

// ---- MacProj (reference Source/MacProj.H:36-94) ------------------------------------------------------
// MacProj::mlmg_mac_solve (Source/MacProj.cpp:1084-1184)
MGStats mlmg_mac_solve(const Geometry& g, MultiFab* const umac[3], const MultiFab& rho, int rho_comp, const MultiFab* S,
                       MultiFab& mac_phi, double rhs_scale, const DomainBC& bc, double mac_tol, double mac_abs_tol,
                       const MGOpts& opts, MultiFab* const fluxes[3], const MultiFab* cphi = nullptr, const Geometry* cgeom = nullptr, int ratio = 2);

// ---- Projection (reference Source/Projection.H:53-134, 244-254) --------------------------------------
// Projection::doMLMGNodalProjection (Source/Projection.cpp:2385-2567), single level:
// rhs = div(vel) at nodes, solve div(sig grad phi) = rhs, vel -= sig grad phi, Gp = / += grad phi.
MGStats nodal_projection(const Geometry& g, MultiFab& vel, int vcomp, MultiFab& phi, const MultiFab& sig, int sig_comp,
                         const DomainBC& bc, double rel_tol, double abs_tol, const MGOpts& opts, MultiFab* gp, bool increment_gp,
                         const MultiFab* rhcc = nullptr /* cell-centred source prepared by make_rhcc: div(sig grad phi) = div(vel) + <rhcc> */,
                         double vel_scale = 1.0 /* the valid cells of the projected velocity are stored times this factor (nodal_mknewu) */);
void nodal_rhcc_add(const Geometry& g, MultiFab& rhs, const MultiFab& rc, const DomainBC& bc);
MultiFab make_rhcc(const Geometry& g, const MultiFab& src, int comp, double scale, const MultiFab* drop);
void mask_mult(MultiFab& y, int ycomp, int nc, const MultiFab& m, bool keep_where_zero, int ng);   // y *= (m == 0) or (m != 0), amrns.hip

// Projection::level_project on one level that covers the domain (Source/Projection.cpp:166-450; declaration Projection.H:53-75):
// P_new = 0; U_new /= dt; U_new += Gp_old/rho_half; sigma = 1/rho_half; nodal projection (Gp_new = grad phi, P_new = phi); U_new *= dt.
// U_new: state with the velocity at comps vcomp..vcomp+2, 1 ghost; rho_half: 1 ghost.
MGStats level_project_single(const Geometry& g, double dt, MultiFab& U_new, int vcomp, MultiFab& P_new, const MultiFab& Gp_old, MultiFab& Gp_new,
                             const MultiFab& rho_half, const DomainBC& bc, double proj_tol, double proj_abs_tol, const MGOpts& opts);

// ---- Diffusion (reference Source/Diffusion.H:53-225) -------------------------------------------------
// explicit viscous terms div tau(U): Diffusion::getTensorViscTerms (Source/Diffusion.cpp:1655-1777): out = -b * L_tensor(U), a = 0
// coarse/fine faces of a refined level (tensorop.setCoarseFineBC): crse = the coarse level's velocity (3 comps, valid data on its own
// layout) or null for homogeneous data
struct TensorCF { const MultiFab* crse; const Geometry* cgeom; int ratio; };
// Diffusion::computeExtensiveFluxes after the apply / solve: flux[d] (3 comps, face d) = or += fac * area * operator flux
struct TensorFlux { MultiFab* flux[3]; double fac; bool add; };
void tensor_apply(const Geometry& g, MultiFab& out, MultiFab& vel /*3 comps, 1 ghost; BC data in ghosts*/, double a_scalar, double b_scalar,
                  const MultiFab* acoef, const MultiFab* const eta[3], const DomainBC* bcs, int nbc /*1 or 3 (per component)*/,
                  const TensorCF* cf = nullptr, const TensorFlux* fx = nullptr);
inline void tensor_apply(const Geometry& g, MultiFab& out, MultiFab& vel, double a_scalar, double b_scalar, const MultiFab* acoef,
                         const MultiFab* const eta[3], const DomainBC& bc) { tensor_apply(g, out, vel, a_scalar, b_scalar, acoef, eta, &bc, 1); }
// Crank-Nicolson implicit solve (a*acoef - b div tau) u = rhs: Diffusion::diffuse_tensor_velocity (Source/Diffusion.cpp:837-929)
MGStats tensor_solve(const Geometry& g, MultiFab& soln, const MultiFab& rhs, double a_scalar, double b_scalar, const MultiFab* acoef,
                     const MultiFab* const eta[3], const DomainBC* bcs, int nbc, double tol_rel, double tol_abs, const MGOpts& opts,
                     const TensorCF* cf = nullptr, const TensorFlux* fx = nullptr);
inline MGStats tensor_solve(const Geometry& g, MultiFab& soln, const MultiFab& rhs, double a_scalar, double b_scalar, const MultiFab* acoef,
                            const MultiFab* const eta[3], const DomainBC& bc, double tol_rel, double tol_abs, const MGOpts& opts)
{ return tensor_solve(g, soln, rhs, a_scalar, b_scalar, acoef, eta, &bc, 1, tol_rel, tol_abs, opts); }

// NavierStokesBase::calc_mut_LES (Source/NS_LES.cpp:22-225) on caller-owned data: the ghost cells of vel (3 comps, 1 ghost, the level's
// boundary data in them as for tensor_apply) are filled by the tensor operator's own boundary step (CellMG::fillBoundaryData: setDomainBC
// with LES_setDomainBC's per-component codes :59-68, 230-285, setCoarseFineBC :76-84, setLevelBC :88), then mu[d] = base + mu_t (les_mut,
// k_les.hip).  bcs[n].maxorder: NS_LES.cpp sets none, MLLinOp's default applies (3 as far as is known: DESIGN.md section 2).
void calc_mut_les(const Geometry& g, MultiFab& vel, const DomainBC bcs[3], int model, double Cs, double base, MultiFab* const mu[3],
                  const TensorCF* cf = nullptr);

// ---- Diffusion operator entries on caller-owned data (diffusion.hip; reference Source/Diffusion.H:53-225) -------------------
// the coarse level's state at the old / new time (valid cells on its own layout; the same component numbering as the fine arrays);
// crse_new == nullptr: homogeneous coarse/fine data (the sync solves)
struct DiffusionCrse { const MultiFab* crse_old; const MultiFab* crse_new; const Geometry* cgeom; int ratio; };
// Diffusion::diffuse_scalar (Source/Diffusion.cpp:207-599): Crank-Nicolson update of component sigma of S_new,
//   (alpha - theta dt div beta grad) s_new = alpha s* + (1 - theta) dt div beta grad s_old + dt delta_rhs,
// rho_flag 0: s = S, alpha = 1; 1: alpha = rho_half; 2: s = S / rho, alpha = rho_new, S_new = s rho_new.  S_old / S_new: at least 1 ghost
// cell, FILLED by the caller (FillPatch: boundary values of the level, Diffusion.cpp:237-239).  fluxn / fluxnp1 (may be null): the
// extensive fluxes (1 - theta) area (-beta grad s_old) and theta area (-beta grad s_new).  add_old_time_divFlux = false: the sync form
// (S_old unused).  Rho_old / Rho_new (null: S_old / S_new): the arrays holding the density in rho_comp.  bc: Diffusion::setDomainBC of the component.
MGStats diffuse_scalar(const Geometry& g, const MultiFab* S_old, const MultiFab* Rho_old, MultiFab& S_new, const MultiFab* Rho_new, int sigma, int rho_comp, double dt, double theta,
                       const MultiFab& rho_half, int rho_flag, MultiFab* const fluxn[3], MultiFab* const fluxnp1[3],
                       const MultiFab* delta_rhs, int rhs_comp, const MultiFab* const betan[3], const MultiFab* const betanp1[3],
                       const DomainBC& bc, const DiffusionCrse* crse, bool add_old_time_divFlux, double visc_tol, const MGOpts& o);
// Diffusion::diffuse_tensor_velocity (Source/Diffusion.cpp:617-957): (alpha - theta dt div tau) u_new = alpha u* + (1 - theta) dt div tau(u_old),
// alpha = rho_half (rho_flag 1) or rho_new with u* weighted by rho_old (rho_flag 3, do_mom_diff).  U_old / U_new: states with the velocity
// in components 0..2 and the density in rho_comp, 1 filled ghost cell.  visc_old_term (may be null): div tau(u_old) if the caller has it
// already and wants no fluxes.  tflux (may be null): the summed extensive viscous fluxes.  fill_new: refills the ghost cells of U_new's
// velocity once it holds rho u* (the FillPatch of Diffusion.cpp:866); null: they are used as they came.  ready (may be null; needs
// visc_old_term and no fluxes): the caller's pass that formed u* has already written rho u* into U_new and the right-hand side into
// ready->rhs and taken its three max norms -- the first pass over the level is skipped.
struct TensorRhsReady { MultiFab* rhs; double norm[3]; };
MGStats diffuse_tensor_velocity(const Geometry& g, const MultiFab* U_old, MultiFab& U_new, int rho_comp, double dt, double theta,
                                const MultiFab& rho_half, int rho_flag, const MultiFab* visc_old_term, const MultiFab* const eta_n[3],
                                const MultiFab* const eta_np1[3], const DomainBC bc_visc[3], const DiffusionCrse* crse,
                                MultiFab* const tflux[3], double visc_tol, const MGOpts& o, const std::function<void(MultiFab&)>& fill_new,
                                const TensorRhsReady* ready = nullptr);

// Diffusion::diffuse_tensor_Vsync (Source/Diffusion.cpp:1010-1178) and Diffusion::diffuse_Ssync as NavierStokes::mac_sync uses them; see diffusion.hip
MGStats diffuse_tensor_Vsync(const Geometry& g, MultiFab& Vsync, double dt, double theta, const MultiFab& rho_half, int rho_flag,
                             const MultiFab* Rho_old, const MultiFab* Rho_new, int rho_comp, const MultiFab* const eta[3],
                             const DomainBC bc_visc[3], const BCRec bc_vel[3], const Geometry* cgeom, int ratio, MultiFab* const tflux[3],
                             double visc_tol, const MGOpts& o);
MGStats diffuse_Ssync(const Geometry& g, MultiFab& Ssync, int sn, double dt, double theta, const MultiFab& rho_half, int rho_flag,
                      const MultiFab& Rho_new, int rho_comp, const MultiFab* const beta[3], const DomainBC& bc, const Geometry* cgeom, int ratio,
                      MultiFab* const flux[3], double visc_tol, const MGOpts& o);

// ---- inter-level data motion (amr.hip) ------------------------------------------------------------------------
// amrex::MultiFab::ParallelCopy between different layouts of one index space; periodic_geom != nullptr adds the periodic images
// add = true: dst += src (MultiFab::ParallelAdd); the source regions must then map to disjoint destination cells
class FluxRegister;
// MacProj::mac_sync_solve (Source/MacProj.cpp:359-470)
MGStats mac_sync_solve(const Geometry& g, FluxRegister& mr, const MultiFab& rho_half, double dt, LayoutP fine_layout, int ratio,
                       MultiFab* const Ucorr[3], MultiFab& mac_sync_phi, const DomainBC& bc, double tol, double abs_tol, const MGOpts& opts,
                       const Geometry* cgeom = nullptr, int cratio = 2);

// ---- regrid.hip: error estimation + grid generation
void derive_mag_vort(const Geometry& g, MultiFab& out, int ocomp, const MultiFab& vel, int vcomp);
// the derived fields of the velocity-gradient tensor (k_velgrad.hip; declared in kernels.h): out(ocomp + q) = quantity which[q]
void derive_velgrad(const Geometry& g, MultiFab& out, int ocomp, int nq, const int* which, const MultiFab& vel, int vcomp, double mu, int path);
void error_tag(const Geometry& g, MultiFab& tags, const MultiFab& field, int comp, int mode, double value, int level,
               const double* rb_lo, const double* rb_hi);
// manual_tags_placement at the outflow faces (NavierStokesBase.cpp:2112-2215): mode 1 do_refine_outflow, 2 do_derefine_outflow with
// ncoarse layers (of blocking-factor-coarsened cells) left unrefined
struct OutflowTags { int nface = 0; int dir[6], side[6]; int mode = 0; int ncoarse = 0; };
// periodic-aware erosion of a 0/1 cell map by `passes` cells inside the bounding box [lo, hi] of its set cells (amrregrid.hip: the proper
// nesting domain of a regrid above level 0)
void erode_map(std::vector<unsigned char>& m, const int n[3], const int per[3], int passes, const int lo[3], const int hi[3]);
std::vector<BoxD> cluster_tags(const unsigned char* tags_host, const BoxD& domain, int blocking_factor, int max_grid_size, double grid_eff,
                               int n_error_buf, const OutflowTags* oft = nullptr, const unsigned char* allowed = nullptr /* domain-sized 0/1: where the new level may lie */);

void parallel_copy(MultiFab& dst, const MultiFab& src, int scomp, int dcomp, int nc, int src_ng, int dst_ng, const Geometry* periodic_geom, bool add = false);
// same cells, different boxes (merged working layout <-> the caller's boxes): ghost cells included, valid data last
void relayout_copy(MultiFab& dst, const MultiFab& src, int nc, int scomp = 0, int dcomp = 0);
// the merged layout of a caller's chopped layout if it covers the domain and merging reduces the box count; else null (mf.h: coalesce_layout)
LayoutP merged_solve_layout(const Geometry& g, const LayoutP& l);
// amrex::average_down (cells), average_down_faces, average_down_nodal: NavierStokesBase::avgDown_StatePress, Source/NavierStokesBase.cpp:4125-4193
void average_down(const MultiFab& fine, MultiFab& crse, int scomp, int ncomp, int ratio);
// StateData of one level: old/new MultiFabs and their times (old_ may be null: only one time level)
struct TimeData { const MultiFab* old_; const MultiFab* new_; double t_old, t_new; };
// AmrLevel::FillPatch on a refined level (FillPatchTwoLevels + CellConservativeLinear + physical BC), see amr.hip
// StateData time interpolation (old or new if `time` is within 1e-3 (t_new - t_old) of it); returns the MultiFab to read and its first component
const MultiFab* state_time_interp(const TimeData& td, double time, int scomp, int ncomp, MultiFab& tmp, int& comp0);
void fillpatch_two_levels(MultiFab& dst, int dcomp, double time, const TimeData& fine, const TimeData& crse, int scomp, int ncomp,
                          const Geometry& cgeom, const Geometry& fgeom, int ratio, const BCRec* bc, const double* extdir_lo, const double* extdir_hi);

// NavierStokesBase::create_umac_grown on a refined level: FaceLinear coarse-fine fill of the ghost faces + IAMR's divergence fix
// (Source/NavierStokesBase.cpp:1108-1311); umac_fine need 1 ghost layer, divu (fine cells, >= 1 ghost) may be null
void create_umac_grown(MultiFab* const umac_fine[3], const MultiFab* const umac_crse[3], const MultiFab* divu,
                       const Geometry& cgeom, const Geometry& fgeom, int ratio);
// amrex::FluxRegister / YAFluxRegister role (see amr.hip)
class FluxRegister {
public:
    FluxRegister(LayoutP fine, LayoutP crse, const Geometry& cgeom, int ratio, int ncomp);
    void setVal(double v);
    void CrseInit(const MultiFab& flux /*coarse level, face type dir*/, int dir, int scomp, int dcomp, int nc, double mult, bool add);
    void FineAdd(const MultiFab& flux /*fine level, face type dir*/, int dir, int scomp, int dcomp, int nc, double mult);
    void Reflux(MultiFab& S /*coarse level, cells*/, double volume, double scale, int scomp, int dcomp, int nc);
    const MultiFab& reg(int dir, int side) const { return m_reg[dir][side]; }
private:
    LayoutP m_fine, m_crse;
    Geometry m_cgeom;
    int m_ratio, m_ncomp;
    LayoutP m_slab[3][2];
    MultiFab m_reg[3][2];
};

// ---- multi-level pieces (amrns.hip) -----------------------------------------------------------------------------
// trilinear interpolation (amrex::NodeBilinear) of a coarse nodal MultiFab at the valid nodes of `fine`: fine = (add: +=) interp(crse);
// mask (nodal, fine layout; may be null): only where mask != 0
void node_interp_from_crse(MultiFab& fine, const MultiFab& crse, const Geometry& cgeom, int ratio, const MultiFab* mask, bool add);
// NavierStokesBase::SyncInterp with cell_cons_interp (Source/NavierStokesBase.cpp:3071-3276): conservative-linear interpolation of
// the coarse cell data crse(scomp..) (valid region; periodic images and homogeneous-ext_dir / extrapolated values outside walls are
// built here) to every valid cell of dst(dcomp..)
void sync_interp_cellcons(MultiFab& dst, int dcomp, const MultiFab& crse, int scomp, int ncomp, const Geometry& cgeom, const Geometry& fgeom,
                          int ratio, const BCRec* bc);
// NavierStokesBase::ComputeAofs with is_sync = true (Source/NavierStokesBase.cpp:4594-4845 as called from MacProj::mac_sync_compute):
// edge states traced with umac, fluxes formed with ucorr, conservative update for every component, sync(acomp..) -= update
void godunov_compute_aofs_sync(const Geometry& g, MultiFab& sync, int acomp, const MultiFab& S, int ncomp, const MultiFab* force,
                               const MultiFab* divu, MultiFab* const umac[3], MultiFab* const ucorr[3], const int* iconserv, double dt,
                               const BCRec* bc, bool is_velocity, bool use_forces_in_trans, MultiFab* const flux_out[3], int scheme = 0);

// MacProj::mac_sync_compute on caller-owned arrays (amrns.hip): the form of NavierStokes::mac_sync (Source/MacProj.cpp:488-731) and the form
// with known edge states (:733-786)
void mac_sync_compute(const Geometry& g, MultiFab* const ucorr[3], MultiFab& Vsync, MultiFab& Ssync, const MultiFab& Svel, const MultiFab& Sscal, int nscal,
                      const MultiFab* visc_vel, const MultiFab* tf_scal, const MultiFab& gradp, const MultiFab* divu, MultiFab* const umac[3],
                      const int* iconserv_scal, bool do_mom_diff, double gravity, double dt, const BCRec* bc_vel, const BCRec* bc_scal,
                      bool use_forces_in_trans, int scheme, MultiFab* const flux_vel[3], MultiFab* const flux_scal[3], const MultiFab* turb_f = nullptr);
void mac_sync_compute_edge(const Geometry& g, MultiFab* const ucorr[3], MultiFab& Sync, int sync_indx, MultiFab* const edgestate[3], int edge_comp,
                           MultiFab* const flux_out[3]);

// SyncRegister (Source/SyncRegister.cpp): nodal values on the faces of the coarsened fine boxes, kept as ONE single-valued nodal
// MultiFab on the coarse level's layout + the node masks that InitRHS needs
class SyncRegister {
public:
    SyncRegister(LayoutP fine, LayoutP crse, const Geometry& cgeom, const Geometry& fgeom, int ratio, const int phys_lo[3], const int phys_hi[3]);
    void CrseInit(const MultiFab& sync_resid_crse, double mult);          // SyncRegister.cpp:306-318
    void FineAdd(const MultiFab& sync_resid_fine, double mult);           // :350-607
    // :302-348; finer: the boxes of the level above the residual's (ratio finer_ratio to it), fgeom: the residual's level.  Modifies the residual.
    void CompAdd(MultiFab& sync_resid_fine, const Geometry& fgeom, const LayoutP& finer, int finer_ratio, double mult);
    void InitRHS(MultiFab& rhs);                                          // :47-304
    const MultiFab& reg() const { return m_reg; }
    const MultiFab& vs_fine() const { return m_vsfine; }                  // node class of the coarse nodes w.r.t. the fine level: 0 untouched, 1 inside, 2 on its boundary
private:
    LayoutP m_fine, m_crse;
    Geometry m_cgeom, m_fgeom;
    int m_ratio;
    int m_plo[3], m_phi[3];
    MultiFab m_reg, m_onreg, m_vsfine;
};

// *nbins = spectrum_nbins(g) first, then the capacity check, then spectrum_compute (kernels.h)
void spectrum_of(const Geometry& g, const MultiFab& S, int nq, const int* comps, int cap, double* out, long* count, int* nbins);
// the same order of checks in front of cospectrum_compute: out[v * nbins + s], v = 0, 1, 2: C_ab, P_a, P_b
void cospectrum_of(const Geometry& g, const MultiFab& A, int acomp, const MultiFab& B, int bcomp, int cap, double* out, long* count, int* nbins);
// ... and in front of spectrum_k2_compute
void spectrum_k2_of(const Geometry& g, const MultiFab& S, int nq, const int* comps, int cap, double* out, int* nbins);
// the common part of the plane-spectrum entries: plane_spectrum_check, *nplanes and *nrings, the capacities, plane_spectrum_compute
void plane_spectrum_of(const Geometry& g, int n, const SpecPair* f, int dir, int pcap, int rcap, double* out, long* count, int* nplanes, int* nrings);
// the common part of the three structure-function entries: pmax, the separations (strfn_resolve_rmax) and the capacity are checked by
// name, count[d * rcap + r] (or null) is filled from strfn_count, then strfn_compute (kernels.h)
void strfn_of(const Geometry& g, const MultiFab& S, int nq, const int* comps, int pmax, const int rmax[3], int rcap, double* out, long long* count,
              double* mean);

class NavierStokes;
// sync residual of a level projection (Hydro::NodalProjector::computeSyncResidualCoarse / Fine): crse_side: on the nodes of the level
// that touch both cells covered by the next finer level and cells that are not, rhs - L(phi) formed with the uncovered cells only;
// fine side: on the nodes of the level's own boundary inside the domain, formed with the level's cells only.  Zero elsewhere.
// ---- multi-level nodal projection on caller-owned data (amrns.hip) ----------------------------------------------------------------
// one level of a composite projection: its geometry, boxes, the nodal LinOp BC (Projection.cpp:2432-2464) and the ratio to the next
// coarser level of the solve; gp: the Gradp array that receives (or accumulates) grad phi (may be null); set_inflow: fills the ghost
// velocities outside inflow faces (Projection::set_boundary_velocity), fill_gp: FillPatch of Gradp afterwards (both may be empty)
struct ProjLevel {
    Geometry g; LayoutP layout; DomainBC nodal_bc; int ratio = 2;
    MultiFab* gp = nullptr;
    std::function<void(MultiFab&, double)> set_inflow;
    std::function<void()> fill_gp;
};
// Hydro::NodalProjector::project on the levels PL[0 .. nl-1] (Projection::doMLMGNodalProjection with nlevel > 1, Projection.cpp:2385-2567):
// div(sig grad phi) = div(vel) + rhnd + <rhcc> on the composite grid; vel -= sig grad phi; gp = / += grad phi
MGStats composite_project(const std::vector<ProjLevel>& PL, MultiFab* const vel[], const int vcomp[], MultiFab* const phi[], const MultiFab* const sig[],
                          const MultiFab* rhnd, double rtol, double atol, bool increment_gp, double inflow_scale, const MGOpts& o,
                          const MultiFab* const rhcc[] = nullptr);
// Projection::initialVelocityProject / initialSyncProject (Source/Projection.cpp:615-838, 970-1185) on caller-owned arrays of the levels
// PL[0 .. nl-1] (amrns.hip; the hierarchy's post_init calls the same functions)
MGStats initial_velocity_project(const std::vector<ProjLevel>& PL, MultiFab* const vel[], const int vcomp[], MultiFab* const pres[], const MultiFab* const rho[],
                                 const int rho_comp[], const MultiFab* const divu[], const int divu_comp[], double proj_tol, double proj_abs_tol, const MGOpts& o);
MGStats initial_sync_project(const std::vector<ProjLevel>& PL, MultiFab* const vel_new[], const int vcomp[], const MultiFab* const vel_old[], MultiFab* const phi[],
                             MultiFab* const pres_new[], const MultiFab* const rho_half[], const MultiFab* const divu_new[], const MultiFab* const divu_old[],
                             const int divu_comp[], double dt, double proj_tol, double proj_abs_tol, const MGOpts& o);
// compSyncResidualCoarse (fine_layout given: the level's nodes that touch both cells covered by fine_layout and cells that are not, formed
// with the uncovered cells) / compSyncResidualFine (fine_layout null: the nodes of the level's own boundary inside the domain)
MultiFab sync_resid(const Geometry& g, const LayoutP& layout, const DomainBC& bcn, const LayoutP& fine_layout, int fine_ratio, const MultiFab& vold,
                    const MultiFab& phi, const MultiFab& sig, const MultiFab* rhcc = nullptr);
// Projection::MLsyncProject (Source/Projection.cpp:457-607) on caller-owned data: the two-level sync projection of the velocity increments
// Vsync (coarse level, 3 comps, 1 ghost) and V_corr (fine level: the interpolated Vsync), with sigma = 1 / rho_crse, 1 / rho_fine and the
// sync register's right-hand side; phi_crse / phi_fine (1 ghost, zeroed here) return the pressure correction, which is also added to
// pres_crse / pres_fine; vel_* += dt * the projected increments; PL[l].gp += grad phi.  crse_sync_reg (level PL[0] is itself refined and
// crse_iteration == crse_dt_ratio): receives the residual of the composite solution on PL[0]'s boundary (SyncRegister::CompAdd).
MGStats ml_sync_project(const ProjLevel PL[2], MultiFab& pres_crse, MultiFab& vel_crse, int vcomp_c, MultiFab& pres_fine, MultiFab& vel_fine, int vcomp_f,
                        const MultiFab& rho_crse, const MultiFab& rho_fine, MultiFab& Vsync, MultiFab& V_corr, MultiFab& phi_crse, MultiFab& phi_fine,
                        SyncRegister& rhs_sync_reg, SyncRegister* crse_sync_reg, double dt, int crse_iteration, int crse_dt_ratio,
                        double sync_tol, double abs_tol, const MGOpts& o);
MultiFab amr_sync_resid(NavierStokes& ns, const MultiFab& vold, const MultiFab& phi, const MultiFab& sig, bool crse_side, const MultiFab* rhcc = nullptr /* valid cells */);

// ---- NavierStokes level (reference Source/NavierStokes.cpp:543-691 advance, :1254-1432 post_init) -----
struct NSParams {
    double cfl = 0.8, visc_coef = 0.0, be_cn_theta = 0.5, gravity = 0.0;
    double mac_tol = 1.e-12, mac_abs_tol = 1.e-16, proj_tol = 1.e-12, proj_abs_tol = 1.e-16, visc_tol = 1.e-10;
    int use_forces_in_trans = 0, do_mom_diff = 0, init_iter = 2, init_vel_iter = 1;
    double init_shrink = 1.0, change_max = 1.1, fixed_dt = -1.0;
    int nscal = 2, verbose = 0;
    double init_dt = -1.0;               // ns.init_dt
    double tracer_diff_coef = 0.0;       // ns.scal_diff_coefs[0]
    int phys_lo[3] = {0, 0, 0}, phys_hi[3] = {0, 0, 0};   // ns.lo_bc / ns.hi_bc (PhysBCType: 0 Interior, 4 SlipWall, 5 NoSlipWall)
    double wall_vel_lo[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, wall_vel_hi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // xlo.velocity ...: [d*3+n]
    double scal_bc_lo[12] = {0}, scal_bc_hi[12] = {0};   // xlo.density, xlo.tracer, xlo.tracer2, xlo.temp (inflow values): [d*4+n], n = the scalar's slot
    int do_cons_trac = 0;                // ns.do_cons_trac
    int do_denminmax = 0, do_scalminmax = 0;   // ns.do_denminmax / ns.do_scalminmax (NavierStokesBase.cpp:466-467)
    int do_trac2 = 0, do_cons_trac2 = 0; // ns.do_trac2 / ns.do_cons_trac2: a second tracer (NavierStokes.cpp:45-46, NS_setup.cpp:312-320)
    double tracer2_diff_coef = 0.0;      // ns.scal_diff_coefs[1]
    int do_temp = 0;                     // ns.do_temp: temperature, the last state component (NavierStokes.cpp:47-48)
    double temp_cond_coef = 0.0;         // ns.temp_cond_coef
    int use_ppm = 0;                     // ns.advection_scheme: 0 Godunov_PLM, 1 Godunov_PPM (NavierStokesBase.cpp:548-553)
    // ns.avg_interval / ns.compute_fluctuations (NS_average.cpp, NavierStokesBase.cpp:487-488): time averages of the velocity, sampled
    // every avg_interval level-0 steps (0: off); ns.sum_interval (NavierStokesBase.cpp:452, 2589-2592): integrated quantities (<= 0: off)
    int avg_interval = 0, compute_fluctuations = 0, sum_interval = 0;
    // ns.do_LES / ns.LES_model (0 Smagorinsky, 1 Sigma) / ns.smago_Cs_cst / ns.sigma_Cs_cst (NavierStokesBase.cpp:142-146, 481-485)
    int do_LES = 0, LES_model = 0;
    double smago_Cs_cst = 0.18, sigma_Cs_cst = 1.5;
};

enum StateComp { Xvel = 0, Yvel = 1, Zvel = 2, Density = 3, Tracer = 4, MAXSCAL = 4, MAXSTATE = 3 + MAXSCAL, MAXSLOT = MAXSCAL + 2 };   // Tracer2 / Temp: NavierStokes::Tracer2 / Temp (-1: absent)

struct ScalForm { int form[MAXSCAL]; };   // captured by device lambdas
void scale_by(MultiFab& y, const MultiFab& x, int xcomp, int ng, bool divide);   // y (comp 0) *= or /= x(xcomp) on ng ghost cells
class SyncRegister;
class AmrNS;
class Particles;
struct FieldEntry;                                            // an entry of the field table (diagnostics.hip)
struct FieldRef { const MultiFab* mf; int comp; };            // where a single-component field is
class NavierStokes {
public:
    // the boxes as the caller (or the grid generator) gave them; `layout` below is coalesce_layout(user_layout): what the level works on
    LayoutP user_layout;
    // turb: the mode table of the turbulent forcing a hierarchy hands to the levels a regrid creates (null: no forcing until set_turb_modes)
    NavierStokes(const Geometry& g, LayoutP layout, const NSParams& p, const MGOpts& o, TurbTableP turb = nullptr);
    ~NavierStokes();
    void init_taylorgreen(double vfac, double a, double b, double c, double rho0);   // Source/prob/prob_init.cpp:509-560
    // probtype 10 (Source/prob/prob_init.cpp:407-488, 3-D branch): fluid at rest, tanh density / tracer interface at mid height,
    // perturbed by the hard-coded random amplitude and phases of the reference
    void init_rayleightaylor(double rho_1, double rho_2, double tra_1, double tra_2, double pertamp, double interface_width);
    void init_rest(double rho0);               // probtype 1 (LidDrivenCavity), Source/prob/prob_init.cpp:102-109
    void post_init(double stop_time);          // NavierStokes::post_init
    double step();                             // Amr::coarseTimeStep on one level: computeNewDt + advance
    double advance(double dt) { return advance(dt, 1, 1); }
    double advance(double dt, int iteration, int ncycle);   // NavierStokes::advance(time, dt, iteration, ncycle); returns the dt estimate
    double estTimeStep();                      // NavierStokesBase::estTimeStep
    // ---- diagnostics of named fields (diagnostics.hip: the field table says which names there are and which entry point takes which)
    // derived quantities of the plotfile (derive_lst of NS_setup.cpp:436-449): "energy" = rho |u|^2 / 2 (derkeng), "mag_vort" = |curl u|
    // (dermgvort, ghost cells by FillPatch), "avg_pressure" = mean of the 8 nodes of the cell (deravgpres); new-time data; out: cell, >= 1 comp;
    // with avg_interval > 0 also "velocity_average" (der_vel_avg, NS_derive.cpp:11-45): 6 components, mean velocity and rms fluctuation;
    // with particles bound the two particle counts; and the ten velocity-gradient names (k_velgrad.hip; "dissipation" with
    // mu = ns.vel_visc_coef: the molecular part only, also in an LES run)
    void derive(const std::string& name, MultiFab& out, int ocomp = 0);
    // out(ocomp + q) = field names[q]: any mix of state names by their plotfile names (x_velocity, y_velocity, z_velocity, density, tracer,
    // and tracer2 / temp when the run has them), the single-component derived names and the velocity-gradient names; ALL
    // velocity-gradient names of the list share ONE fillpatch of the velocity and ONE derive_velgrad launch
    void derive_fields(int n, const std::string* names, MultiFab& out, int ocomp = 0);
    // out[q] = volume-weighted sum of field names[q] (a state name, energy, mag_vort, avg_pressure or a velocity-gradient name) over all
    // cells of the level, summed over the ranks: sum_integrated for named fields
    void integrate(int n, const std::string* names, double* out) { integrate_of({this}, n, names, out); }
    MultiFab& get_new_data(int type) { return type == 0 ? S[inew] : (type == 1 ? P[pnew] : Gp[pnew]); }
    MultiFab& get_old_data(int type) { return type == 0 ? S[1 - inew] : (type == 1 ? P[1 - pnew] : Gp[1 - pnew]); }
    MultiFab& umac(int d) { return u_mac[d]; }
    MultiFab& Aofs() { return aofs; }
    // ---- on-the-fly velocity statistics (Average_Type, NS_setup.cpp:389-405; defined only with avg_interval > 0): components 0..2 the
    // time integral of u, v, w, 3..5 the time integral of the squared fluctuation; no ghost cells, on the level's working layout like the
    // state, zero at initialisation.  The reference keeps an old and a new copy of this state type and writes both identically in
    // time_average (NS_average.cpp:45-55); nothing ever reads them at different times, so ONE array is kept here.
    // time_avg / time_avg_fluct / dt_avg: NavierStokesBase::time_avg[level] etc. (NavierStokesBase.cpp:2467-2522)
    bool has_average() const { return p.avg_interval > 0; }
    MultiFab& average_data() { if (!has_average()) throw Error("iamrx NavierStokes: no time averages (ns.avg_interval = 0)"); return Savg; }
    double time_avg = 0.0, time_avg_fluct = 0.0, dt_avg = 0.0;
    // NavierStokesBase::time_average (NS_average.cpp:19-69): dt_avg += dt_level; every avg_interval-th level-0 step the accumulation
    // kernel (k_stats.hip), then the three scalars.  Nothing happens (no launch) with avg_interval = 0.
    void time_average(double dt_level, int level0_steps);
    // NavierStokes::sum_integrated_quantities (NavierStokes.cpp:1046-1079) of this level alone: volume-weighted sums of density, tracer and
    // kinetic energy over all its cells, summed over the ranks
    void sum_integrated(double out[3]) { sum_integrated_of({this}, out); }
    // plane-averaged profile of this level alone along dir (k_profile.hip; nothing masked): out[q * nbins + b], PROFILE_NQ quantities of the
    // new-time state, nbins = cells of the domain along dir.  Collective; every rank receives the result.  Returns nbins.
    int plane_profile(int dir, double* out, int cap) { return plane_profile_of({this}, dir, 0, out, cap); }
    // shell-summed power spectra of u, v, w and the first tracer of the new-time state (k_spectrum.hip): out[q * nbins + s], SPECTRUM_NQ
    // columns, count[s] (or null) the modes of shell s.  *nbins is set before the capacity is checked.  Collective; every rank receives the
    // result.
    void spectrum(int cap, double* out, long* count, int* nbins);
    // ring-summed plane spectra of u, v, w, rho and the first tracer of the new-time state along the normal axis dir (k_spectrum.hip):
    // out[(q * nplanes + p) * nrings + s], PLANE_SPECTRUM_NQ columns; only the two directions in the plane must be periodic.  *nplanes and
    // *nrings are set before the capacities are checked.  Collective; every rank receives the result.
    void plane_spectrum(int dir, int pcap, int rcap, double* out, long* count, int* nplanes, int* nrings);
    // spectral kinetic-energy budget of the new-time state (include/iamrx.h): out[q * nbins + s], BUDGET_NQ columns E, T, D, F.  One
    // FillPatch of the velocity (one ghost layer), the skew-symmetric nonlinear term (k_convect.hip) and, with the turbulent forcing on, its
    // acceleration at cur_time() into arrays that return to the arena, then one packed transform per pair (u_i, N_i) and (u_i, f_i).
    // *nbins is set before the capacity is checked.  Collective; every rank receives the result.
    void spectral_budget(int cap, double* out, long* count, int* nbins);
    // a-priori LES analysis of the new-time velocity (include/iamrx.h: iamrx_mf_sgs; no ghost cell is read): sgs_compute on S[inew].
    // Collective; every rank receives the same statistics.
    void sgs(int kind, double kc, MultiFab* out, int ocomp, int nout, const int* which, double* stats, long* counts)
    {
        sgs_compute(g, S[inew], Xvel, kind, kc, out, ocomp, nout, which, stats, counts);
    }
    // structure functions and two-point correlations along the axes of u, v, w and the first tracer of the new-time state (k_strfn.hip):
    // out[((d * STRFN_NQ + c) * ncol + col) * rcap + r], count[d * rcap + r] and mean[c] (either may be null).  Collective; every rank
    // receives the result.
    void strfn(int pmax, const int rmax[3], int rcap, double* out, long long* count, double* mean);
    // histograms of named fields of the new-time data (k_hist.hip; the binning rule: kernels.h; the names: those of integrate; anything
    // else is an error that lists the known names).  histogram: counts[q * (nbins + 3) + s], s < nbins the bins, then below, above, nan;
    // histogram2: counts[bx * nby + by], then `outside`.  Collective; every rank receives the result.
    void histogram(int n, const std::string* names, const double* lo, const double* hi, int nbins, long long* counts) { histogram_of({this}, n, names, lo, hi, nbins, counts); }
    void histogram2(const std::string& namex, const std::string& namey, const double lo[2], const double hi[2], const int nbins[2], long long* counts)
    { histogram2_of({this}, namex, namey, lo, hi, nbins, counts); }
    double time = 0.0, dt = 0.0;
    int nstep = 0;
    MGStats st_mac, st_nodal, st_visc, st_scal;
    double t_sections[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // accumulated ms: predict, mac, advect, update, visc, nodal
    bool profile_sections = false;

    // ---- AMR hierarchy (amrns.hip): level index, neighbours, StateData times (State_Type: Point; Press_Type / Gradp_Type: Interval,
    // NavierStokesBase::setTimeLevel, Source/NavierStokesBase.cpp:2978-2996), registers owned by the fine level of an interface
    int level = 0, ratio = 1;
    NavierStokes *crse = nullptr, *fine = nullptr;
    double st_new = 0.0, st_old = 0.0, pt_new[2] = {0.0, 0.0}, pt_old[2] = {0.0, 0.0};
    int iteration = 1, ncycle = 1;
    MultiFab mac_phi;                          // MacProj::mac_phi_crse[level]
    MultiFab rho_avg, p_avg;                   // level > 0
    MultiFab Vsync, Ssync;                     // level < finest
    std::unique_ptr<FluxRegister> reg_adv, reg_visc, reg_mac;
    std::unique_ptr<SyncRegister> sync_reg;
    void set_time_level(double time, double dt_old, double dt_new);
    // checkpoint / restart (AmrLevel::checkPoint / restart role, Source/NavierStokesBase.cpp:856-897, 2706-2727): everything of the level
    // that outlives a time step besides the State / Press / Gradp arrays -- the StateData times, step counters, and the initial-guess
    // history of the MAC solve (this library's addition: it makes a restarted run bit-identical to the uninterrupted one).
    // v[0..15] = time, dt, nstep, st_new, st_old, pt_new[2], pt_old[2], dt_prev_mac, have_mac_prev, have_mac_prev2, dt_min_adv, stop_time, inew, pnew
    void get_restart_state(double v[16]) const;
    void set_stop_time(double t) { m_stop_time = t; }      // amr.restart: stop_time comes from the inputs file
    void set_restart_state(const double v[16]);            // call after the arrays are set; also leaves the initial-step state
    MultiFab& mac_phi_history(int which);                  // 0: last MAC potential, 1: the one before (defined on demand)
    // ns.do_LES: the face viscosities of the last velocity_diffusion_update, which 0 eta_n / 1 eta_np1, direction d
    const MultiFab& les_viscosity(int which, int d) const;
    // ---- turbulent forcing (k_turb.hip; getForce of Tutorials/HIT/NS_getForce.cpp:205-707).  The acceleration f(x, t) of the mode table
    // on the cells and one ghost layer, evaluated once per time value and kept (two arrays: the f(t^n+1) estTimeStep asks for is the
    // f(t^n) of the next step); null without forcing.  Every site that forms gravity * rho adds rho * f.  The forcing is on exactly while the
    // level holds a mode table: set_turb_forcing builds upstream's (TurbulentForcing::init_turbulent_forcing for the level's domain, from
    // turb.nmodes / turb.mode_start / turb.div_free_force, TurbulentForcing_def.H:39-49), set_turb_modes takes a caller's (null: off)
    void set_turb_forcing(int nmodes, int mode_start, int div_free) { set_turb_modes(turb_make_table(g, nmodes, mode_start, div_free)); }
    const MultiFab* turb_force_at(double t);
    void set_turb_modes(TurbTableP t) { turb = std::move(t); m_turb_have[0] = m_turb_have[1] = false; }
    const TurbTableP& turb_modes() const { return turb; }
    // ---- tracer particles (k_particles.hip; theNSPC() of NavierStokesBase.cpp:198-222).  A level on its own takes the container over
    // (set_particles: the container is rebound to the level's working boxes and redistributed); a hierarchy binds it and hands every
    // level the pointer (AmrNS::set_particles).  advance() moves the level's particles with u_mac at its end, except in the initial
    // step (NavierStokes.cpp:672-677); step() then redistributes.  Null: nothing is allocated and no launch is added.
    void set_particles(std::shared_ptr<Particles> pc);
    const std::shared_ptr<Particles>& particle_container() const { return particles; }
    // the level's share of the timestamp files (NavierStokesBase::post_timestep_particle, NavierStokesBase.cpp:3908-3951): the state
    // components the container was given (Particles::set_timestamp), FillPatched from the new state on ng ghost layers -- one fill per
    // boundary-condition group: the velocity, each scalar slot -- sampled at the level's particles and appended at the level's new time.
    // Collective on several ranks (the fill); the callers (step, AmrNS::post_timestep) skip a level without particles on any rank
    void timestamp_particles(int ng);
    // the times getForce is called with: the level's own state times in a hierarchy (which keeps them), the level's clock otherwise
    bool amr_times = false;
    double prev_time() const { return amr_times ? st_old : time; }
    double cur_time() const { return amr_times ? st_new : time; }
    const Geometry& geom() const { return g; }
    const LayoutP& lay() const { return layout; }
    const NSParams& params() const { return p; }
    const DomainBC& nodal_bc() const { return bc_nodal; }
    friend class AmrNS;

private:
    // ---- diagnostics.hip.  find_field: the table's entry of a name this run has and the entry point `use` takes (else an error that lists
    // those names).  resolve_fields: where each single-component field of a list is -- state names in place, the others formed into `direct`
    // (field q at dcomp + q) or into `scratch`.  integrate_level, hist_add*_names: this level's part of a diagnostic, over the cells where cov (this
    // level's layout; null: none) is zero; the histograms add every counted cell with `weight` to the device slots.
    const FieldEntry& find_field(const std::string& name, unsigned use, const char* who) const;
    int state_comp(const FieldEntry& e) const;
    void derive_pointwise(const FieldEntry& e, MultiFab& out, int ocomp);
    std::vector<FieldRef> resolve_fields(int n, const std::string* names, unsigned use, const char* who, MultiFab& scratch, MultiFab* direct = nullptr, int dcomp = 0);
    void form_fields(int n, const std::string* names, unsigned use, const char* who, MultiFab& out, int ocomp);
    void finish_sums(int n, double* out) const;
    void integrate_level(int n, const std::string* names, const MultiFab* cov, double* out);
    void hist_add_names(int n, const std::string* names, const MultiFab* cov, const double* lo, const double* hi, int nbins,
                        unsigned long long weight, unsigned long long* d_counts);
    void hist_add2_names(const std::string& namex, const std::string& namey, const MultiFab* cov, const double lo[2], const double hi[2],
                         const int nbins[2], unsigned long long weight, unsigned long long* d_counts);
    // the ONE implementation of each diagnostic, over the levels of a hierarchy, coarsest first (every level over the cells the next
    // finer one does not cover, the levels added in that order); a level is a hierarchy of one and passes {this}, AmrNS its levels
    struct Levels;
    using LevelList = std::vector<NavierStokes*>;
    static void sum_integrated_of(const LevelList& lev, double out[3]);
    static void integrate_of(const LevelList& lev, int n, const std::string* names, double* out);
    static int plane_profile_of(const LevelList& lev, int dir, int bin_level, double* out, int cap);
    static void histogram_of(const LevelList& lev, int n, const std::string* names, const double* lo, const double* hi, int nbins, long long* counts);
    static void histogram2_of(const LevelList& lev, const std::string& namex, const std::string& namey, const double lo[2], const double hi[2], const int nbins[2], long long* counts);
    void advance_setup(double dt, int iteration, int ncycle);
    void swap_time_levels(double dt);
    void fill_gp(MultiFab& G, double time);
    void make_rho_curr_time();
    void adv_registers(MultiFab* const flux[3], int state_indx, int ncomp, double dt);
    double predict_velocity(double dt);
    void mac_project(double dt);
    void velocity_advection(double dt);
    void scalar_advection(double dt);
    void scalar_update_rho(double dt);
    void scalar_update_tracers(double dt);
    void scal_min_max(int comp, bool conservative);
    void velocity_advection_update(double dt);
    void scalar_diffusion_update(double dt);
    void get_visc_terms_scalar(MultiFab& visc, MultiFab& Sdata, int comp);
    void scalar_diffusion_update_one(double dt, int sigma);
    void first_order_extrap(MultiFab& mf);
    // data of the coarse level at this level's time t, on the coarse level's own layout (the crsedata of Diffusion.cpp:733-744, 1725-1736)
    void crse_state_at(MultiFab& out, double t, int scomp, int ncomp);
    void crse_scalar_at(MultiFab& out, double t, int comp, bool over_rho);   // a coarse scalar (divided by the coarse density: rho_flag 2)
    double state_time(const MultiFab& Sdata) const { return &Sdata == &S[1 - inew] ? st_old : st_new; }
    const MultiFab& cf_mask();                 // cf_build_mask of the level (2 ghost cells), level > 0
    // div tau(U^n) of the running advance: getViscTerms(prev_time) is asked for by the velocity prediction, by the advection forcing and
    // (times (1 - theta) dt) by the Crank-Nicolson right-hand side -- one tensor apply instead of three (valid only inside advance())
    MultiFab m_visc_old;
    bool m_visc_old_valid = false, m_in_advance = false;
    // IAMRX_ADVANCE_GLUE ("Advance: the passes around the Godunov kernels").  The velocity forcing (f + visc - Gp) / rho
    // of the old time on one ghost layer, components 0..2 of an nstate-component array: predict_velocity forms it, advection_all (convective
    // form) reads it and adds the scalar components instead of forming all of them again.  Validity as m_visc_old.
    MultiFab m_force;
    bool m_force_valid = false;
    // the right-hand side of the viscous solve and its three max norms, formed by update_all from the u* it holds (valid until
    // velocity_diffusion_update has taken them)
    MultiFab m_visc_rhs;
    double m_visc_rhs_norm[3] = {0.0, 0.0, 0.0};
    bool m_visc_rhs_valid = false;
    bool update_all(double dt);                // the update passes between the advection and the solves in one; false: not applicable
    // ns.do_LES: the face viscosity visc_coef + mu_t of the old state, computed once per advance (the old state does not change inside
    // one; validity as m_visc_old), and that of the new state as velocity_diffusion_update last saw it.  Not allocated without LES.
    MultiFab m_eta_n[3], m_eta_np1[3];
    bool m_eta_n_valid = false, m_eta_have = false;
    std::shared_ptr<Particles> particles;
    MultiFab m_part_umac[3];                   // u_mac on ncycle ghost layers (refined levels with particles only)
    void advect_particles(double dt);
    TurbTableP turb;
    MultiFab m_turb_f[2];
    double m_turb_t[2] = {0.0, 0.0};
    bool m_turb_have[2] = {false, false};
    int m_turb_last = 0;                       // the array handed out last: the other one is overwritten by a new time
    MultiFab m_cf_mask;
    MultiFab m_mac_phi_prev, m_mac_phi_prev2;  // initial guess of the next MAC solve (last two potentials)
    bool m_have_mac_prev = false, m_have_mac_prev2 = false;
    double dt_prev_mac = 0.0;
    bool m_cf_mask_built = false;
    void fill_gradp_bc();
    void set_inflow_ghosts(MultiFab& vel, double scale);
    bool is_diffusive_scal(int comp) const { return scal_diff[comp - Density] > 0.0; }
    void velocity_diffusion_update(double dt);
    void initial_velocity_diffusion_update(double dt);
    void level_project(double dt);
    void initial_velocity_project();
    void initial_pressure_project();
    bool set_outflow_bcs(MultiFab& phi, const MultiFab& rho, int rcomp);   // hydrostatic data on outflow faces (Projection::set_outflow_bcs)
    LayoutP m_outflow_strip[6];
    double m_stop_time = -1.0;
    void initial_sync_project(double dt);
    void get_visc_terms_vel(MultiFab& visc, MultiFab& Sdata);
    // NavierStokes::getViscosity (NavierStokes.cpp:2119-2153) at the time of Sdata (the level's old or new state): ep[d] = the face
    // viscosity.  Without LES the level's constant arrays (nothing computed); with LES visc_coef + mu_t in store[d] (calc_mut_LES:
    // FillPatch of the velocity, the coarse level's velocity on a refined level, the operator's boundary step, k_les_mut) -- or the
    // advance's cached old-time arrays
    void get_viscosity(const MultiFab* ep[3], MultiFab store[3], MultiFab& Sdata);
    void calc_mut_LES(MultiFab out[3], MultiFab& Sdata);
    void compute_visc_terms_vel(MultiFab& visc, MultiFab& Sdata);
    const MultiFab& visc_terms_vel_old(MultiFab& scratch);
    const MultiFab& old_visc_or_zero(MultiFab& scratch);
    void advection_all(double dt);
    void fillpatch(MultiFab& dst, const MultiFab& src, int scomp, int ncomp, const BCRec* bc);
    bool is_diffusive_vel() const { return p.visc_coef > 0.0; }

    Geometry g;
    LayoutP layout;
    NSParams p;
    MGOpts o;
    MultiFab S[2], P[2], Gp[2], Savg;
    int inew = 0, pnew = 0;
    MultiFab u_mac[3], aofs, rho_ptime, rho_ctime, rho_half;
    MultiFab eta[3];
    double dt_min_adv = 1.e200;
    bool initial_step = false, initial_iter = false;
    // NavierStokes::Initialize (NavierStokes.cpp:43-55): Density, Tracer, [Tracer2], [Temp]; per scalar slot (0 = density): advectionType ==
    // Conservative (NS_setup.cpp:297-320), Diffusion::set_rho_flag(diffusionType) (0 Laplacian_S, 1 RhoInverse_Laplacian_S, 2 Laplacian_SoverRho)
    int nstate = 5, nscal = 2, Tracer2 = -1, Temp = -1;
    // ns.do_temp: Divu_Type and Dsdt_Type exist (NS_setup.cpp:365-383).  They are Point-type cell data with the times of State_Type and are kept
    // here as two more components of the S arrays (Divu = nstate, Dsdt = nstate + 1, nalloc = nstate + 2), with their BCRecs in the slots
    // after the scalars: FillPatch in time and from the coarse level, averaging down and the regrid fill treat them like the state
    bool have_divu = false;
    int nalloc = 5, Divu = -1, Dsdt = -1;
    void calc_divu(bool use_new);                                 // NavierStokes::calc_divu (NavierStokes.cpp:1876-1958)
    void calc_dsdt(double dt);                                    // NavierStokesBase::calc_dsdt (NavierStokesBase.cpp:818-858)
    void divu_half(MultiFab& out, double dt, int ng, bool with_dsdt);   // getDivCond(prev_time) (+ dt/2 getDsdt(prev_time)), zero without divu
    int scal_cons[MAXSCAL] = {1, 0, 0, 0}, scal_rho_flag[MAXSCAL] = {1, 0, 0, 1};
    double scal_diff[MAXSCAL] = {-1.0, 0.0, 0.0, 0.0};
    DomainBC bc_mac, bc_nodal, bc_visc[3], bc_scal_lin[MAXSCAL];
    BCRec bc_vel[3], bc_scal[MAXSLOT], bc_gp[3];
    double ed_vel_lo[9], ed_vel_hi[9];     // ext_dir values [n*3+d]
    double ed_scal_lo[3 * MAXSLOT], ed_scal_hi[3 * MAXSLOT];   // ext_dir (inflow) values of density, tracer, ... [n*3+d]
    MultiFab diff_b[MAXSCAL][3];           // scalar diffusivities on faces (defined for the diffusive slots)
    bool any_wall = false;
};

}  // namespace iamrx
