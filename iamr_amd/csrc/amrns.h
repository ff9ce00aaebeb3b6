// iamr_amd/csrc/amrns.h -- the AMR hierarchy driver (amrns.hip): the role of amrex::Amr::coarseTimeStep / timeStep for IAMR's
// NavierStokes levels, NavierStokesBase::post_timestep and the multi-level projections of Projection.
#pragma once
#include "operators.h"
#include "particles.h"
#include <vector>
#include <memory>

namespace iamrx {

MultiFab fine_coverage(const LayoutP& crse, const LayoutP& fine, const Geometry& cgeom, int ratio);

class AmrNS {
public:
    // layouts[l]: boxes of level l in that level's index space (level 0 covers the domain); ratio 2 between levels
    AmrNS(const Geometry& g0, const std::vector<LayoutP>& layouts, int ratio, const NSParams& p, const MGOpts& o);
    int nlevels() const { return (int)lev.size(); }
    NavierStokes& level(int l) { return *lev[l]; }
    void post_init(double stop_time);            // NavierStokes::post_init for the hierarchy (Source/NavierStokes.cpp:1254-1299)
    double coarse_step();                        // Amr::coarseTimeStep; returns the level-0 dt
    double time() const { return lev[0]->time; }
    double dt(int l) const { return dt_level[l]; }
    MGStats st_sync, st_mac_sync;                // last MLsyncProject / mac_sync_solve
    // Hydro::NodalProjector::project on levels c0 .. c0+nl-1 (Projection::doMLMGNodalProjection with nlevel > 1)
    MGStats composite_project(int c0, int nl, MultiFab* const vel[], const int vcomp[], MultiFab* const phi[], const MultiFab* const sig[],
                              const MultiFab* rhnd, double rtol, double atol, bool increment_gp, double inflow_scale, const MultiFab* const rhcc[] = nullptr);
    ProjLevel proj_level(int l);                 // the descriptor of level l for composite_project / ml_sync_project
    // building blocks, public for the unit tests
    void reflux(int l);
    void avg_down(int l);
    void mac_sync(int l);
    void level_sync(int l, int crse_iteration = -1);      // crse_iteration: of level l within the step of level l-1 (-1: the last one)
    void post_timestep(int l, int crse_iteration = -1);
    void time_step(int l, double time, int iteration, int niter);
    // NavierStokes::sum_integrated_quantities (NavierStokes.cpp:1046-1079): composite mass, tracer and kinetic energy -- every level over the
    // cells the next finer one does not cover, the levels added coarsest first.  post_init and level 0's post_timestep (every
    // sum_interval-th level-0 step) call it and leave what they found in last_sum (last_sum_step: the level-0 step count then, -1: never)
    void sum_integrated_quantities(double out[3]) { NavierStokes::sum_integrated_of(levels(), out); }
    double last_sum[3] = {0.0, 0.0, 0.0}, last_sum_time = 0.0;
    // the same for named fields (the names: NavierStokes::integrate): out[q] = composite volume-weighted sum of
    // field names[q], every level with its own cell volume over the cells the next finer one does not cover, coarsest first
    void integrate(int n, const std::string* names, double* out) { NavierStokes::integrate_of(levels(), n, names, out); }
    // plane-averaged profile of the composite state along dir (k_profile.hip): the PROFILE_NQ volume-weighted means of every slab of the
    // index space of level bin_level (0 .. finest), over the cells no finer level covers; out[q * nbins + b].  Returns nbins.
    int plane_profile(int dir, int bin_level, double* out, int cap) { return NavierStokes::plane_profile_of(levels(), dir, bin_level, out, cap); }
    // composite histograms of named fields (k_hist.hip; the names: NavierStokes::integrate): level l counts the cells level l + 1 does not
    // cover, each with the weight 8^(finest - l), so the slots are in units of finest-level cell volumes and together sum to
    // cells(level 0) * 8^finest (an error unless that stays below 2^53).  Layout of counts as NavierStokes::histogram / histogram2.
    void histogram(int n, const std::string* names, const double* lo, const double* hi, int nbins, long long* counts) { NavierStokes::histogram_of(levels(), n, names, lo, hi, nbins, counts); }
    void histogram2(const std::string& namex, const std::string& namey, const double lo[2], const double hi[2], const int nbins[2], long long* counts)
    { NavierStokes::histogram2_of(levels(), namex, namey, lo, hi, nbins, counts); }
    int last_sum_step = -1;
    // ---- regridding (Amr::regrid from level 0 at the start of a coarse step; NavierStokes::errorEst, NS_error.cpp:10-145;
    // NavierStokesBase::init(AmrLevel&) / init(), NavierStokesBase.cpp:1713-1806) ----
    struct TagRule {
        int comp = Tracer;              // state component, or -1: magnitude of vorticity (mag_vort)
        int mode = 0;                   // 0 value_greater, 1 value_less, 2 vorticity_greater (x 2^level), 3 adjacent_difference_greater
        std::vector<double> value;      // per level (the last one repeats)
        int max_level = 1000;           // tags only on levels < max_level
        bool has_box = false;
        double box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    };
    struct RegridOpts {
        int max_level = 0, regrid_int = 0;
        int blocking_factor = 8, max_grid_size = 32, n_error_buf = 1;
        double grid_eff = 0.7;
        int do_refine_outflow = 0, do_derefine_outflow = 1, nbuf_outflow = 1;   // ns.do_refine_outflow / do_derefine_outflow / Nbuf_outflow (NavierStokesBase.cpp:136-138)
        int compute_new_dt_on_regrid = 0;   // amr.compute_new_dt_on_regrid (Amr::timeStep: computeNewDt(post_regrid_flag = 1) after a level-0 regrid; default 0)
        std::vector<TagRule> rules;
    };
    void set_regrid(const RegridOpts& r) { const int keep = rg.compute_new_dt_on_regrid; rg = r; if (!r.compute_new_dt_on_regrid) rg.compute_new_dt_on_regrid = keep; }
    void set_compute_new_dt_on_regrid(int on) { rg.compute_new_dt_on_regrid = on; }
    void set_outflow_tagging(int refine, int derefine, int nbuf) { rg.do_refine_outflow = refine; rg.do_derefine_outflow = derefine; rg.nbuf_outflow = nbuf; }
    // new grids of levels 1 .. max_level from the tags of the current data (coarse to fine nesting enforced); the level-l boxes
    std::vector<std::vector<BoxD>> make_new_grids(int lbase = 0);
    // install grids (levels 1 ..): new levels are filled from the old level where it existed and from the next coarser level elsewhere;
    // returns false if nothing changed
    bool install_grids(const std::vector<std::vector<BoxD>>& grids, int lbase = 0, double cur_time = 0.0);
    bool regrid(int lbase = 0, double cur_time = 0.0) { return install_grids(make_new_grids(lbase), lbase, cur_time); }
    // Amr::timeStep's regrid check (okToRegrid(i) for i = level .. finest at the start of every step of every level): level_count_v[i] = steps
    // of level i since the grids above it were last rebuilt.  regrid_log: what was rebuilt during the last coarse step (base level, time,
    // boxes per level) -- a driver that mirrors the hierarchy elsewhere (the tests' oracle) replays it
    std::vector<int> level_count_v;
    struct RegridEvent { int lbase; double time; std::vector<std::vector<BoxD>> grids; };
    std::vector<RegridEvent> regrid_log;
    void maybe_regrid(int l, double time);
    int level_count = 0;                // coarse steps since the last regrid (Amr::level_count[0])
    // Amr::checkPoint / restart: dt_level, dt_min, n_cycle per level, level_steps, level_count, stop_time
    void get_restart_state(double* dt_lev, double* dt_mn, int* ncyc, int counters[2], double* stop) const;
    void set_restart_state(const double* dt_lev, const double* dt_mn, const int* ncyc, const int counters[2], double stop);
    void get_level_counts(int* counts, int n) const;
    void set_level_counts(const int* counts, int n);
    // turbulent forcing: the mode table is built once from the level-0 domain (set_turb_forcing: upstream's table) or handed in
    // (set_turb_modes: a caller's; null: off) and shared by every level, also by the levels a regrid creates
    void set_turb_modes(TurbTableP t) { turb = t; for (auto& s : lev) s->set_turb_modes(t); }
    void set_turb_forcing(int nmodes, int mode_start, int div_free) { set_turb_modes(turb_make_table(lev[0]->geom(), nmodes, mode_start, div_free)); }
    // tracer particles: ONE container for the hierarchy (NSPC, NavierStokesBase.cpp:198-222), bound to the levels' working boxes and bound
    // again after every regrid (post_regrid: Redistribute(lbase), :2448-2452); post_timestep(l) redistributes the levels l .. finest
    // (post_timestep_particle, :3866-3879).  Null: off
    void set_particles(ParticlesP pc);
    const ParticlesP& particle_container() const { return particles; }
    uint64_t grid_generation() const { return m_grid_gen; }   // incremented whenever the grids change
    uint64_t m_grid_gen = 0;
    // section profile of the coarse step (host clock around stream syncs, only while profile_on): [0] reflux, [1] avgDown,
    // [2] mac_sync_solve, [3] mac_sync rest (re-advection, viscous / scalar sync solves, SyncInterp), [4] level_sync (MLsyncProject +
    // interpolation to finer levels), [5] regrid, [8 + l] advance of level l (all its sub-steps; the level's own t_sections split it further)
    bool profile_on = false;
    double t_prof[16] = {0};
    void set_profile(bool on);

private:
    NSParams p;
    MGOpts o;
    std::vector<std::unique_ptr<NavierStokes>> lev;
    std::vector<int> n_cycle;
    std::vector<double> dt_level, dt_min;
    int level_steps = 0;
    double stop_time = -1.0;
    RegridOpts rg;
    TurbTableP turb;
    ParticlesP particles;
    void bind_particles();
    // what the diagnostics above walk (diagnostics.hip: ONE implementation of each for a level and a hierarchy)
    std::vector<NavierStokes*> levels() const { std::vector<NavierStokes*> v; for (auto& s : lev) v.push_back(s.get()); return v; }
    int m_ratio = 2;
    void link_level(int l);
    void check_nesting(const std::vector<BoxD>& fine, const std::vector<BoxD>& crse, const Geometry& cgeom, int l) const;
    void validate_grids(const std::vector<std::vector<BoxD>>& grids, int lbase = 0) const;   // throws before anything is modified
    void compute_new_dt(bool post_regrid);
};

}  // namespace iamrx
