/*
 * include/iamrx.h -- C-ABI of libiamrx.so: the MI355X-native (gfx950) replacement for the
 * data-parallel hot path of AMReX-Fluids/IAMR.
 *
 * Conventions
 *   - every entry point returns 0 on success, non-zero on failure; iamrx_last_error() gives the
 *     message.  IAMR itself has no return codes (errors are amrex::Abort, e.g. reference
 *     Source/NavierStokesBase.cpp:501-507): the reference-side wrapper turns non-zero into Abort.
 *   - arrays are double precision, AMReX Array4 layout seen at IAMR's seam (reference
 *     Source/NavierStokesBase.cpp:4665-4677): offset(i,j,k,n) = (i-lo0) + n0*((j-lo1) + n1*((k-lo2) + n2*n)),
 *     ghost cells included; index boxes are inclusive [lo,hi].
 *   - all compute runs on the library's HIP stream of the selected device; there is NO CPU fallback:
 *     iamrx_init fails if no gfx950 device is present.
 *   - handles are opaque; objects are owned by the library until the matching *_destroy.
 *
 * Each function cites the reference interface it replaces (file:line relative to /root/reference).
 */
#ifndef IAMRX_H
#define IAMRX_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct iamrx_layout_s* iamrx_layout;   /* BoxArray + DistributionMapping of one level */
typedef struct iamrx_fluxreg_s* iamrx_fluxreg; /* amrex::FluxRegister of one coarse/fine interface (see below) */
typedef struct iamrx_mf_s* iamrx_mf;           /* MultiFab (device resident) */
typedef struct iamrx_ns_s* iamrx_ns;           /* NavierStokes level object */
typedef struct iamrx_syncreg_s* iamrx_syncreg; /* SyncRegister of one coarse/fine interface */
typedef struct iamrx_particles_s* iamrx_particles; /* tracer particles of a level or a hierarchy (see below) */
typedef struct iamrx_amr_s* iamrx_amr;         /* hierarchy of NavierStokes levels (the Amr / AmrLevel role for the hot path) */

typedef struct iamrx_geom {
    int dom_lo[3], dom_hi[3];       /* cell-centred domain box */
    double prob_lo[3], prob_hi[3];
    int periodic[3];
} iamrx_geom;

/* MLMG controls (defaults = reference defaults, except the nodal cycle shape, see nodal_nu1: Source/MacProj.cpp:41-101, Source/Projection.cpp:19-37,
 * Source/Diffusion.cpp:85-96 and upstream amrex::MLMG nu1=nu2=2, nuf=8, bottom BiCGStab rtol 1e-4) */
typedef struct iamrx_mg_opts {
    int nu1, nu2, nuf, nub;
    int max_iters, bottom_maxiter;
    double bottom_reltol;
    double omega;
    int maxorder;
    int max_coarsening_level, min_width;
    int nodal_sweeps, nodal_smoother;
    int verbose;
    int bottom_smoother_only;
    int fixed_iters;
    /* nodal V-cycle shape: pre / post smooth calls (nodal_sweeps Gauss-Seidel sweeps each).  amrex::MLNodeLaplacian / MLMG use 4 sweeps and
     * 2 + 2 calls; iamrx_mg_default_opts() gives 2 sweeps and 1 + 1 calls -- the converged solution is the same, the time to solution is
     * 1/3 shorter on MI355X.  Set nodal_sweeps = 4, nodal_nu1 = nodal_nu2 = 2 for the upstream cycle. */
    int nodal_nu1, nodal_nu2;
    /* cell-centred bottom: 1 (default) = the hierarchy ends at the first single-box level of <= 8^3 cells, solved by one single-workgroup
     * device launch (BiCGStab to bottom_reltol + nub sweeps, no host synchronisation); 0 = coarsen to min_width, host-driven BiCGStab
     * (amrex::MLMG's shape).  Same converged solution. */
    int device_bottom;
    /* 1: the level is a 2-D problem lifted onto a thin periodic slab (iamr_amd/inputs.py lift_2d): once the slab is two cells thick the
     * multigrid keeps it at two cells and coarsens the plane only.  0 (default): ordinary coarsening.  A property
     * of the problem handed to each solver, not process-wide state (the IAMRX_MG_SLAB switch still forces it for tests). */
    int slab;
} iamrx_mg_opts;

typedef struct iamrx_mg_stats {
    int iters;
    double resnorm0, rhsnorm0, resnorm;
    int bottom_iters_total;
    int converged;             /* 1: the tolerance was met; 2 (nodal solves): the residual stalled at the fp64 round-off floor within 100x of the tolerance (h <= 1/512) */
    double vcycle_ms;
    int nlevels;
} iamrx_mg_stats;

/* ---- runtime ---------------------------------------------------------------------------- */
int iamrx_init(int device);                      /* amrex::Initialize role (Source/main.cpp:26-40) */
int iamrx_finalize(void);
const char* iamrx_last_error(void);
int iamrx_sync(void);                            /* amrex::Gpu::synchronize */
void* iamrx_stream(void);                        /* the hipStream_t every kernel is launched on */
int iamrx_mem_info(size_t* bytes_live, size_t* bytes_cached);
int iamrx_alloc_count(size_t* n_device_malloc);  /* hipMalloc calls so far (caching-allocator misses; The_Arena role) */
/* Run-time switches (kernel variants kept for A/B measurement and as references of the parity tests, solver
 * shortcuts, tile shapes) live in ONE registry.  It is filled once, at iamrx_init, from the environment variables IAMRX_<KEY> that are
 * set (e.g. IAMRX_GODUNOV_Z=0 -> key "GODUNOV_Z"), can be changed afterwards only through iamrx_tuning_set, and is consulted at the
 * point of use -- a change takes effect at the next call; nothing is cached for the life of the process.  Per-solve choices that belong
 * to a call are arguments (iamrx_mg_opts, the Godunov `scheme`), not keys. */
int iamrx_tuning_set(const char* key, double value);
int iamrx_tuning_get(const char* key, double default_value, double* value);
/* scoped wall-time profile of the library's host-side sections (measurement aid; synchronises the stream at every scope boundary while
 * enabled).  Writes the accumulated report (one line per scope path: name, ms, calls) into report[capacity] first (may be NULL), then
 * enable: 1 on, 0 off, -1 unchanged; reset != 0 clears the accumulated times. */
int iamrx_scope_profile(int enable, int reset, char* report, size_t capacity);
/* halo exchanges with other ranks since iamrx_init: out[0] exchanges issued on the main stream (in front of the kernel that needs the data:
 * exposed), out[1] doubles sent by them; out[2] / out[3] the same for exchanges issued on the side stream beside interior work (the
 * multi-box red + black sweep: hidden as far as the interior tiles last); the role of the comm rows of a TINY_PROFILE */
int iamrx_exchange_counts(size_t out[4]);
/* how often the level objects have merged a caller's boxes so far (IAMRX_COALESCE = 1, the default): lets a test
 * harness tell the calls whose result depends on that mode (tests/conftest.py runs those in both).  No counterpart upstream. */
int iamrx_coalesce_merge_count(size_t* n);
int iamrx_sync_count(size_t* n_stream_sync);     /* host waits on the library stream so far (scalar read-backs of norms / dot products, plan uploads) */
/* HIP-event stopwatch on the library stream (the role of BL_PROFILE / ParallelDescriptor::second() pairs,
 * e.g. Source/NavierStokesBase.cpp:2088-2107): start records an event, stop records + waits and returns ms */
int iamrx_timer_start(void);
int iamrx_timer_stop(double* ms);
void iamrx_mg_default_opts(iamrx_mg_opts* o);
/* HIP-event probes around the launches of one kernel family inside running solves (the role of TINY_PROFILE rows such as MLMG smoother
 * times): which = 0 nodal Gauss-Seidel pass (k_nodal_gs4), 1 scalar GSRB colour pass (k_abec_gsrb), 2 fused Godunov advection (k_god_z), 3 fused
 * velocity prediction (k_pred_z); only launches on levels
 * with at least min_points nodes / cells per box, every stride-th one.  stop waits for the stream and returns the summed durations. */
int iamrx_kernel_probe_start(int which, long min_points, int stride);
int iamrx_kernel_probe_stop(int which, double* total_ms, long* launches);

/* ---- communicator (amrex::ParallelDescriptor / FabArray point-to-point role) ------ */
/* One process per GPU.  Call AFTER iamrx_init and BEFORE creating layouts.  RCCL: rank 0 obtains a unique id,
 * the host program broadcasts the 128 bytes (MPI_Bcast / torch.distributed), every rank calls init. */
int iamrx_comm_get_unique_id(char id[128]);
int iamrx_comm_init_rccl(const char id[128], int rank, int nranks);
/* transport supplied by the host program (tests: torch.distributed gloo); buffers are host memory.
 * op: 0 sum, 1 max, 2 min */
typedef void (*iamrx_allreduce_cb)(double* vals, int n, int op);
typedef void (*iamrx_exchange_cb)(int nsend, const int* send_peers, double** send_bufs, const long* send_counts,
                                  int nrecv, const int* recv_peers, double** recv_bufs, const long* recv_counts);
int iamrx_comm_init_callback(int rank, int nranks, iamrx_allreduce_cb ar, iamrx_exchange_cb ex);
int iamrx_comm_rank(int* rank, int* nranks);
/* all-reduce of a HOST buffer over the ranks through the installed communicator (RCCL or the callback transport; one rank: the buffer is
 * left as it is); op as iamrx_allreduce_cb.  Collective.  The ParallelDescriptor::ReduceRealSum / Barrier role for host-side code (the
 * plotfile / checkpoint writers exchange file offsets and minima / maxima with it and use a one-element sum as their barrier). */
int iamrx_comm_allreduce(double* vals, int n, int op);
/* transport probe: exchange `count` doubles with `peer` through the installed communicator (peer == own rank: loop-back); 0 = data intact */
int iamrx_comm_probe_exchange(int peer, long count);
const char* iamrx_comm_last_error(void);

/* ---- containers (amrex::BoxArray/DistributionMapping/MultiFab role) ----------- */
int iamrx_layout_create(int nboxes, const int* lo_hi /* 6 ints per box: lo[3],hi[3] */, const int* owner_rank,
                        iamrx_layout* out);
/* The level objects (iamrx_ns_*, iamrx_amr_*) work on the caller's boxes MERGED: boxes of one owner rank that share a full face become one box,
 * repeatedly (one process drives one GPU, so small boxes inside a rank only cost ghost fills and launches; the reference's amr.max_grid_size
 * chopping -- RunningProblems.rst:362-368 -- is undone inside the level and restored at its data accessors, which keep speaking the caller's
 * boxes).  This returns the merged boxes of a layout; IAMRX_COALESCE = 0 (iamrx_tuning_set("COALESCE", 0)) switches the merging off. */
int iamrx_layout_coalesced_boxes(iamrx_layout l, int* nboxes, int* lo_hi /* 6 ints per box, or NULL to query the count */);
int iamrx_layout_destroy(iamrx_layout l);
int iamrx_layout_nlocal(iamrx_layout l, int* nlocal);
int iamrx_layout_local_box(iamrx_layout l, int local_idx, int lo_hi[6], int* global_idx);
/* the DistributionMapping: owner rank of every box, in box order (nboxes ints) -- what a regrid's knapsack dealt (iamrx_amr_level_layout) */
int iamrx_layout_owners(iamrx_layout l, int* owners /* nboxes */);
int iamrx_mf_create(iamrx_layout l, const int type[3] /* 1 = nodal in that direction */, int ncomp, int ngrow, iamrx_mf* out);
int iamrx_mf_destroy(iamrx_mf m);
int iamrx_mf_info(iamrx_mf m, int* ncomp, int* ngrow, int type[3], int* nlocal);
int iamrx_mf_fab_box(iamrx_mf m, int local_idx, int lo_hi[6]);         /* allocated region incl. ghosts */
int iamrx_mf_dev_ptr(iamrx_mf m, int local_idx, double** p);
int iamrx_mf_to_host(iamrx_mf m, int local_idx, double* dst);            /* whole fab, all comps */
int iamrx_mf_from_host(iamrx_mf m, int local_idx, const double* src);
int iamrx_mf_setval(iamrx_mf m, double v);                                /* MultiFab::setVal */
int iamrx_mf_copy(iamrx_mf dst, iamrx_mf src, int scomp, int dcomp, int ncomp, int ngrow);  /* MultiFab::Copy */
int iamrx_mf_fill_boundary(iamrx_mf m, const iamrx_geom* g);              /* FillBoundary(geom.periodicity()): Source/MacProj.cpp:1127 */
/* physical-BC fill of cell-centred ghost cells outside the domain (the BCRec part of FillPatch; ext_dir with constant
 * boundary values as in Source/NS_bcfill.H:17-95 / Source/NavierStokes.cpp:72-83).  bcrec: [ncomp][6];
 * extdir_lo/hi: [ncomp][3] boundary values (may be NULL) */
int iamrx_mf_fill_physbc(iamrx_mf m, const iamrx_geom* g, int scomp, int ncomp, const int* bcrec, const double* extdir_lo,
                         const double* extdir_hi);
int iamrx_mf_norm0(iamrx_mf m, int comp, int ncomp, int ngrow, double* out);   /* MultiFab::norm0: Source/NavierStokesBase.cpp:4408 */
/* The library's other level-wide reductions, each a thin call of the internal one (tests/test_gpu_reductions.py compares them with
 * numpy).  Every maximum of absolute values follows one rule: a NaN anywhere in the region read gives +inf, +-inf gives +inf, and the
 * result does not depend on where the NaN sits.
 * norm0_comps: out[n] = max |m(comp + n)| over the valid region grown by ngrow, n < ncomp.  form 0: MultiFab::norm0_comps; form 1: the
 * functor reduction (reduce_max_f<ncomp>, finish read back by the host); form 2: the same with the finish left on the device
 * (reduce_max_f_dev<ncomp>, the device-resident Krylov loop's form), then copied back.  Forms 1 and 2 take ncomp = 1, 3 or 6; their
 * per-point functor keeps a NaN as NaN, so the combine steps have to carry it to the end, where it is reported as +inf. */
int iamrx_mf_norm0_comps(iamrx_mf m, int comp, int ncomp, int ngrow, int form, double* out);
/* smallest and largest value of one component over the valid region grown by ngrow; a NaN gives mn = -inf, mx = +inf */
int iamrx_mf_minmax(iamrx_mf m, int comp, int ngrow, double* mn, double* mx);
/* owner-weighted dot products over the valid points (MultiFab::Dot of the solvers): out[0] = x0.y0, out[1] = x1.y1 (x1 = y1 = NULL: out[0]
 * only), components comp .. comp + ncomp - 1.  Nodal / face data: every point counted once, weight 1/2 per Neumann wall a node lies on;
 * lobc / hibc are the LinOpBC codes of iamrx_nodal_solve and give the walls as the nodal solver sees them.  on_device: the finish
 * left on the device (the device-resident Krylov loop's form), then copied back. */
int iamrx_mf_dot(const iamrx_geom* g, const int lobc[3], const int hibc[3], iamrx_mf x0, iamrx_mf y0, iamrx_mf x1, iamrx_mf y1, int comp,
                 int ncomp, int on_device, double out[2]);
/* owner-weighted sum of one component (MultiFab::sum_unique), with the weights of iamrx_mf_dot */
int iamrx_mf_sum_unique(const iamrx_geom* g, const int lobc[3], const int hibc[3], iamrx_mf m, int comp, double* out);

/* host-only (works without a GPU): the ghost-exchange plan that `rank` executes for FillBoundary of a level
 * (FabArray::FillBoundary role).  desc: 16 ints per descriptor = kind (0 local copy, 1 pack+send, 2 recv+unpack),
 * peer rank, src global box, dst global box, region lo[3] hi[3] (destination index frame), shift[3]
 * (src index = dst index + shift), buffer offset in points, 2 pad.  Call with desc == NULL to size. */
int iamrx_host_fill_plan(int nboxes, const int* lo_hi, const int* owner, int rank, const int type[3], int ngrow, const iamrx_geom* g,
                         int max_desc, int* desc, int* ndesc);
/* the same for a fill whose SOURCE boxes also hand on their first `wall_ext` ghost layers beyond the non-periodic sides of the domain
 * (cell-centred data; the two-layer density copy of the multi-box sweep: the edge ghost cells beyond a wall behind a box-box face take
 * the face ghost values of the box next door).  No counterpart upstream: amrex::FillBoundary copies valid cells only. */
int iamrx_host_fill_plan_wall_ext(int nboxes, const int* lo_hi, const int* owner, int rank, const int type[3], int ngrow, const iamrx_geom* g,
                                  int wall_ext, int max_desc, int* desc, int* ndesc);

/* host-only (works without a GPU): how a smoothing call of the cell-centred multigrid (MLMG::mgVcycle's smooth on MLABecLaplacian /
 * MLTensorOp, as set up at MacProj.cpp:1150-1183 and Diffusion.cpp:715-923) runs on a level -- decided once per level per solve, from the
 * level's global box list.  lo_hi: 6 ints per box; lobc / hibc: LinOpBC codes; coef 0: stored face coefficients, 1: recomputed from the
 * density, 2: uniform; has_cf: the level has coarse/fine faces; finest: level 0 of its hierarchy; ngrow: ghost widths of the correction,
 * the right-hand side, the density and the a-term.  out[0] path (0 two colour passes, 1 one-launch sweep on a box spanning the domain,
 * 2 on a refined box strictly inside it, 3 on several boxes covering it, 4 the opt-in fused sweep + shell pass), out[1] wavefronts of a
 * sweep workgroup (12 / 16), out[2] sweep issued in two parts, out[3] the first sweep may start from zero; the colour pass: out[4] kernel
 * (0 general, 1 plane-pipelined, 2 pair-marching, 3 pair-marching per component), out[5] coefficient mode, out[6] planes in flight,
 * out[7] coarse/fine ghost cells maintained, out[8] all ghost cells coarse/fine, out[9] periodic index wrap, out[10] walls applied in the
 * kernel, out[11] first pass from zero allowed.  No counterpart upstream (amrex picks nothing: one smoother kernel). */
int iamrx_host_abec_smoother_plan(int nboxes, const int* lo_hi, const iamrx_geom* g, const int lobc[3], const int hibc[3], int maxorder, int ncomp,
                                  int coef, int has_a, int has_cf, int finest, const int ngrow[4], int out[12]);
/* host-only (works without a GPU): whether level `level` (0 = finest) of a cell-centred hierarchy runs the down leg of a V-cycle (nu1
 * sweeps from zero, residual, restriction) and its up leg (prolongation, nu2 sweeps) as ONE launch each instead of ten.  Inputs as for
 * iamrx_host_abec_smoother_plan, plus the level, the cycle shape and whether the step to the next coarser level goes through a slab or an
 * agglomerated level.  out[0] legs (0 / 1); out[1..3] tile lengths of the down leg, out[4..6] of the up leg (zero without legs); out[7],
 * out[8] the halo widths 2 nu1, 2 nu2 by which a workgroup grows its tile.  No counterpart upstream. */
int iamrx_host_abec_leg_plan(int nboxes, const int* lo_hi, const iamrx_geom* g, const int lobc[3], const int hibc[3], int maxorder, int ncomp,
                             int coef, int has_a, int has_cf, int finest, const int ngrow[4], int level, int nu1, int nu2, int slab_transition,
                             int agg_transition, int out[9]);
/* host-only (works without a GPU): how a smoothing call and the bottom solve of the nodal multigrid (MLMG::mgVcycle on MLNodeLaplacian, as set
 * up at Projection.cpp:2512-2542) run on a level -- decided once per level per solve, from the level's global box list (a single rank's view).
 * lo_hi: 6 ints per box; lobc / hibc: LinOpBC codes; has_mask: the level has Dirichlet nodes (outflow faces, the boundary of a refined
 * level); nodal_smoother, bottom_smoother_only, device_bottom, nodal_sweeps: iamrx_mg_opts; coarsest: the last level of its hierarchy;
 * ngrow: ghost widths of the correction and of the right-hand side (the solver allocates both with out[1]).  out[0] path (0 weighted Jacobi,
 * 1 eight colour passes, each behind a ghost fill, 2 every sweep in one single-workgroup launch, 3 two plane-fused passes per sweep staged
 * in LDS, 4 the same register-resident), out[1] ghost width the solver allocates, out[2] images read by index wrap instead of ghost nodes,
 * out[3] directions with mirror images about Neumann walls (bit d), out[4] the residual and the restriction read images too (no ghost fill
 * inside a cycle), out[5] no zero fill behind the allocation, out[6] the first sweep on a zero correction is told so, out[7] ghost fills
 * of one plane parity, out[8] a pass behind a ghost fill can be issued in two parts, out[9] bottom solve (0 not the coarsest level,
 * 1 smoothing calls only, 2 single-workgroup device solver of a periodic box, 3 the same with walls / Dirichlet nodes, 4 BiCGStab driven
 * from the host), out[10] sweeps per smoothing call.  No counterpart upstream (amrex picks nothing: one smoother kernel). */
int iamrx_host_nodal_smoother_plan(int nboxes, const int* lo_hi, const iamrx_geom* g, const int lobc[3], const int hibc[3], int has_mask,
                                   int nodal_smoother, int bottom_smoother_only, int device_bottom, int nodal_sweeps, int coarsest, const int ngrow[2],
                                   int out[11]);
/* host-only (works without a GPU): the launches ONE call of the fused Godunov kernels issues on a level -- pred 1: ExtrapVelToFaces
 * (k_pred_z, ncomp 3), pred 0: ComputeAofs (k_god_z) -- decided at every call from the level's box list (lo_hi: 6 ints per box, a single
 * rank's view), the geometry, the call's flags (scheme 0 PLM / 1 PPM, forcing present, use_forces_in_trans, divu present, edge states /
 * fluxes stored, the components' iconserv) and the tuning keys IAMRX_GODUNOV_ZTX / _PTX / _ZKC / _SPLIT_BC / _SPEC.
 * head: tile cells in x and y, planes of a z-chunk, launches (<= 4), z-chunks (<= 18).  launches: 16 ints each, in issue order -- sel (0 the
 * full tile grid, 1 the tiles off the walls, 2 the tiles at the walls), boundary-condition variant, the template flags FRC, DVU, OUT, CNS (-1:
 * run-time value), components, 0, the component table (8).  starts: first plane of every chunk relative to the box, then the length.
 * tiles (5 ints each; none when sel is 0): class (0 off / 1 at the walls), box, tile x, tile y, chunk, in the order the launch works through
 * them; box -1: padding of a class of >= 64 tiles, whose list is dealt to the eight XCDs.  *ntiles entries exist, at most max_tiles are
 * written (tiles may be null).  No counterpart upstream. */
int iamrx_host_godunov_plan(int pred, int nboxes, const int* lo_hi, const iamrx_geom* g, int scheme, int has_force, int fit, int has_divu, int edge_out,
                            int flux_out, int ncomp, const int* iconserv, int head[5], int launches[64], int starts[20], int* tiles, int max_tiles, int* ntiles);

/* ---- cell-centred linear operator primitives (amrex::MLABecLaplacian role) ---- */
/* one red or black Gauss-Seidel pass of (alpha*a - beta div b grad) phi = rhs; ghost cells of phi must be filled */
int iamrx_abec_gsrb(const iamrx_geom* g, double alpha, double beta, iamrx_mf a /* may be NULL */, iamrx_mf bx, iamrx_mf by, iamrx_mf bz,
                    iamrx_mf phi, iamrx_mf rhs, int redblack, double omega, const int lobc[3], const int hibc[3], int maxorder);
/* one full red+black sweep with the ghost/BC fill in front of each colour (homogeneous BC, as inside MLMG::mgVcycle);
 * fused = 1: single-pass kernel (red everywhere + black off the box surfaces) followed by the black pass on the box surfaces */
/* The finest-level kernel forms of the cell-centred multigrid on caller data (inside a solve CellMG picks them by itself): coef = 1: the MAC
 * operator with its face coefficients b_d = scale / (0.5 (rho(cell - e_d) + rho(cell))) recomputed from the cell-centred rho (>= 1 filled ghost
 * cell; the role of MacProj.cpp:1098-1128's coefficients), coef = 2: uniform face coefficients bu[3] (constant viscosity / diffusivity).
 * op 0 / 1: red / black colour pass on phi (ghost cells filled by the caller; abec_gsrb role); 4 / 5: the same with the index wrap of one box
 * spanning a periodic domain (no ghost cells read); 2: out = rhs - L phi; 3: out (on the layout coarsened by 2) = restriction of rhs - L phi;
 * 6: out = phi after one red + black sweep in ONE launch (one box spanning the domain, 128 or 256 cells in x, every side periodic, Neumann,
 * reflect-odd or Dirichlet of order <= 3 -- homogeneous, as inside a V-cycle; no ghost cell of phi is read; out != phi, >= 1 ghost cell),
 * 7: the same with phi taken as zero without being read; 8 / 9: the sweep of 6 / 7 on a level of SEVERAL boxes that covers its domain (a
 * chopped level; the boxes of a level sharded over GPUs; rows of 128 / 256 cells in every box): phi and out with two ghost layers, rhs
 * with one, rho with two -- the entry fills them from the neighbour boxes / periodic images (one exchange per sweep instead of one per
 * colour; rho's ghost cells beyond domain walls stay the caller's), updates the red ghost cells next to box faces in place and sweeps;
 * 10 / 11: the sweep of 6 / 7 on a REFINED level that is one box strictly inside the domain g (ratio 2 to the level below; the role of
 * MLLinOp::setCoarseFineBC's homogeneous ghost values inside MLMG::mgVcycle on a level set up by MacProj.cpp:1166-1170): every face of the
 * box is a coarse/fine face whose ghost value of order `maxorder` (<= 4: the face cell, the cell behind it and the one behind that) the
 * kernel forms itself; no ghost cell of phi is read, rho's first ghost layer is the caller's (FillPatch). */
int iamrx_abec_form(const iamrx_geom* g, int coef, iamrx_mf rho, int rho_comp, double scale, const double bu[3], double beta, int op,
                    iamrx_mf phi, iamrx_mf rhs, iamrx_mf out, double omega, const int lobc[3], const int hibc[3], int maxorder);
int iamrx_abec_gsrb_sweep(const iamrx_geom* g, double alpha, double beta, iamrx_mf a /* may be NULL */, iamrx_mf bx, iamrx_mf by, iamrx_mf bz,
                          iamrx_mf phi, iamrx_mf rhs, double omega, const int lobc[3], const int hibc[3], int maxorder, int fused);
/* out = rhs - L(phi)  (rhs == NULL: out = L(phi)).  tensor = 1: MLTensorOp on a 3-component phi whose ghost cells (edges and corners
 * included) are filled; b* hold b_d(comp) in 3 components, or the face viscosity in 1 component -- then the level residual of a tensor
 * solve runs, constant viscosity in its fused launch (k_tensor_uni). */
int iamrx_abec_residual(const iamrx_geom* g, double alpha, double beta, iamrx_mf a, iamrx_mf bx, iamrx_mf by, iamrx_mf bz,
                        iamrx_mf out, iamrx_mf phi, iamrx_mf rhs, int tensor);
int iamrx_cc_restrict(iamrx_mf crse, iamrx_mf fine);
int iamrx_cc_prolong_add(iamrx_mf fine, iamrx_mf crse);
int iamrx_face_avgdown(iamrx_mf crse, iamrx_mf fine, int dir);
/* full MLMG solve: amrex::MLMG::solve on MLABecLaplacian (tensor = 1: MLTensorOp, b = eta faces with 1 comp) */
int iamrx_abec_solve(const iamrx_geom* g, double alpha, double beta, iamrx_mf a, iamrx_mf bx, iamrx_mf by, iamrx_mf bz,
                     iamrx_mf phi, iamrx_mf rhs, const int lobc[3], const int hibc[3], double rtol, double atol,
                     const iamrx_mg_opts* o, int tensor, iamrx_mg_stats* st);

/* ---- MAC projection -------------------------------------------------------------------- */
/* MacProj::mlmg_mac_solve (Source/MacProj.cpp:1084-1184; declaration Source/MacProj.H:82-94):
 * b = (1/rhs_scale)/rho_face, rhs = S - div(u_mac), solve, u_mac -= b grad phi.  rho needs 1 filled ghost layer (the face average reads one
 * cell beyond every box face): a density array without ghost cells is an error. */
int iamrx_mlmg_mac_solve(const iamrx_geom* g, iamrx_mf umac_x, iamrx_mf umac_y, iamrx_mf umac_z, iamrx_mf rho, int rho_comp,
                         iamrx_mf S /* may be NULL */, iamrx_mf mac_phi, double rhs_scale, const int lobc[3], const int hibc[3],
                         double mac_tol, double mac_abs_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* the same on an AMR level > 0: cphi = mac_phi_crse[level-1] (the coarse level's MAC phi on its own layout, geometry cgeom) supplies the
 * Dirichlet data of the coarse/fine faces (macproj.setCoarseFineBC(cphi, ratio), Source/MacProj.cpp:1166-1170).  rho needs its ghost cells
 * filled (FillPatch from the coarse level at coarse/fine faces); a density array without ghost cells is an error. */
int iamrx_mlmg_mac_solve_cf(const iamrx_geom* g, iamrx_mf umac_x, iamrx_mf umac_y, iamrx_mf umac_z, iamrx_mf rho, int rho_comp,
                            iamrx_mf S /* may be NULL */, iamrx_mf mac_phi, double rhs_scale, const int lobc[3], const int hibc[3],
                            iamrx_mf crse_phi, const iamrx_geom* cgeom, int ratio, double mac_tol, double mac_abs_tol,
                            const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* MacProj::mac_sync_solve (Source/MacProj.cpp:359-470): coarse-level solve for the correction velocity that removes the mismatch between
 * the coarse MAC velocity and the fine one on the coarse/fine interface.  mac_reg: the interface's register after
 * CrseInit(u_mac_crse, mult = -area_crse) and FineAdd(u_mac_fine, mult = +area_fine / ncycle) (Source/MacProj.cpp:306-346);
 * ucorr_*: coarse face arrays (out), mac_sync_phi: coarse cells, 1 ghost (out); fine: the fine level's layout.  rho_half: 1 filled ghost layer,
 * as for iamrx_mlmg_mac_solve (without ghost cells: an error). */
int iamrx_mac_sync_solve(const iamrx_geom* g, iamrx_fluxreg mac_reg, iamrx_mf rho_half, double dt, iamrx_layout fine, int ratio,
                         iamrx_mf ucorr_x, iamrx_mf ucorr_y, iamrx_mf ucorr_z, iamrx_mf mac_sync_phi, const int lobc[3], const int hibc[3],
                         double mac_sync_tol, double mac_abs_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* MacProj::check_div_cond (Source/MacProj.cpp:792-846): div = div(u_mac) */
int iamrx_mac_divergence(const iamrx_geom* g, iamrx_mf div, iamrx_mf umac_x, iamrx_mf umac_y, iamrx_mf umac_z);

/* ---- Godunov advection ---------------------------------------------------------------- */
/* bcrec: 6 ints per component (lo[3], hi[3]) = amrex::BCRec mathematical BC codes
 * (reference Source/NS_BC.H:7-55). */
/* scheme (last argument of the three entries): the edge-state reconstruction, ns.advection_scheme / godunov_use_ppm
 * (Source/NavierStokesBase.cpp:548-553, 4654-4656): IAMRX_GODUNOV_PLM 0, IAMRX_GODUNOV_PPM 1.  Per call: the library keeps no
 * process-wide advection mode. */
#define IAMRX_GODUNOV_PLM 0
#define IAMRX_GODUNOV_PPM 1
#define IAMRX_BDS 2          /* Bell-Dawson-Shubin edge states in ComputeAofs (the velocity prediction stays Godunov_PLM, as upstream) */
/* Godunov::ExtrapVelToFaces as called from NavierStokesBase::predict_velocity
 * (Source/NavierStokesBase.cpp:4487-4491): vel (3 comps, 3 filled ghosts), force (3 comps, 1 ghost) -> u_mac */
int iamrx_godunov_extrap_vel_to_faces(const iamrx_geom* g, iamrx_mf vel, iamrx_mf force, iamrx_mf umac_x, iamrx_mf umac_y,
                                      iamrx_mf umac_z, double dt, const int* bcrec /* [3][6] */, int use_forces_in_trans, int scheme);
/* the kernel chain of NavierStokesBase::ComputeAofs (Source/NavierStokesBase.cpp:4594-4845):
 * ComputeFluxesOnBoxFromState("Godunov") + ComputeDivergence(mult=-1, area weighted) + ComputeConvectiveTerm,
 * aofs(acomp+n) = -update.  edge_* / flux_* (ncomp face comps) are optional outputs (NULL to skip). */
int iamrx_godunov_compute_aofs(const iamrx_geom* g, iamrx_mf aofs, int acomp, iamrx_mf S, int ncomp, iamrx_mf force, iamrx_mf divu,
                               iamrx_mf umac_x, iamrx_mf umac_y, iamrx_mf umac_z, const int* iconserv, double dt,
                               const int* bcrec /* [ncomp][6] */, int is_velocity, int use_forces_in_trans,
                               iamrx_mf edge_x, iamrx_mf edge_y, iamrx_mf edge_z, iamrx_mf flux_x, iamrx_mf flux_y, iamrx_mf flux_z, int scheme);

/* ---- nodal projection (amrex::MLNodeLaplacian / Hydro::NodalProjector role) ------- */
/* out = rhs - div(sig grad phi) at nodes (rhs == NULL: out = div(sig grad phi)); phi and sig need 1 filled ghost */
int iamrx_nodal_residual(const iamrx_geom* g, iamrx_mf out, iamrx_mf phi, iamrx_mf sig, iamrx_mf rhs);
/* the same on a level that is one box spanning its domain, every direction periodic or between Neumann walls (lobc / hibc: LinOpBC codes):
   the nodes outside the box are read at their periodic / mirror images inside it, so the ghost nodes of phi need no fill (sig: as above);
   norm != NULL: the max norm of out.  The same doubles as iamrx_nodal_residual on filled ghost nodes; an error where the level does not qualify */
int iamrx_nodal_residual_images(const iamrx_geom* g, iamrx_mf out, iamrx_mf phi, iamrx_mf sig, iamrx_mf rhs, const int lobc[3], const int hibc[3],
                                double* norm);
/* one colour (0..7) of the 8-colour Gauss-Seidel sweep */
int iamrx_nodal_gs_color(const iamrx_geom* g, iamrx_mf phi, iamrx_mf rhs, iamrx_mf sig, int color);
/* one full 8-colour Gauss-Seidel sweep incl. its ghost fills.  fused = 0: eight colour passes (8 fills);
 * fused = 1: plane-fused variant, two passes (2 fills), identical arithmetic; needs phi/sig ngrow >= 4, rhs >= 3
 * (rhs ghosts must be filled by the caller) */
int iamrx_nodal_gs_sweep(const iamrx_geom* g, iamrx_mf phi, iamrx_mf rhs, iamrx_mf sig, int fused);
int iamrx_nodal_restrict(iamrx_mf crse, iamrx_mf fine);      /* full weighting; fine needs 1 filled ghost */
/* the same with image reads of the fine level (g: its geometry; conditions as for iamrx_nodal_residual_images): no fill of fine's ghost nodes */
int iamrx_nodal_restrict_images(const iamrx_geom* g, iamrx_mf crse, iamrx_mf fine, const int lobc[3], const int hibc[3]);
int iamrx_nodal_interp_add(iamrx_mf fine, iamrx_mf crse, iamrx_mf sig_fine);
int iamrx_nodal_divu(const iamrx_geom* g, iamrx_mf rhs, iamrx_mf vel, int vcomp);
/* the same with the boundary codes of the non-periodic faces (LinOpBC codes: 102 Neumann wall, 103 inflow -- only the normal velocity
   outside the face counts); periodic directions ignore theirs */
int iamrx_nodal_divu_bc(const iamrx_geom* g, iamrx_mf rhs, iamrx_mf vel, int vcomp, const int lobc[3], const int hibc[3]);
/* MLNodeLaplacian::compGrad as used by NavierStokesBase::computeGradP (Source/NavierStokesBase.cpp:4102-4122) */
int iamrx_nodal_compgrad(const iamrx_geom* g, iamrx_mf gp, iamrx_mf phi);
/* Projection::doMLMGNodalProjection, one level (Source/Projection.cpp:2385-2567; declaration Source/Projection.H:244-254):
 * rhs = div(vel), solve div(sig grad phi) = rhs, vel -= sig grad phi, gp = (increment_gp ? += : =) grad phi */
int iamrx_nodal_projection(const iamrx_geom* g, iamrx_mf vel, int vcomp, iamrx_mf phi, iamrx_mf sig, int sig_comp,
                           const int lobc[3], const int hibc[3], double rel_tol, double abs_tol, const iamrx_mg_opts* o,
                           iamrx_mf gp /* may be NULL */, int increment_gp, iamrx_mg_stats* st);

/* iamrx_abec_solve on an AMR level > 0 (MLLinOp::setCoarseFineBC + setLevelBC as MacProj::mlmg_mac_solve and the Diffusion solves use
 * them on refined levels, Source/MacProj.cpp:1166-1170): the level of phi does not cover the domain; its box faces inside the domain
 * that touch no other box of the level are coarse/fine faces with Dirichlet data taken from crse_phi (the coarse level's solution on its
 * own layout, geometry cgeom; NULL: zero), interpolated along the face (InterpBndryData, third order) and applied with the level's
 * maxorder half a coarse cell behind the face. */
int iamrx_abec_solve_cf(const iamrx_geom* g, double alpha, double beta, iamrx_mf a, iamrx_mf bx, iamrx_mf by, iamrx_mf bz,
                        iamrx_mf phi, iamrx_mf rhs, const int lobc[3], const int hibc[3], iamrx_mf crse_phi, const iamrx_geom* cgeom,
                        int ratio, double rel_tol, double abs_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* the nodal solve alone: div(sig grad phi) = rhs on the level `phi` lives on (MLMG::solve on MLNodeLaplacian, as driven by
 * Hydro::NodalProjector inside Projection::doMLMGNodalProjection, Source/Projection.cpp:2512-2542, and by the sync solves of
 * Projection::MLsyncProject, :457-607).  LinOpBC codes: Neumann (walls, inflow), Dirichlet (outflow).  Nodes on Dirichlet domain
 * faces and -- if the level does not cover the domain (an AMR level > 0) -- on the level's boundary inside the domain are
 * Dirichlet nodes: they keep the incoming phi (MLNodeLaplacian's Dirichlet mask). */
int iamrx_nodal_solve(const iamrx_geom* g, iamrx_mf phi, iamrx_mf rhs, iamrx_mf sig, int sig_comp, const int lobc[3], const int hibc[3],
                      double rel_tol, double abs_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* ---- tensor diffusion (amrex::MLTensorOp role) -------------------------------------- */
/* out = (a*acoef - b div tau(vel)); Diffusion::getTensorViscTerms uses a = 0, b = -1 (Source/Diffusion.cpp:1697-1698).
 * eta_*: face viscosity (1 comp); vel: 3 comps, 1 ghost.
 * lobc/hibc: nbc*3 LinOpBC codes, [n*3+d]; nbc = 1 (all components alike) or 3 (one set per velocity component, the
 * per-component arrays Diffusion::setDomainBC hands to MLTensorOp, Source/Diffusion.cpp:724-731, 1939-2020) */
int iamrx_tensor_apply(const iamrx_geom* g, iamrx_mf out, iamrx_mf vel, double a, double b, iamrx_mf acoef, iamrx_mf eta_x,
                       iamrx_mf eta_y, iamrx_mf eta_z, const int* lobc, const int* hibc, int nbc, int maxorder);
/* implicit Crank-Nicolson solve of Diffusion::diffuse_tensor_velocity (Source/Diffusion.cpp:837-929) */
int iamrx_tensor_solve(const iamrx_geom* g, iamrx_mf soln, iamrx_mf rhs, double a, double b, iamrx_mf acoef, iamrx_mf eta_x,
                       iamrx_mf eta_y, iamrx_mf eta_z, const int* lobc, const int* hibc, int nbc, double tol_rel, double tol_abs,
                       const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* Diffusion::computeExtensiveFluxes on the tensor operator (Source/Diffusion.cpp:1463-1537: MLMG::getFluxes -- the face fluxes of the operator
 * without its b scalar -- times fac x face area), the input of viscflux_reg->FineAdd / CrseInit (:946-954):
 * flux_d(n) = or += fac * area_d * ( -eta_d (4/3 if n == d) du_n/dx_d + cross terms ).  vel: 3 comps, >= 1 ghost cell, as the operator
 * left it after iamrx_tensor_apply(_cf) / iamrx_tensor_solve(_cf) (ghost cells filled with the operator's boundary values). */
int iamrx_tensor_extensive_flux(const iamrx_geom* g, iamrx_mf vel, iamrx_mf eta_x, iamrx_mf eta_y, iamrx_mf eta_z,
                                iamrx_mf flux_x, iamrx_mf flux_y, iamrx_mf flux_z, double fac, int add);
/* the same on a refined level that does not cover the domain (tensorop.setCoarseFineBC(&crsedata, ratio), Source/Diffusion.cpp:733-744,
 * 876-887, 1725-1736; crse_vel == NULL: homogeneous coarse/fine data as in diffuse_tensor_Vsync, :1096-1099).  crse_vel: the coarse
 * level's velocity (3 comps, valid data on its own layout) at the time of the operator. */
int iamrx_tensor_apply_cf(const iamrx_geom* g, iamrx_mf out, iamrx_mf vel, double a, double b, iamrx_mf acoef, iamrx_mf eta_x,
                          iamrx_mf eta_y, iamrx_mf eta_z, const int* lobc, const int* hibc, int nbc, int maxorder,
                          iamrx_mf crse_vel, const iamrx_geom* cgeom, int ratio);
int iamrx_tensor_solve_cf(const iamrx_geom* g, iamrx_mf soln, iamrx_mf rhs, double a, double b, iamrx_mf acoef, iamrx_mf eta_x,
                          iamrx_mf eta_y, iamrx_mf eta_z, const int* lobc, const int* hibc, int nbc, iamrx_mf crse_vel,
                          const iamrx_geom* cgeom, int ratio, double tol_rel, double tol_abs, const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* ---- large-eddy simulation: eddy viscosity on faces (Source/NS_LES.cpp) -------------------------------------------------- */
/* The model loops of NavierStokesBase::calc_mut_LES (Source/NS_LES.cpp:105-222) on the face gradients of MLTensorOp::compVelGrad (:97), and
 * the setVal + Add of NavierStokes::getViscosity (Source/NavierStokes.cpp:2136, 2150), in one launch: mu_d (face d, 1 comp, the layout of vel)
 * = base + mu_t.  vel: cells, velocity in components vcomp .. vcomp + 2, >= 1 ghost layer whose face and edge cells are read AS THE CALLER
 * LEFT THEM.  model: 0 Smagorinsky (:122-136), 1 Sigma (:150-212); Cs: ns.smago_Cs_cst / ns.sigma_Cs_cst; filter width dx[d]. */
int iamrx_les_mut(const iamrx_geom* g, iamrx_mf vel, int vcomp, int model, double Cs, double base, iamrx_mf mu_x, iamrx_mf mu_y, iamrx_mf mu_z);

/* ---- turbulent forcing of forced homogeneous isotropic turbulence (Tutorials/HIT) ----
 * HOST ONLY, no device needed: the mode table of TurbulentForcing::init_turbulent_forcing (Tutorials/HIT/TurbulentForcing_def.H:21-366; seed
 * 111397, generator Tutorials/HIT/depRand.cpp: MT19937, draws in upstream's order, the zero mode's included) for the domain prob_lo .. prob_hi,
 * as the compact list of the modes upstream's two loops write (:142-239 and the 1 <= kz < zstep set :244-341) instead of its 17 arrays of
 * 33^3 entries: kxyz[3 m + d] the integer wavevector, data[17 m + q] the values FTX, TAT, FPX, FPY, FPZ, FAX, FAY, FAZ, FPXX, FPXY, FPXZ, FPYX,
 * FPYY, FPYZ, FPZX, FPZY, FPZZ of mode m (the nine FPab are zero with div_free = 0, where upstream leaves them unwritten).  *M: the number
 * of modes; kxyz / data may be NULL to ask for it, else they hold cap modes.  Refused: Lx != Ly (:34), Lz < Lx (only z may be the long
 * direction), nmodes * zstep > 32 (array_size = 33, Tutorials/HIT/TurbulentForcing_params.H:19). */
int iamrx_host_turb_modes(const double prob_lo[3], const double prob_hi[3], int nmodes, int mode_start, int div_free, int cap, int* M, int* kxyz, double* data);
/* k_turb_force alone: out(ocomp .. ocomp + 2) = the acceleration f(x, time) of the forcing block of NavierStokesBase::getForce
 * (Tutorials/HIT/NS_getForce.cpp:553-686: both forms :570-616 by div_free, every mode of the table -- upstream's two mode loops) on the cells
 * and EVERY ghost cell of the cell-centred array out, at x = prob_lo + (i - dom_lo + 0.5) dx (upstream: from the box's corner, :544-546). */
int iamrx_turb_force(const iamrx_geom* g, int M, const int* kxyz, const double* data, int div_free, double time, iamrx_mf out, int ocomp);
/* NavierStokesBase::calc_mut_LES (Source/NS_LES.cpp:22-225) behind its FillPatch: vel (3 comps, 1 ghost layer) carries the level's boundary
 * data in its ghost cells (what FillPatch left there, :86-88), the tensor operator's boundary step fills them (tensorop.setDomainBC with the
 * per-component codes of LES_setDomainBC, :59-68, 230-285; setLevelBC, :88), then mu_d = mu_t.  lobc / hibc: 9 LinOpBC codes, [n*3+d].
 * maxorder: NS_LES.cpp sets none on its operator; MLLinOp's default is 3 as far as is known.  vel's ghost cells are overwritten. */
int iamrx_calc_mut_les(const iamrx_geom* g, iamrx_mf vel, const int* lobc, const int* hibc, int maxorder, int model, double Cs,
                       iamrx_mf mu_x, iamrx_mf mu_y, iamrx_mf mu_z);
/* the same on a refined level that does not cover the domain (tensorop.setCoarseFineBC(&crsedata, crse_ratio[0]), Source/NS_LES.cpp:76-84);
 * crse_vel: the coarse level's velocity (3 comps, valid data on its own layout) at the same time, NULL: homogeneous */
int iamrx_calc_mut_les_cf(const iamrx_geom* g, iamrx_mf vel, const int* lobc, const int* hibc, int maxorder, int model, double Cs,
                          iamrx_mf mu_x, iamrx_mf mu_y, iamrx_mf mu_z, iamrx_mf crse_vel, const iamrx_geom* cgeom, int ratio);

/* ---- inter-level data motion (first building blocks) ------------------------------------------------------ */
/* amrex::MultiFab::ParallelCopy: dst(valid + dst_ng) <- src(valid + src_ng) wherever they intersect; dst and src may live on
 * different layouts of the same index space (same index type); periodic_geom != NULL adds the periodic images of src */
int iamrx_parallel_copy(iamrx_mf dst, iamrx_mf src, int scomp, int dcomp, int ncomp, int src_ng, int dst_ng, const iamrx_geom* periodic_geom);
/* amrex::average_down / average_down_faces / average_down_nodal (by index type) as called from NavierStokesBase::avgDown_StatePress
 * (Source/NavierStokesBase.cpp:4125-4193): crse(scomp..) <- mean / injection of fine(scomp..); ratio 2 or 4 */
int iamrx_average_down(iamrx_mf fine, iamrx_mf crse, int scomp, int ncomp, int ratio);
/* NavierStokesBase::create_umac_grown on a refined level (Source/NavierStokesBase.cpp:1108-1311): ghost faces of the fine mac velocities
 * (1 ghost layer) from the coarse ones (FaceLinear) or from neighbouring fine boxes, then IAMR's divergence fix of the outer face of every
 * not-covered ghost cell that has exactly one face neighbour inside the fine level; divu: fine cells with >= 1 ghost, or NULL */
int iamrx_create_umac_grown(iamrx_mf umac_fine_x, iamrx_mf umac_fine_y, iamrx_mf umac_fine_z, iamrx_mf umac_crse_x, iamrx_mf umac_crse_y,
                            iamrx_mf umac_crse_z, iamrx_mf divu, const iamrx_geom* cgeom, const iamrx_geom* fgeom, int ratio);
/* amrex::FluxRegister / YAFluxRegister role for one coarse-fine interface (advective registers: Source/NavierStokesBase.cpp:5036-5096,
 * viscous: Source/NavierStokes.cpp:975-992, Source/Diffusion.cpp:940-953; consumer NavierStokes::reflux, Source/NavierStokes.cpp:1736-1838).
 * Fluxes are extensive (area-weighted) as in IAMR.  crse_init: reg = (add: +=) mult*coarse flux; fine_add: reg += mult * sum of the fine
 * fluxes of a coarse face; reflux: S(outside coarse cell) -=/+= scale*reg/volume on the low/high side of a fine box (periodic images incl.) */
int iamrx_fluxreg_create(iamrx_layout fine, iamrx_layout crse, const iamrx_geom* cgeom, int ratio, int ncomp, iamrx_fluxreg* out);
int iamrx_fluxreg_destroy(iamrx_fluxreg fr);
int iamrx_fluxreg_setval(iamrx_fluxreg fr, double v);
int iamrx_fluxreg_crse_init(iamrx_fluxreg fr, iamrx_mf crse_flux, int dir, int scomp, int dcomp, int ncomp, double mult, int add);
int iamrx_fluxreg_fine_add(iamrx_fluxreg fr, iamrx_mf fine_flux, int dir, int scomp, int dcomp, int ncomp, double mult);
int iamrx_fluxreg_reflux(iamrx_fluxreg fr, iamrx_mf S_crse, double volume, double scale, int scomp, int dcomp, int ncomp);
/* AmrLevel::FillPatch of cell-centred StateData on a refined level = amrex::FillPatchTwoLevels with cell_cons_interp
 * (CellConservativeLinear, linear limiting), the interpolater IAMR registers for State_Type / Gradp_Type (Source/NS_setup.cpp:206-394;
 * call sites e.g. Source/NavierStokesBase.cpp:3382-3418, 4399-4435): dst (fine layout, dst ghost width) <- fine data where a fine box
 * (or its periodic image) exists, conservative-linear interpolation of the coarse data elsewhere inside the domain, physical BC
 * outside; both levels are linearly interpolated in time between their old and new data (old may be NULL).
 * bcrec: ncomp x {lo[3], hi[3]} amrex::BCType codes; extdir_*: [n*3+d] ext_dir values (NS_bcfill.H) or NULL */
int iamrx_fillpatch_two_levels(iamrx_mf dst, int dcomp, double time, iamrx_mf fine_old, iamrx_mf fine_new, double t_fine_old, double t_fine_new,
                               iamrx_mf crse_old, iamrx_mf crse_new, double t_crse_old, double t_crse_new, int scomp, int ncomp,
                               const iamrx_geom* cgeom, const iamrx_geom* fgeom, int ratio, const int* bcrec, const double* extdir_lo, const double* extdir_hi);

/* ---- error estimation and grid generation ---------------------------------------------- */
/* "mag_vort" derived quantity (dermgvort, Source/NS_derive.cpp:86-264, non-EB): out(ocomp) = |curl u|, vel needs 1 filled ghost cell */
int iamrx_derive_mag_vort(const iamrx_geom* g, iamrx_mf out, int ocomp, iamrx_mf vel, int vcomp);
/* Derived fields of the velocity-gradient tensor (this library's own; csrc/k_velgrad.hip).  A[n][d] = d u_n / d x_d at the cell centre is
 * the centred difference 0.5 * (u_n(+e_d) - u_n(-e_d)) * (1 / dx_d) over vel(vcomp .. vcomp + 2), which needs at least 1 FILLED ghost
 * layer (only the face neighbours of a cell are read).  out(ocomp + q) = quantity which[q], q < nq <= 10, on the valid cells; the ids:
 *   0 diveru = (A00 + A11) + A22;  1 2 3 vort_x, vort_y, vort_z = A21 - A12, A02 - A20, A10 - A01;
 *   4 enstrophy = 0.5 * (vort_x^2 + vort_y^2 + vort_z^2);  5 strain_rate = sqrt(2 SS);  6 dissipation = mu * (2 SS);
 *   7 q_criterion = 0.5 * (enstrophy - SS) (= -A_ij A_ji / 2);  8 r_invariant = -det(A);  9 helicity = u . vort
 * with SS = A00^2 + A11^2 + A22^2 + 0.5 * ((A01 + A10)^2 + (A02 + A20)^2 + (A12 + A21)^2).  One pass forms all of them.
 * path 0: the marching form (velocity planes in LDS) where the level's largest box holds a full 32 x 8 tile, else the plain form; 1 / 2
 * force the marching / plain form (1 on a level without a full tile is an error).  Both give the same bits.  iamrx_velgrad_path: the
 * form (1 / 2) such a call takes on the layout of vel. */
int iamrx_derive_velgrad(const iamrx_geom* g, iamrx_mf out, int ocomp, int nq, const int* which, iamrx_mf vel, int vcomp, double mu, int path);
int iamrx_velgrad_path(iamrx_mf vel, int path, int* form);
/* measurement aid (tools/bench_velgrad.py): reps times one launch of nq outputs into out(0 .. nq) (split != 0: nq single-output launches)
 * between two events; ms[r] = milliseconds of repeat r.  Nothing is read back. */
int iamrx_velgrad_bench(const iamrx_geom* g, iamrx_mf out, int nq, const int* which, iamrx_mf vel, int vcomp, double mu, int path, int split, int reps, float* ms);
/* one amr.refinement_indicators entry (NavierStokes::error_setup / errorEst, Source/NS_error.cpp:10-145; AMRErrorTag):
 * mode 0 value_greater, 1 value_less, 2 vorticity_greater (value x 2^level), 3 adjacent_difference_greater (field with 1 ghost cell);
 * realbox_lo/hi: in_box_lo / in_box_hi or NULL.  tags: cell-centred, 1 comp; tagged cells are set to 1 */
int iamrx_error_tag(const iamrx_geom* g, iamrx_mf tags, iamrx_mf field, int comp, int mode, double value, int level,
                    const double* realbox_lo, const double* realbox_hi);
/* grid generation from the tags of a level (AmrMesh::MakeNewGrids role: buffer by n_error_buf, Berger-Rigoutsos clustering on the
 * blocking-factor lattice until grid_eff is met, chop to max_grid_size).  Boxes are returned in the index space of the tags
 * (6 ints each: lo, hi); *nboxes in: capacity of boxes, out: number of boxes (error if the capacity is too small). */
int iamrx_cluster_tags(const iamrx_geom* g, iamrx_mf tags, int blocking_factor, int max_grid_size, double grid_eff, int n_error_buf,
                       int* boxes, int* nboxes);
/* The host side of the same on HOST arrays (no device is touched): tags / allowed: one byte per cell of [dom_lo, dom_hi], x fastest; allowed
 * (may be NULL): cells the new level may cover (Amr::regrid(lbase > 0): the proper nesting domain) -- a block of the blocking-factor
 * lattice counts only if all of its cells are allowed.  iamrx_host_erode: the erosion that forms that domain (a cell survives `passes`
 * passes if its 26 neighbours do; periodic images count, nothing constrains beyond a non-periodic face), in place. */
int iamrx_host_cluster_tags(const unsigned char* tags, const int dom_lo[3], const int dom_hi[3], int blocking_factor, int max_grid_size, double grid_eff,
                            int n_error_buf, const unsigned char* allowed, int* boxes, int* nboxes);
int iamrx_host_erode(unsigned char* map, const int n[3], const int periodic[3], int passes);

/* ---- Diffusion operator entries on caller-owned data (the operator-level boundary) -------------------------------------
 * What NavierStokes::scalar_diffusion_update / velocity_diffusion_update / mac_sync hand to the reference's Diffusion class, for a host
 * code that keeps its own state.  All arrays are the caller's; the level's own time step (iamrx_ns_advance) goes through the same code.
 * LinOp BC types (lobc / hibc): as iamrx_abec_* (Diffusion::setDomainBC, Source/Diffusion.cpp:1886-1941); per velocity component for
 * the tensor entries ([n*3+d]).  crse: the coarse level of a refined level, NULL on level 0: its state at the old / new time (valid cells
 * on its own layout, same component numbering as the fine arrays), crse_new NULL = homogeneous coarse/fine data. */
typedef struct iamrx_diffusion_crse { iamrx_mf crse_old, crse_new; const iamrx_geom* cgeom; int ratio; } iamrx_diffusion_crse;
/* Diffusion::diffuse_scalar (Source/Diffusion.cpp:207-599; declaration Source/Diffusion.H:79-104): Crank-Nicolson update of component sigma,
 *   (alpha - theta dt div beta grad) s_new = alpha s* + (1 - theta) dt div beta grad s_old + dt delta_rhs,
 * rho_flag 0: s = S, alpha = 1; 1: alpha = rho_half; 2: s = S / rho, alpha = rho_new, S_new = s rho_new.  S_old / S_new: >= 1 ghost cell
 * FILLED by the caller (FillPatch, Source/Diffusion.cpp:237-239); Rho_old / Rho_new (NULL: S_old / S_new) hold the density in rho_comp;
 * fluxn / fluxnp1 (3 face arrays each, or NULL): the extensive fluxes (1 - theta) area (-beta grad s_old), theta area (-beta grad s_new);
 * delta_rhs (NULL: none); betan / betanp1: 3 face arrays of the diffusivity (betan NULL with theta = 1 or add_old_time_divFlux = 0). */
int iamrx_diffuse_scalar(const iamrx_geom* g, iamrx_mf S_old, iamrx_mf Rho_old, iamrx_mf S_new, iamrx_mf Rho_new, int sigma, int rho_comp, double dt,
                         double be_cn_theta, iamrx_mf rho_half, int rho_flag, const iamrx_mf* fluxn, const iamrx_mf* fluxnp1, iamrx_mf delta_rhs,
                         int rhs_comp, const iamrx_mf* betan, const iamrx_mf* betanp1, const int* lobc, const int* hibc,
                         const iamrx_diffusion_crse* crse, int add_old_time_divFlux, double visc_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* Diffusion::diffuse_tensor_velocity (Source/Diffusion.cpp:617-957; Source/Diffusion.H:117-127): (alpha - theta dt div tau) u_new =
 * alpha u* + (1 - theta) dt div tau(u_old), alpha = rho_half (rho_flag 1) or rho_new with u* weighted by rho_old (rho_flag 3).  U_old / U_new:
 * states with the velocity in components 0..2 and the density in rho_comp, 1 filled ghost cell.  visc_old_term (NULL: evaluate): div tau(u_old).
 * tflux (3 face arrays of 3 components, or NULL).  fill_new (NULL: none): called once U_new's velocity holds rho u*, to refill its ghost
 * cells (the FillPatch of Source/Diffusion.cpp:866). */
int iamrx_diffuse_tensor_velocity(const iamrx_geom* g, iamrx_mf U_old, iamrx_mf U_new, int rho_comp, double dt, double be_cn_theta, iamrx_mf rho_half,
                                  int rho_flag, iamrx_mf visc_old_term, const iamrx_mf* eta_n, const iamrx_mf* eta_np1, const int* lobc, const int* hibc,
                                  const iamrx_diffusion_crse* crse, const iamrx_mf* tflux, double visc_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st,
                                  void (*fill_new)(void* ctx, iamrx_mf U_new), void* ctx);
/* Diffusion::diffuse_Vsync -> diffuse_tensor_Vsync (Source/Diffusion.cpp:960-1178): Vsync (3 components, 1 ghost cell) is replaced by the
 * solution of (alpha - theta dt div tau) V = rho Vsync with homogeneous boundary and coarse/fine data (cgeom NULL: level 0); eta: the face
 * coefficients (upstream passes ones, :1122-1135); bcrec_vel: the BCRecs of the velocity (6 ints per component), ghost cells outside
 * ext_dir faces end up zero (:987-1008); tflux: theta area (-tau), or NULL. */
int iamrx_diffuse_tensor_vsync(const iamrx_geom* g, iamrx_mf Vsync, double dt, double be_cn_theta, iamrx_mf rho_half, int rho_flag, iamrx_mf Rho_old,
                               iamrx_mf Rho_new, int rho_comp, const iamrx_mf* eta, const int* lobc, const int* hibc, const int* bcrec_vel,
                               const iamrx_geom* cgeom, int ratio, const iamrx_mf* tflux, double visc_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* Diffusion::diffuse_Ssync as NavierStokes::mac_sync calls it (Source/NavierStokes.cpp:1590-1640, Source/Diffusion.cpp:1181-1352): component
 * comp of Ssync (a rate) becomes the diffused sync increment, (alpha - theta dt div beta grad) s = dt Ssync (x rho_half for rho_flag 1),
 * Ssync = s (x rho_new for rho_flag 2); flux: theta area (-beta grad s), or NULL. */
int iamrx_diffuse_ssync(const iamrx_geom* g, iamrx_mf Ssync, int comp, double dt, double be_cn_theta, iamrx_mf rho_half, int rho_flag, iamrx_mf Rho_new,
                        int rho_comp, const iamrx_mf* beta, const int* lobc, const int* hibc, const iamrx_geom* cgeom, int ratio, const iamrx_mf* flux,
                        double visc_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* ---- level time step (NavierStokes::advance and the init sequence) ----------------------------------- */
typedef struct iamrx_ns_params {
    double cfl, visc_coef, be_cn_theta, gravity;
    double mac_tol, mac_abs_tol, proj_tol, proj_abs_tol, visc_tol;
    int use_forces_in_trans, do_mom_diff, init_iter, init_vel_iter;
    double init_shrink, change_max, fixed_dt;
    int nscal, verbose;
    double init_dt;              /* ns.init_dt: dt when the state has no velocity/force scale (LidDrivenCavity start) */
    double tracer_diff_coef;     /* ns.scal_diff_coefs[0] (<= 0: tracer not diffusive) */
    int phys_lo[3], phys_hi[3];  /* ns.lo_bc / ns.hi_bc, Source/NS_BC.H: 0 Interior (periodic), 1 Inflow, 2 Outflow, 3 Symmetry, 4 SlipWall, 5 NoSlipWall */
    double wall_vel_lo[9], wall_vel_hi[9];   /* xlo.velocity ... zhi.velocity: [d*3+n] = component n on the lo/hi face of direction d */
    double scal_bc_lo[12], scal_bc_hi[12];   /* xlo.density, xlo.tracer, xlo.tracer2, xlo.temp ... zhi.* (inflow values): [d*4+n], n = the scalar's slot: 0 density, 1 tracer, then tracer2 / temp as present */
    int do_cons_trac;            /* ns.do_cons_trac: the tracer is rho*q, advected conservatively and diffused as div beta grad(S/rho) (Source/NS_setup.cpp:306-310) */
    int do_denminmax, do_scalminmax;   /* ns.do_denminmax / ns.do_scalminmax (Source/NavierStokesBase.cpp:466-467): clip the advected density / scalars to the 27-point min / max of the old data (ConservativeScalMinMax / ConvectiveScalMinMax, :4256-4368) */
    int do_trac2, do_cons_trac2; /* ns.do_trac2 / ns.do_cons_trac2: a second tracer, state component 5 (Source/NavierStokes.cpp:45-46, Source/NS_setup.cpp:312-320) */
    double tracer2_diff_coef;    /* ns.scal_diff_coefs[1] */
    int do_temp;                 /* ns.do_temp: temperature as the last state component (Source/NavierStokes.cpp:47-48; temp_bc, RhoInverse_Laplacian_S) */
    double temp_cond_coef;       /* ns.temp_cond_coef */
    int use_ppm;                 /* ns.advection_scheme: 0 = Godunov_PLM, 1 = Godunov_PPM, 2 = BDS (Source/NavierStokesBase.cpp:548-553, 4654-4656) */
    int avg_interval;            /* ns.avg_interval (Source/NavierStokesBase.cpp:487, Source/NS_average.cpp:8-17): > 0: time averages of the velocity, a sample every avg_interval level-0 steps; 0: off */
    int compute_fluctuations;    /* ns.compute_fluctuations (Source/NavierStokesBase.cpp:488): 1 = also the time integral of the squared velocity fluctuation */
    int sum_interval;            /* ns.sum_interval (Source/NavierStokesBase.cpp:452, 2589-2592): > 0: a hierarchy forms its integrated quantities every sum_interval level-0 steps; <= 0: off */
    int do_LES;                  /* ns.do_LES (Source/NavierStokesBase.cpp:142, 481): 1 = the face viscosity of every viscous apply / solve is visc_coef + mu_t (NavierStokes::getViscosity, Source/NavierStokes.cpp:2139-2152) */
    int LES_model;               /* ns.LES_model (Source/NavierStokesBase.cpp:143, 482): 0 = "Smagorinsky", 1 = "Sigma" */
    double smago_Cs_cst;         /* ns.smago_Cs_cst (Source/NavierStokesBase.cpp:144, 483), default 0.18 */
    double sigma_Cs_cst;         /* ns.sigma_Cs_cst (Source/NavierStokesBase.cpp:145, 484), default 1.5 */
} iamrx_ns_params;
void iamrx_ns_default_params(iamrx_ns_params* p);     /* defaults of Source/NavierStokesBase.cpp:96-170 */
int iamrx_ns_create(const iamrx_geom* g, iamrx_layout l, const iamrx_ns_params* p, const iamrx_mg_opts* o, iamrx_ns* out);
int iamrx_ns_destroy(iamrx_ns ns);
/* The turbulent forcing of Tutorials/HIT (upstream: the compile-time switch USE_TURBULENT_FORCING, Tutorials/HIT/NS_getForce.cpp:205) is a
 * property set on the level after iamrx_ns_create and before iamrx_ns_post_init -- iamrx_ns_params keeps its layout.  on = 1: the level builds
 * the mode table of TurbulentForcing::init_turbulent_forcing (Tutorials/HIT/TurbulentForcing_def.H:21-366) for its domain from turb.nmodes
 * (upstream's default 4), turb.mode_start (0) and turb.div_free_force (1) (:39-49), and getForce adds rho f(x, t) from then on; on = 0: off,
 * the state of a new level (nothing allocated, no launch added, every result what it is without the forcing). */
int iamrx_ns_set_turb_forcing(iamrx_ns ns, int on, int nmodes, int mode_start, int div_free);
/* the same with a caller's table (custom spectra); layout as iamrx_host_turb_modes.  Switches the forcing on. */
int iamrx_ns_set_turb_modes(iamrx_ns ns, int M, const int* kxyz, const double* data, int div_free);
int iamrx_ns_init_taylorgreen(iamrx_ns ns, double vfac, double a, double b, double c, double rho0);  /* Source/prob/prob_init.cpp:509-560 */
/* prob.probtype = 10, RayleighTaylor (Source/prob/prob_init.cpp:407-488) */
int iamrx_ns_init_rayleightaylor(iamrx_ns ns, double rho_1, double rho_2, double tra_1, double tra_2, double pertamp, double interface_width);
int iamrx_ns_init_rest(iamrx_ns ns, double rho0);          /* probtype 1, LidDrivenCavity (Source/prob/prob_init.cpp:102-109) */
int iamrx_ns_post_init(iamrx_ns ns, double stop_time);     /* NavierStokes::post_init (Source/NavierStokes.cpp:1254-1299) */
int iamrx_ns_step(iamrx_ns ns, double* dt_used);           /* computeNewDt + NavierStokes::advance (Source/NavierStokes.cpp:543-691) */
int iamrx_ns_advance(iamrx_ns ns, double dt, double* dt_est);
int iamrx_ns_time(iamrx_ns ns, double* time, double* dt, int* nstep);
/* snapshot COPY (caller destroys it with iamrx_mf_destroy) of a persistent array: 0 S_new, 1 S_old, 2 P_new,
 * 3 P_old, 4 Gp_new, 5 Gp_old, 6..8 u_mac, 9 aofs  (get_new_data/get_old_data role); 10, 11: the last two MAC potentials (the
 * initial-guess history of the MAC solve, part of a checkpoint);
 * 12: the time-average accumulators (the reference's Average_Type, Source/NS_setup.cpp:389-405; only with avg_interval > 0): 6 components,
 * no ghost cells -- 0..2 the time integral of u, v, w, 3..5 the time integral of the squared fluctuation (Source/NS_average.cpp:45-55);
 * 13..15: the face viscosity visc_coef + mu_t (x, y, z faces, 1 comp, no ghost cells) of the OLD state, 16..18: of the new state (which held
 * U*), as the last velocity_diffusion_update formed them (loc_viscn / loc_viscnp1, Source/NavierStokes.cpp:1022-1028); an error with
 * do_LES = 0 or before the first step */
int iamrx_ns_data(iamrx_ns ns, int which, iamrx_mf* out);
/* Derived quantities of the plotfile (derive_lst, Source/NS_setup.cpp:436-449; amr.derive_plot_vars): "energy" = rho |u|^2 / 2 (derkeng,
 * Source/NS_derive.cpp:266-295), "mag_vort" = |curl u| (dermgvort, :86-264, ghost cells by FillPatch), "avg_pressure" = mean of the eight
 * nodes of the cell (deravgpres, :51-80) of the level's new-time data, into component ocomp of the cell-centred out (the level's layout).
 * With avg_interval > 0 also "velocity_average" (der_vel_avg, Source/NS_derive.cpp:11-45; declared Source/NS_setup.cpp:412-431): SIX
 * components from ocomp on, x/y/z_vel_average = accumulator / time_avg and x/y/z_vel_rms = sqrt(accumulator / time_avg_fluct), a zero
 * divisor counting as 1.  Without averages the name is unknown. */
int iamrx_ns_derive(iamrx_ns ns, const char* name, iamrx_mf out, int ocomp);
/* iamrx_ns_derive also knows the ten velocity-gradient names of iamrx_derive_velgrad (ghost cells by FillPatch as for mag_vort;
 * "dissipation" with mu = ns.vel_visc_coef: the molecular part only, also in an LES run).
 * iamrx_ns_derive_fields: out(ocomp + q) = field names[q] for any mix of state names (the plotfile names of iamrx_ns_histogram),
 * single-component derived names and velocity-gradient names; ALL velocity-gradient names of the list share one ghost fill and one launch.
 * iamrx_ns_integrate: out[q] = volume-weighted sum of field names[q] over ALL cells of the level, on all ranks (iamrx_ns_sum_integrated
 * for named fields; the same summation order).  Unknown names are errors that list the known ones. */
int iamrx_ns_derive_fields(iamrx_ns ns, int nnames, const char* const* names, iamrx_mf out, int ocomp);
int iamrx_ns_integrate(iamrx_ns ns, int nnames, const char* const* names, double* out);
/* NavierStokesBase::time_average (Source/NS_average.cpp:19-69) as NavierStokes::post_init (Source/NavierStokes.cpp:1287-1297) and
 * NavierStokesBase::post_timestep (Source/NavierStokesBase.cpp:2630-2634) call it: dt_avg += dt_level; if level0_steps is a multiple of
 * avg_interval the new-time velocity enters the accumulators with weight dt_avg, then time_avg += dt_avg, time_avg_fluct += dt_avg (or
 * = 0 without fluctuations), dt_avg = 0.  A hierarchy (iamrx_amr_post_init / iamrx_amr_coarse_step) makes these calls itself; the caller
 * of iamrx_ns_post_init / iamrx_ns_step makes them for a single level.  No-op with avg_interval = 0. */
int iamrx_ns_time_average(iamrx_ns ns, double dt_level, int level0_steps);
/* NavierStokesBase::time_avg / time_avg_fluct / dt_avg of the level (Source/NavierStokesBase.cpp:2467-2522; checkpointed in
 * <chk>/TimeAverage, :863-888): v[3] = time_avg, time_avg_fluct, dt_avg.  set = 0: read, 1: write.  Error with avg_interval = 0. */
int iamrx_ns_average_state(iamrx_ns ns, int set, double v[3]);
/* One level's part of NavierStokes::sum_integrated_quantities (Source/NavierStokes.cpp:1046-1079): sums[3] = volume-weighted sums of
 * density (MASS), tracer (TRAC) and rho |u|^2 / 2 (KINETIC ENERGY) over ALL cells of the level, on all ranks.  One fused reduction. */
int iamrx_ns_sum_integrated(iamrx_ns ns, double sums[3]);
/* Plane-averaged profiles along one axis (this library's own diagnostic, no upstream counterpart; k_profile.hip; not to be confused with
 * the section timers iamrx_ns_profile / iamrx_amr_profile below).  iamrx_profile_nq: the
 * number of quantities, 14, in this order: 1, u, v, w, rho, c, uu, vv, ww, uv, uw, vw, rho rho, c c (c: the first tracer; new-time
 * state).  iamrx_ns_plane_profile: one level, nothing masked; *nbins = cells of the domain along dir (0, 1, 2), out[q * nbins + b] = mean of
 * quantity q over plane b.  Sums in a fixed order: the same call gives the same bits.  A NaN in a cell reaches the bin of that cell only.
 * Collective on several ranks, every rank receives the result.  Error: dir outside 0..2, nbins_cap smaller than *nbins. */
int iamrx_profile_nq(void);
int iamrx_ns_plane_profile(iamrx_ns ns, int dir, int nbins_cap, double* out, int* nbins);
/* Shell-summed power spectra of a level on a fully periodic domain (this library's own diagnostic; k_spectrum.hip; the role of the
 * plotfile post-processor Tutorials/HIT/README names, settings file derivespect-inputs).  For a cell-centred field f on n = (n_x, n_y,
 * n_z) cells, N = n_x n_y n_z, side lengths L_d:
 *   transform    F(m) = (1/N) sum_x f(x) exp(-2 pi i sum_d m_d x_d / n_d), signed mode numbers m_d in [-n_d/2, n_d/2): an index
 *                j >= n_d/2 means j - n_d;
 *   shell index  L_max = max_d L_d, r_d = L_max / L_d, kappa = sqrt((m_x r_x)^2 + (m_y r_y)^2 + (m_z r_z)^2) (the squares added left to
 *                right in double, no FMA), s = (int)(kappa + 0.5); shell s stands for the wavenumber k_s = s 2 pi / L_max;
 *   shells       *nbins = (int)(kappa(-n/2) + 0.5) + 1 with kappa(-n/2) at m_d = -n_d/2 in every direction: all N modes are counted,
 *                none is cut off at the Nyquist sphere;
 *   power        P_f(s) = sum over the modes of shell s of |F(m)|^2, so that sum_s P_f(s) = mean(f^2) (Parseval);
 *   count        count(s) = number of modes of shell s (exact), sum_s count(s) = N.
 * iamrx_spectrum_nq: the number of columns of the level and hierarchy entries, 4: P_u, P_v, P_w, P_c (c: the first tracer; new-time
 * state); the kinetic-energy spectrum is E = (P_u + P_v + P_w) / 2.  No density weighting.
 * iamrx_mf_spectrum: out[q * nbins + s] = P(s) of component comp + q (q < ncomp) of a caller-owned cell-centred array whose boxes tile
 * the domain of g; ghost cells are never read; count[nbins] may be NULL.  It needs no level object.
 * iamrx_ns_spectrum: the four columns from the level's new-time state.
 * All of them: hand-written batched FFTs staged in LDS, one component at a time through one complex work array of 16 N bytes that
 * returns to the library's arena; sums in a fixed order without floating-point atomics: the same call gives the same bits, and the
 * bits do not depend on how the level is cut into boxes.  Collective on several ranks: every rank writes the cells of its own boxes
 * into a zeroed real array, the arrays are summed through the communicator (exact: a cell has one owner), and EVERY rank then
 * transforms the whole field and receives the same bits -- a gather that does not scale with the number of ranks (the default; the
 * slab-decomposed transform below, SPECTRUM_DIST = 1, gives the same bits from N / R modes per rank).  Error: a direction that is not periodic; an extent that is not a power of two in 4 .. 1024 (the message
 * names it); nbins_cap < *nbins (*nbins is set all the same); boxes that do not cover the domain; more than 2048 shells (side lengths
 * that differ too much for the extents). */
int iamrx_spectrum_nq(void);
int iamrx_mf_spectrum(const iamrx_geom* g, iamrx_mf mf, int comp, int ncomp, int nbins_cap, double* out, long* count, int* nbins);
int iamrx_ns_spectrum(iamrx_ns ns, int nbins_cap, double* out, long* count, int* nbins);
/* measurement aid (tools/bench_spectrum.py): reps times the five passes of one component (pack, x, y, z transform, shell sums) with an
 * event between them; ms[5 * r + p] = milliseconds of pass p in repeat r.  Nothing is read back. */
int iamrx_spectrum_bench(const iamrx_geom* g, iamrx_mf mf, int comp, int reps, float* ms);
/* Plane spectra: ring-summed 2-D spectra along a wall-normal axis, E(k_h; z) (this library's own diagnostic; k_spectrum.hip).  For a
 * cell-centred field f on n = (n_x, n_y, n_z) cells:
 *   axes         dir in {0, 1, 2} is the normal axis.  It is not transformed and may have any boundary type and any extent >= 1.  a < b
 *                are the other two axes; both must be periodic with extents that are powers of two in 4 .. 1024.  M = n_a n_b,
 *                L2 = max(L_a, L_b) (the normal axis does not enter), r_a = L2 / L_a, r_b = L2 / L_b;
 *   transform    for plane p, the cell index along dir counted from the domain's low end:
 *                F_p(m_a, m_b) = (1/M) sum f exp(-2 pi i (m_a x_a / n_a + m_b x_b / n_b)), signed mode numbers as for iamrx_mf_spectrum;
 *   ring index   s = (int)(kappa + 0.5), kappa = sqrt((m_a r_a)^2 + (m_b r_b)^2) (the squares added left to right in double, no FMA);
 *                ring s stands for the horizontal wavenumber k_s = s 2 pi / L2;
 *   rings        *nrings = (int)(kappa(-n_a/2, -n_b/2) + 0.5) + 1, at most 2048;
 *   power        P(p, s) = sum over the modes of ring s of |F_p|^2, so that sum_s P(p, s) = the plane mean of f^2 (Parseval per plane)
 *                and P(p, 0) = the plane mean squared;
 *   count        count(s) = number of modes of ring s: the same for every plane, formed from integers, sum_s count(s) = M;
 *   co-spectrum  C_ab(p, s) = sum over ring s of Re(F_a conj F_b) of two real fields, with P_a and P_b, from ONE transform of Z = a + i b
 *                read with its mirror mode (-m_a, -m_b), which lies in the same plane; sum_s C_ab(p, s) = the plane mean of a b.
 * iamrx_plane_spectrum_nq: the columns of the level and hierarchy entries, 5: P_u, P_v, P_w, P_rho, P_c (c: the first tracer), new-time
 * state; E = (P_u + P_v + P_w) / 2.  No density weighting.
 * iamrx_mf_plane_spectrum: out[(q * nplanes + p) * nrings + s] = P(p, s) of component comp + q (q < ncomp) of a caller-owned cell-centred
 * array whose boxes tile the domain of g; ghost cells are never read (also not those beyond a wall); count[nrings] may be NULL.
 * iamrx_mf_plane_cospectrum: out[(v * nplanes + p) * nrings + s], v = 0, 1, 2: C_ab, then P_a, then P_b, of component acomp of a and
 * bcomp of b, which may be the same array and may have different box layouts.
 * iamrx_ns_plane_spectrum: the five columns from the level's new-time state.  iamrx_amr_plane_spectrum (below): of LEVEL 0.
 * All of them: the dense image, the transform passes (two of the three), the twiddles and the slot sum of iamrx_mf_spectrum; the ring
 * sums are kernels of their own: rows along x that lie in one plane (dir 1, 2) go through a segmented wave scan into LDS bins per
 * plane; for dir 0, where every element of a row lies in another plane, the rows are sorted by ring on the host and lanes along x add
 * them in table order.  No floating-point atomics, a fixed summation order that depends on the shape alone: the same call gives the same
 * bits, whatever the box layout and the number of ranks.  Collective on several ranks: the gather of iamrx_mf_spectrum, every rank
 * receives the same bits.  SPECTRUM_DIST = 1 leaves these calls on the gather, as it leaves the filters (a slab form is not built).
 * Errors, by name and in this order, before anything is allocated: dir outside 0 .. 2; an array that is not cell-centred; a component
 * out of range; a transformed direction that is not periodic (the message names the axis); a transformed extent that is not a power of
 * two in 4 .. 1024; no length along an axis; more than 2048 rings; boxes that do not tile the domain; nplanes_cap < *nplanes or
 * nrings_cap < *nrings (both are set all the same).  The normal direction is never checked for periodicity or for a power of two.
 * Not built: a slab-decomposed form, levels above 0, time averaging, density weighting, a per-plane budget, a chosen subset of planes,
 * two-dimensional runs. */
int iamrx_plane_spectrum_nq(void);
int iamrx_mf_plane_spectrum(const iamrx_geom* g, iamrx_mf mf, int comp, int ncomp, int dir, int nplanes_cap, int nrings_cap, double* out, long* count,
                            int* nplanes, int* nrings);
int iamrx_mf_plane_cospectrum(const iamrx_geom* g, iamrx_mf a, int acomp, iamrx_mf b, int bcomp, int dir, int nplanes_cap, int nrings_cap, double* out,
                              long* count, int* nplanes, int* nrings);
int iamrx_ns_plane_spectrum(iamrx_ns ns, int dir, int nplanes_cap, int nrings_cap, double* out, long* count, int* nplanes, int* nrings);
/* measurement aid (tools/bench_plane_spectrum.py): reps times the four passes of one component (pack, the first and the second transform
 * pass, the ring sums with their slot sum) with an event between them; ms[IAMRX_PLANE_SPECTRUM_BENCH_NP * r + p].  Nothing is read back. */
#define IAMRX_PLANE_SPECTRUM_BENCH_NP 4
int iamrx_plane_spectrum_bench(const iamrx_geom* g, iamrx_mf mf, int comp, int dir, int reps, float* ms);
/* The slab-decomposed transform of the shell-summed diagnostics on several ranks (registry key SPECTRUM_DIST = 1, default 0: the gather
 * above, byte for byte).  With the key at 1, iamrx_mf_spectrum, iamrx_mf_spectrum_k2, iamrx_mf_cospectrum and whatever calls them
 * (the level and hierarchy spectra and budgets) take this path whenever the array is spread over R > 1 ranks: rank r owns the planes
 * k in [r n_z / R, (r + 1) n_z / R) as a complex slab of N / R elements; the boxes are cut by the slabs and the pieces that belong to
 * another rank travel as real doubles; x and y passes on the slab; a transpose to y-slabs, the z pass, a transpose back; the shell sums
 * with the workgroup partition, the wavefront order and the slot order of one rank (a workgroup's rows lie on one rank; the slot arrays
 * are summed exactly: a slot has one owner, the others hold +0), so the bytes of the result are those of one rank; a packed pair
 * receives its mirror planes in at most two messages.  No rank holds an N-sized array.  Eligible: R a power of two that divides n_y and
 * n_z; with the key at 1 an ineligible call is an error that names the reason, on every rank, before anything is sent.  One rank or a
 * replicated layout: the key has no effect.  The way back from mode space, the a-priori LES analysis and the structure functions stay on
 * the gather.
 * iamrx_host_spectrum_slab_plan: host only, no device.  The scatter plan of rank `rank` of `nranks` for the boxes lo_hi[6 b] .. (lo,
 * then hi) with owners owner[b] on the domain of g.  *eligible = 1, or 0 with the reason in reason[reason_cap] (may be NULL).
 * rows[10 * n + .]: kind (0 the piece stays on the rank, 1 sent, 2 received), peer (the own rank for kind 0), global box index, piece
 * lo[3], hi[3], offset of the piece (doubles) in the buffer to or from that peer (kind 0: -1).  A piece is a box cut by a slab; the
 * pieces of a buffer follow one another in box order, x fastest inside a piece, so that p's rows to q are q's rows from p.  *nrows is
 * the number of rows, of which min(*nrows, max_rows) are written (rows may be NULL).
 * iamrx_spectrum_slab_info: the last shell-sum call on this rank.  out[0] path (0 local or gather, 1 slab), [1] ranks, [2] complex
 * elements of the largest work image allocated, [3] elements transformed per pass, [4] doubles sent and [5] doubles received through
 * the communicator's exchange, summed over the call (the all-reduce of the gather and of the slot arrays is not an exchange),
 * [6] transforms done.
 * iamrx_spectrum_slab_bench (tools/bench_spectrum_slab.py): the kernels ONE rank of nranks runs for one plain transform, on arena
 * buffers of the per-rank shapes with the exchanges left out: ms[IAMRX_SPECTRUM_SLAB_BENCH_NP * r + p], p = 0 scatter, 1 x, 2 y, 3 pack,
 * 4 unpack, 5 z, 6 pack, 7 unpack, 8 shell sums, 9 k_spec_expand over N / nranks elements (the streaming yardstick).  One process, no
 * communicator needed. */
#define IAMRX_SPECTRUM_SLAB_BENCH_NP 10
int iamrx_host_spectrum_slab_plan(const iamrx_geom* g, int nboxes, const int* lo_hi, const int* owner, int rank, int nranks, int* eligible,
                                  char* reason, size_t reason_cap, int max_rows, long* rows, int* nrows);
int iamrx_spectrum_slab_info(long out[7]);
int iamrx_spectrum_slab_bench(const iamrx_geom* g, int nranks, int reps, float* ms);
/* Co-spectra and the spectral kinetic-energy budget dE(k)/dt = T(k) - D(k) + F(k) of a fully periodic level (this library's own
 * diagnostic; k_spectrum.hip, k_convect.hip).  The transform F, the signed mode numbers, kappa, the shell index s, *nbins and count are
 * those of iamrx_mf_spectrum, and so are the restrictions and the errors, checked in the same order (*nbins is set before the capacity
 * error).  N: the number of cells.
 *   co-spectrum    C_ab(s) = sum over the modes of shell s of Re(F_a(m) conj(F_b(m))) of two cell-centred fields a, b, so that
 *                  sum_s C_ab(s) = mean(a b) (Parseval) and C_aa = P_a;
 *   k^2 weighting  W_f(s) = sum over the modes of shell s of k(m)^2 |F_f(m)|^2, k(m)^2 = (2 pi / L_max)^2 ((m_x r_x)^2 + (m_y r_y)^2 +
 *                  (m_z r_z)^2), the squares added in the order the shell index uses.  This is the SPECTRAL |grad f|^2, not the one of the
 *                  solver's discrete operators;
 *   nonlinear term in skew-symmetric centred form: with delta_d f(x) = (f(x + e_d) - f(x - e_d)) (0.5 / dx_d) and i = 0, 1, 2,
 *                  N_i(x) = 0.5 sum_d [ u_d(x) delta_d u_i(x) + delta_d(u_d u_i)(x) ]  (built without FMA contraction).  Only the six face
 *                  neighbours of a cell are read.  sum_x u_i N_i = 0 identically on a periodic grid (summation by parts), so the
 *                  transfer below sums to zero over the shells up to rounding;
 *   budget         of the new-time state, no density weighting (as for E): E(s) = (P_u + P_v + P_w) / 2, T(s) = -(C_{u N_0} + C_{v N_1}
 *                  + C_{w N_2}), D(s) = visc_coef (W_u + W_v + W_w) (the molecular part only, also in an LES run, as "dissipation"),
 *                  F(s) = C_{u f_0} + C_{v f_1} + C_{w f_2} with f the acceleration of the turbulent forcing at the level's time as
 *                  iamrx_turb_force evaluates it, exactly zero with the forcing off.  The flux Pi(s) = -(T(0) + ... + T(s)) is left to
 *                  the caller (iamr_amd/budget.py adds left to right).
 * iamrx_mf_cospectrum: out[0 .. nbins) = C_ab, then P_a, then P_b, of component acomp of a and bcomp of b: caller-owned cell-centred
 * arrays that each tile the domain of g; they may be the same array and may have different box layouts; count may be NULL.  The pair goes
 * through ONE transform as Z = a + i b; the shell sums read every mode with its mirror mode -m, index ((n_x - i) % n_x, (n_y - j) % n_y,
 * (n_z - k) % n_z): Re(F_a conj F_b)(m) = Im(Z(m) Z(-m)) / 2, |F_a|^2 = |Z(m) + conj Z(-m)|^2 / 4, |F_b|^2 = |Z(m) - conj Z(-m)|^2 / 4.
 * Sums in a fixed order, no floating-point atomics: the same call gives the same bits, whatever the box layouts.  C_ab and C_ba agree
 * within rounding, not to the bit (the packed fields differ).
 * iamrx_mf_spectrum_k2: out[q * nbins + s] = W(s) of component comp + q, one plain transform each.
 * iamrx_convective_term: out(ocomp + i) = N_i of vel(vcomp .. vcomp + 2) on the valid cells; out and vel on one layout, vel with at
 * least one FILLED ghost layer.  Walls are allowed: the stencil is pointwise and a ghost cell's value is differenced like any other.
 * iamrx_budget_nq: the columns of the level and hierarchy entries, 4: E, T, D, F.  iamrx_ns_spectral_budget: out[q * nbins + s]; the
 * velocity is FillPatched once with one ghost layer, N (and f) are formed into arrays that return to the arena, three packed transforms
 * (u_i, N_i) give E, T and D, three more (u_i, f_i) give F when the forcing is on.  Collective on several ranks as the spectra are (a
 * gather, or the slab-decomposed transform with SPECTRUM_DIST = 1).  Not built: density weighting, levels above 0, time averaging, the
 * eddy-viscosity part of D. */
int iamrx_mf_cospectrum(const iamrx_geom* g, iamrx_mf a, int acomp, iamrx_mf b, int bcomp, int nbins_cap, double* out, long* count, int* nbins);
int iamrx_mf_spectrum_k2(const iamrx_geom* g, iamrx_mf mf, int comp, int ncomp, int nbins_cap, double* out, int* nbins);
int iamrx_convective_term(const iamrx_geom* g, iamrx_mf out, int ocomp, iamrx_mf vel, int vcomp);
int iamrx_budget_nq(void);
int iamrx_ns_spectral_budget(iamrx_ns ns, int nbins_cap, double* out, long* count, int* nbins);
/* measurement aids (tools/bench_budget.py): the five passes of one packed pair (pack, x, y, z transform, shell sums with the mirror read),
 * ms[5 * r + p] as iamrx_spectrum_bench; one launch of the nonlinear term into out(0 .. 2), ms[r].  Nothing is read back. */
int iamrx_cospectrum_bench(const iamrx_geom* g, iamrx_mf a, int acomp, iamrx_mf b, int bcomp, int reps, float* ms);
int iamrx_convective_bench(const iamrx_geom* g, iamrx_mf out, iamrx_mf vel, int vcomp, int reps, float* ms);
/* The way back from mode space: spectral filters, the solenoidal projection and a synthetic isotropic field (this library's own; the role
 * of the off-line generator Tutorials/HIT/README names; k_spectrum.hip).  The transform F, the signed mode numbers m_d, r_d, kappa, the
 * shell index s and *nbins are those of iamrx_mf_spectrum, and so are the restrictions and the errors, checked in the same order.
 * Physical wavenumber k_d = 2 pi m_d / L_d = k0 m_d r_d with k0 = 2 pi / L_max, so |k| = k0 kappa.  dx_d = L_d / n_d.
 *   inverse        f = conj(FFT(conj(N F))) / N with the passes and twiddle tables of the forward transform: the conjugation and the 1 / N
 *                  are folded into the mode-space pass in front, and the unpack takes real parts (the last conjugation is free);
 *   filter         F(m) <- G(m) F(m); the cut-off kc is given in units of k0 and Delta = pi / (k0 kc):
 *                    kind 0  identity  G = 1 (the round trip)
 *                    kind 1  sharp     G = 1 where kappa^2 <= kc^2 (kappa^2 formed exactly as the shell index forms it), otherwise 0
 *                    kind 2  Gaussian  G = exp(-|k|^2 Delta^2 / 24) = prod_d exp(-(pi m_d r_d / kc)^2 / 24)
 *                    kind 3  box       G = prod_d sinc(k_d Delta / 2) = prod_d sinc(pi m_d r_d / (2 kc)), sinc(x) = sin(x) / x, sinc(0) = 1
 *                  Kinds 2 and 3 are products of one factor per axis; the factors come from per-axis tables the host makes in extended
 *                  precision (as the twiddles), multiplied as (g_x g_y) g_z;
 *   projection     on three components at once, u(m) <- u(m) - q (q . u(m)) / |q|^2 with q . u = (q_x u_x + q_y u_y) + q_z u_z and
 *                  |q|^2 = (q_x^2 + q_y^2) + q_z^2; modes with |q|^2 = 0 are left alone:
 *                    wavenumber 0  exact    q_d = k_d: the continuous field becomes divergence-free
 *                    wavenumber 1  centred  q_d = sin(2 pi m_d / n_d) / dx_d: the centred difference (f(x + e_d) - f(x - e_d)) / (2 dx_d)
 *                                           of "diveru" and of the nonlinear term becomes divergence-free
 *                  Nyquist rule: q_d = 0 for m_d = -n_d / 2 in both forms (the sine gives it by itself; without it the exact form is not
 *                  Hermitian there and the real part taken at the end would break the projection in those modes);
 *   shell scale    F(m) <- a[s(m)] F(m);
 *   noise          depends on (seed, component c counted from 0 at `comp`, global cell index o = i + n_x (j + n_y k)) alone, in 64-bit
 *                  wrapping arithmetic: mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                  z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31);  h = mix(mix(seed ^ ((c + 1) * 0x9E3779B97F4A7C15)) + o);
 *                  value = ((h >> 12) + 0.5) 2^-52 - 0.5: uniform in (-1/2, 1/2), every step exact in double, the same for every box
 *                  layout and number of ranks.
 * iamrx_mf_noise: the valid cells of components comp .. comp + ncomp - 1 of a cell-centred array whose boxes tile the domain of g (g
 * gives n_x, n_y; periodicity and extents are not restricted).
 * iamrx_mf_filter: dst(dcomp + q) = filtered src(scomp + q), q < ncomp, one component at a time; dst and src may be the same array or
 * live on different layouts of the same domain; ghost cells are neither read nor written.  Error besides those of the spectra: kind
 * outside 0 .. 3, kc not > 0 (any kind).
 * iamrx_mf_solenoidal: dst(dcomp .. dcomp + 2) = the solenoidal part of src(scomp .. scomp + 2); three work arrays.  Error: wavenumber
 * outside 0 .. 1.
 * iamrx_mf_synthesize: dst(dcomp .. dcomp + 2) = a random solenoidal field whose kinetic-energy spectrum E(s) = (P_u + P_v + P_w) / 2 is
 * E_target[0 .. nbins): noise(seed) for c = 0, 1, 2, three forward transforms, the projection, E_now(s) through the shell sums of the
 * spectra, a(s) = sqrt(E_target(s) / E_now(s)) (a = 0 where E_now(s) = 0 or s = 0), the shell scale, three inverse transforms, the
 * unpack.  nbins must be that of g.  Error: a negative or non-finite E_target(s); E_target(s) > 0 in a shell where E_now(s) = 0 (s = 0
 * is never asked for: the field has no mean); in that case dst is not written.
 * All of them: one 16 N byte work array per component in flight from the arena, no floating-point atomics, sums in the fixed order of
 * the spectra: the same call gives the same bits, whatever the box layouts.  Collective on several ranks as the spectra are: a gather,
 * every rank transforms the whole field, the unpack writes the rank's own boxes.  On any error dst is untouched. */
int iamrx_mf_noise(const iamrx_geom* g, iamrx_mf mf, int comp, int ncomp, unsigned long long seed);
int iamrx_mf_filter(const iamrx_geom* g, iamrx_mf dst, int dcomp, iamrx_mf src, int scomp, int ncomp, int kind, double kc);
int iamrx_mf_solenoidal(const iamrx_geom* g, iamrx_mf dst, int dcomp, iamrx_mf src, int scomp, int wavenumber);
int iamrx_mf_synthesize(const iamrx_geom* g, iamrx_mf dst, int dcomp, unsigned long long seed, int nbins, const double* E_target, int wavenumber);
/* measurement aid (tools/bench_filter.py): iamrx_specop_bench_np() = 17 passes with an event between them, ms[17 * r + p]: one filter of
 * src(scomp) into dst(0) -- 0 pack, 1 2 3 forward x y z, 4 multiplier, 5 6 7 inverse x y z, 8 unpack -- then one synthesis into
 * dst(0 .. 2) -- 9 noise, 10 nine forward passes, 11 projection, 12 shell sums and a(s), 13 shell scale, 14 nine inverse passes,
 * 15 unpack -- and 16 one dense_pack of src(scomp) alone, the yardstick of the streaming passes.  Nothing is read back. */
int iamrx_specop_bench_np(void);
int iamrx_specop_bench(const iamrx_geom* g, iamrx_mf dst, iamrx_mf src, int scomp, int kind, double kc, int wavenumber, int reps, float* ms);
/* A-priori LES analysis: the subgrid stress of a filtered field, the energy it drains from the large scales and what the Smagorinsky
 * operators of the closure (k_les.hip) make of the same filtered field (this library's own diagnostic; k_sgs.hip, driver in
 * k_spectrum.hip).  The level is cell-centred and triply periodic with power-of-two extents 4 .. 1024: the conditions and the errors
 * of the spectra.  u = vel(vcomp .. vcomp + 2); the filter is (kind, kc) of iamrx_mf_filter, written ~ below; Delta = pi / (k0 kc) =
 * L_max / (2 kc); N = the cells of the level; <.> = the sum over all cells divided once by N.  Per cell:
 *   filtered velocity   u~_i: the filtered u_i;
 *   filtered product    (u_i u_j)~ for i <= j: the filtered cell-wise product, formed in double (one rounding) before the filter;
 *   stress              tau_ij = (u_i u_j)~ - u~_i u~_j (one product, one difference);
 *   subgrid energy      k_sgs = 0.5 ((tau_xx + tau_yy) + tau_zz);
 *   deviatoric stress   taud_ij = tau_ij - delta_ij ((2 / 3) k_sgs);
 *   filtered gradient   A[n][d] = 0.5 (u~_n(x + e_d) - u~_n(x - e_d)) (1 / dx_d) with periodic wrap: the centred difference of
 *                       iamrx_derive_velgrad (the same bits as (u~_n(x + e_d) - u~_n(x - e_d)) (0.5 / dx_d));
 *   filtered strain     S_ij = 0.5 (A[i][j] + A[j][i]); with s_ij = A[i][j] + A[j][i] for i < j,
 *                       SS = A00^2 + A11^2 + A22^2 + 0.5 (s_01^2 + s_02^2 + s_12^2), each sum left to right as iamrx_derive_velgrad's,
 *                       |S|^2 = 2 SS and |S| = sqrt(2 SS): "strain_rate" of u~;
 *   inter-scale flux    Pi = -tau_ij S_ij, all nine terms (the six off-diagonal ones in pairs, tau_ij s_ij = 2 tau_ij S_ij):
 *                       Pi = -(((tau_xx A00 + tau_yy A11) + tau_zz A22) + ((tau_xy s_01 + tau_xz s_02) + tau_yz s_12));
 *   eddy viscosity at C_s = 1, two operators:
 *                       m = 0 "strain"    D_0 = Delta^2 |S|, the textbook Smagorinsky form;
 *                       m = 1 "gradient"  D_1 = Delta^2 sqrt(2 A_ij A_ij) = les_model<0>(A, Delta^2) of the closure, the expression
 *                                         ns.smago_Cs_cst multiplies in this code (one function, les_model.h, for both);
 *                       model stress M^m_ij = -2 D_m S_ij, model flux P_m = D_m |S|^2 = D_m (2 SS);
 *   taud_ij taud_ij   = ((taud_xx^2 + taud_yy^2) + taud_zz^2) + 2 ((tau_xy^2 + tau_xz^2) + tau_yz^2);
 *   taud_ij S_ij      = ((taud_xx A00 + taud_yy A11) + taud_zz A22) + ((tau_xy s_01 + tau_xz s_02) + tau_yz s_12).
 * sgs statistics: iamrx_sgs_nstat() = 16 doubles, index name value (m = 0: strain, m = 1: gradient at 6 + 5 m .. 10 + 5 m)
 *    0  Pi            <Pi>
 *    1  Pi2           <Pi^2>
 *    2  Pi_neg        <min(Pi, 0)>
 *    3  k_sgs         <k_sgs>
 *    4  S2            <|S|^2>
 *    5  taud2         <taud_ij taud_ij>
 *    6  P_strain      <P_0>
 *    7  P2_strain     <P_0^2>
 *    8  PiP_strain    <Pi P_0>
 *    9  MM_strain     <D_0^2 |S|^2>           (= <M^0 M^0> / 2)
 *   10  LM_strain     <D_0 taud_ij S_ij>      (= -<taud M^0> / 2)
 *   11  P_gradient    <P_1>
 *   12  P2_gradient   <P_1^2>
 *   13  PiP_gradient  <Pi P_1>
 *   14  MM_gradient   <D_1^2 |S|^2>
 *   15  LM_gradient   <D_1 taud_ij S_ij>
 * and two exact integers counts[2] = {N, the cells with Pi < 0} (counts may be null).  The sums run in a fixed order -- per thread in
 * index order over a grid that depends on N alone, across a wavefront by a butterfly in which both partners add the same two numbers
 * in the same order, per workgroup into its own slots, the slots in slot order -- without floating-point atomics: the same call gives
 * the same bits for every box layout and number of ranks.
 * sgs fields: by id, any subset in any order, field which[q] into component ocomp + q of the valid cells of `out`
 *    0  tau_xx
 *    1  tau_xy
 *    2  tau_xz
 *    3  tau_yy
 *    4  tau_yz
 *    5  tau_zz
 *    6  k_sgs
 *    7  sgs_flux          Pi
 *    8  filtered_strain   |S|
 *    9  smag_flux         P_0
 * `out` is a caller-owned cell-centred array on any layout that tiles the domain (not necessarily that of vel); ghost cells are
 * neither read nor written, of vel or of out.  out = NULL with nout = 0: statistics only, no field is stored or unpacked.
 * One component per transform, the filter's own sequence and per-field accuracy; nine 16 N byte images from the arena for the length
 * of the call, returned on every path.  Errors: those of the spectra (not cell-centred, component range, boxes that do not tile, not
 * periodic, extents) and of the filter (kind, kc); a field id outside 0 .. 9; nout > 0 with a null out or which; out aliasing vel; null
 * stats.  On any error out is untouched.  Collective on several ranks exactly as iamrx_mf_filter; every rank receives the same bits.
 * iamrx_ns_sgs: the new-time velocity of the level's state (no ghost cell is needed).
 * Not built: the Sigma operator (its acos of a clamped argument is ill-conditioned; a derived parity bound is a piece of work of its
 * own), density weighting, levels above 0, a distributed transform, pair-packed transforms, time averaging. */
int iamrx_sgs_nstat(void);
int iamrx_mf_sgs(const iamrx_geom* g, iamrx_mf vel, int vcomp, int kind, double kc, iamrx_mf out, int ocomp, int nout, const int* which,
                 double* stats, long* counts);
int iamrx_ns_sgs(iamrx_ns ns, int kind, double kc, iamrx_mf out, int ocomp, int nout, const int* which, double* stats, long* counts);
/* measurement aid (tools/bench_sgs.py): iamrx_sgs_bench_np() = 6 passes with an event between them, ms[6 * r + p]: 0 the three plain
 * packs, 1 the six product packs, 2 the 54 transform passes and nine multipliers, 3 k_sgs_point with its finish kernel, 4 the unpack of
 * the nout fields into out(0 .. nout - 1), 5 one dense_pack of vel(vcomp) alone.  Nothing is read back. */
int iamrx_sgs_bench_np(void);
int iamrx_sgs_bench(const iamrx_geom* g, iamrx_mf out, iamrx_mf vel, int vcomp, int kind, double kc, int nout, const int* which, int reps, float* ms);
/* Structure functions and two-point correlations along the axes (this library's own diagnostic, no upstream counterpart; k_strfn.hip).
 * Unlike the spectra they are defined with walls and on extents that are not powers of two.  For a cell-centred component f on a level
 * whose boxes tile the domain, n = (n_x, n_y, n_z) cells, N = n_x n_y n_z, an axis d and an integer separation r in cells:
 *   pairs        periodic axis: x and x + r e_d with wrap-around, for all N cells x: count(d, r) = N, also for r = n_d / 2, where every
 *                unordered pair is met twice.  Non-periodic axis: only pairs inside the domain, no wrap, no ghost cell:
 *                count(d, r) = (n_d - r) N / n_d;
 *   separations  r = 0 .. rmax_d.  rmax_d = -1: the largest allowed value, n_d / 2 on a periodic axis and n_d - 1 otherwise;
 *                rmax_d = 0: the axis is skipped, nothing is launched for it; a larger request is an error that names the axis;
 *   columns      with delta = f(x + r e_d) - f(x), every column a sum over the pairs divided by count(d, r):
 *                column 0: R = <f(x) f(x + r e_d)>; columns 1 .. pmax: <delta^p>, signed; then one column for each odd p <= pmax:
 *                <|delta|^p>.  1 <= pmax <= 8, ncol = 1 + pmax + ceil(pmax / 2) (iamrx_strfn_ncol; -1 for a pmax out of range).
 *                Powers by successive multiplication in double;
 *   mean         mean[c] = <f_c> over the N cells;
 *   count        exact integers from the formula above (no kernel forms them);
 *   extents      n_d <= 1024 on an axis that is not skipped; any extent, a power of two or not (an extent of 1 has rmax_d = 0).
 * iamrx_strfn_nq: the components of the level and hierarchy entries, 4: u, v, w and the first tracer of the new-time state.
 * iamrx_mf_strfn: components comp + c (c < ncomp) of a caller-owned cell-centred array; out[((d * ncomp + c) * ncol + col) * rcap + r],
 * zero for r > rmax_d; count[d * rcap + r] (zero for r > rmax_d) and mean[ncomp] may be NULL; rcap >= 1 + the largest resolved rmax_d.
 * iamrx_ns_strfn: the four components of the level's new-time state (ncomp = 4 in the indexing above).
 * All of them: the valid cells are packed into one dense real array of 8 N bytes from the library's arena (ghost cells are never
 * read), one component at a time; one launch per axis stages pencils in LDS and forms every separation from there; sums in a fixed
 * order without floating-point atomics: the same call gives the same bits, for any way the level is cut into boxes and any number of
 * ranks.  Collective on several ranks: the field is gathered on every rank as for the spectra (it does not scale with the ranks).
 * Error, by name: an array that is not cell-centred; a bad component range; boxes that do not tile the domain; pmax outside 1 .. 8;
 * rmax_d below -1 or beyond the axis's limit; rcap too small; an extent above 1024 on an axis that is not skipped. */
int iamrx_strfn_ncol(int pmax);
int iamrx_strfn_nq(void);
int iamrx_mf_strfn(const iamrx_geom* g, iamrx_mf mf, int comp, int ncomp, int pmax, const int rmax[3], int rcap, double* out, long long* count, double* mean);
int iamrx_ns_strfn(iamrx_ns ns, int pmax, const int rmax[3], int rcap, double* out, long long* count, double* mean);
/* measurement aid (tools/bench_strfn.py): reps times the four passes of one component (pack, then the pair launch of x, y and z, each
 * with its finish kernel) with an event between them; ms[4 * r + p] = milliseconds of pass p in repeat r.  Nothing is read back. */
int iamrx_strfn_bench(const iamrx_geom* g, iamrx_mf mf, int comp, int pmax, const int rmax[3], int reps, float* ms);
/* Histograms of cell-centred fields: the counts a probability density function is made of (this library's own diagnostic, no upstream
 * counterpart; k_hist.hip; iamr_amd/pdf.py forms the PDFs).  The counts are integers and exact: the same bits on every call, for every
 * way the level is cut into boxes and for every number of ranks.  The binning rule, per column:
 *   bounds       lo < hi, both finite, hi - lo finite; 1 <= nbins <= 4096; inv = nbins / (hi - lo), formed once in double;
 *   a value v    NaN -> the slot `nan`; v < lo -> the slot `below`; v > hi -> the slot `above`;
 *                otherwise bin b = min((int)((v - lo) * inv), nbins - 1): a subtraction, then a multiplication (never fused), then a
 *                truncation, so that numpy reproduces it exactly;
 *   therefore    v == hi lies in the last bin; a value on an interior edge lies in the upper bin; -0.0 with lo = 0 lies in bin 0;
 *                -inf / +inf go to below / above;
 *   slots        counts[q * (nbins + 3) + s] (64-bit integers) for column q: s < nbins the bins, then below, above, nan;
 *   cells        the valid cells of the boxes; ghost cells are never read; a cell with cov != 0 (cov: a cell-centred array on the same
 *                layout, may be NULL) is skipped, not multiplied by zero: what it holds reaches no slot; every counted cell adds the
 *                integer `weight` (>= 1; 1 for a single level).
 * iamrx_mf_histogram: columns q < ncomp = components comp + q of a caller-owned cell-centred array, all with nbins bins, lo[ncomp], hi[ncomp].
 * iamrx_mf_histogram2: the joint histogram of components compx and compy, the same rule per axis with lo[2], hi[2], nbins[2] and
 * nbins[0] * nbins[1] <= 16384: counts[bx * nby + by], followed by ONE slot `outside` for a cell that is NaN or out of range on either axis
 * (nbx * nby + 1 slots).
 * iamrx_ns_histogram / iamrx_ns_histogram2: fields of a level by name, weight 1, nothing masked.  The names: the state components by
 * their plotfile names x_velocity, y_velocity, z_velocity, density, tracer (tracer2 / temp when the run has them) and the single-component
 * derived quantities energy, mag_vort, avg_pressure and the ten velocity-gradient names (formed as iamrx_ns_derive forms them, into a scratch array that returns to the
 * library's arena); new-time data.
 * All of them are collective on several ranks: every rank counts its own boxes, the slots are summed through the communicator (which
 * carries doubles: integers below 2^53 are summed exactly; a slot or a total that reaches 2^53 is an error) and every rank receives the
 * result.  Error: hi <= lo, a bound that is not finite, nbins outside its range, an unknown name (the message lists the known ones), a
 * coverage array on another layout, components outside the array. */
int iamrx_mf_histogram(iamrx_mf mf, int comp, int ncomp, iamrx_mf cov /* may be NULL */, const double* lo, const double* hi, int nbins, long long weight, long long* counts);
int iamrx_mf_histogram2(iamrx_mf mf, int compx, int compy, iamrx_mf cov /* may be NULL */, const double lo[2], const double hi[2], const int nbins[2], long long weight, long long* counts);
int iamrx_ns_histogram(iamrx_ns ns, int nnames, const char* const* names, const double* lo, const double* hi, int nbins, long long* counts);
int iamrx_ns_histogram2(iamrx_ns ns, const char* namex, const char* namey, const double lo[2], const double hi[2], const int nbins[2], long long* counts);
/* measurement aid (tools/bench_hist.py): reps times the launches of one iamrx_mf_histogram (nby = 0) or iamrx_mf_histogram2 (ncomp = 2,
 * nbins x nby bins) between two events; ms[r] = milliseconds of repeat r.  Nothing is read back. */
int iamrx_hist_bench(iamrx_mf mf, int comp, int ncomp, iamrx_mf cov /* may be NULL */, const double* lo, const double* hi, int nbins, int nby, int reps, float* ms);

/* overwrite state (0,1), pressure (2,3) or grad p (4,5) with src (same layout and ngrow; ncomp at most the array's: the leading
 * components are set): the role of NavierStokes::initData for caller-supplied initial data (Source/NavierStokes.cpp:318-420).
 * The state arrays hold u v w density tracer [tracer2] [temp], and with ns.do_temp two more components, divu and dsdt (the
 * reference's Divu_Type / Dsdt_Type), which the library computes. */
int iamrx_ns_set_data(iamrx_ns ns, int which, iamrx_mf src);      /* which: 0..5, 10, 11, 12 */
/* checkpoint / restart of one level (AmrLevel::checkPoint / NavierStokesBase::restart role, Source/NavierStokesBase.cpp:856-897,
 * 2706-2727): what outlives a time step besides the arrays of iamrx_ns_data.  state[16] = time, dt, nstep, State_Type new / old time,
 * Press_Type new interval [2], old interval [2], dt of the last MAC solve, two history flags, dt estimate of the last advance,
 * stop_time, 2 unused.  set = 0: read; set = 1: write (after the arrays have been set with iamrx_ns_set_data; the level then continues
 * as if it had taken the steps itself -- no post_init). */
int iamrx_ns_restart_state(iamrx_ns ns, int set, double state[16]);
int iamrx_ns_stats(iamrx_ns ns, iamrx_mg_stats* mac, iamrx_mg_stats* nodal, iamrx_mg_stats* visc);
/* per-section wall time accumulation (ms): predict, mac, advect, update, viscous, nodal; enable=1 inserts stream syncs (2: and resets).
 * enable=3: no syncs; HIP events on the launch stream around every 8th k_nodal_gs4 launch of the level's own (finest) MG level until the
 * next call, which returns their total duration (ms) in sections_ms[6] and their number in sections_ms[7] */
int iamrx_ns_profile(iamrx_ns ns, int enable, double sections_ms[8]);

/* ---- zero-copy view of caller-owned device memory ----------------------------------------------------------------------
 * AMReX keeps its FABs in device memory on GPU builds (The_Arena); with the same Array4 layout on both sides a MultiFab needs no
 * copy at the seam: dev_ptrs[li] = FArrayBox::dataPtr() of the li-th LOCAL box (allocated region = valid box converted to `type`
 * and grown by ngrow).  The library never frees, moves or reallocates the memory; destroy the handle with iamrx_mf_destroy. */
int iamrx_mf_alias(iamrx_layout l, const int type[3], int ncomp, int ngrow, double* const* dev_ptrs, iamrx_mf* out);

/* Projection::level_project on a level that covers the domain (Source/Projection.cpp:166-450; declaration Source/Projection.H:53-75), the
 * call NavierStokesBase::level_projector makes (Source/NavierStokesBase.cpp:1894-1924): P_new = 0; U_new /= dt; U_new += Gp_old/rho_half;
 * sigma = 1/rho_half; doMLMGNodalProjection (Gp_new = grad phi, P_new = phi); U_new *= dt.  In place, like the reference.
 * U_new: velocity at comps vcomp..vcomp+2, 1 ghost cell (inflow data in the ghost cells of inflow faces, in U/dt units);
 * lobc/hibc: LinOpBC codes of Projection.cpp:2432-2464 (102 Neumann, 101 outflow, 103 inflow). */
int iamrx_level_project(const iamrx_geom* g, double dt, iamrx_mf U_new, int vcomp, iamrx_mf P_new, iamrx_mf Gp_old, iamrx_mf Gp_new,
                        iamrx_mf rho_half, const int lobc[3], const int hibc[3], double proj_tol, double proj_abs_tol,
                        const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* SyncRegister (Source/SyncRegister.H:40-49, Source/SyncRegister.cpp): nodal register on the faces of the coarsened fine boxes.
 * crse_init: SyncRegister::CrseInit(Sync_resid_crse, crse_geom, mult) (:306-318); fine_add: FineAdd(Sync_resid_fine, crse_geom, mult)
 * (:350-607; the fine residual needs no ghost nodes here); init_rhs: InitRHS(rhs, geom, phys_bc) (:47-304; rhs: nodal, coarse layout).
 * phys_lo/hi: PhysBCType codes of ns.lo_bc / ns.hi_bc (outflow faces are zeroed in InitRHS). */
int iamrx_syncreg_create(iamrx_layout fine, iamrx_layout crse, const iamrx_geom* cgeom, const iamrx_geom* fgeom, int ratio,
                         const int phys_lo[3], const int phys_hi[3], iamrx_syncreg* out);
int iamrx_syncreg_destroy(iamrx_syncreg r);
int iamrx_syncreg_crse_init(iamrx_syncreg r, iamrx_mf sync_resid_crse, double mult);
int iamrx_syncreg_fine_add(iamrx_syncreg r, iamrx_mf sync_resid_fine, double mult);
int iamrx_syncreg_init_rhs(iamrx_syncreg r, iamrx_mf rhs);
/* Projection::MLsyncProject (Source/Projection.cpp:457-607; declaration Source/Projection.H:99-118) on caller-owned data: the two-level sync
 * projection NavierStokesBase::level_sync drives (Source/NavierStokesBase.cpp:1927-2044).  A level of the solve: its geometry and boxes,
 * the nodal LinOp BC (lobc / hibc: periodic / Neumann / Dirichlet at outflow / inflow, Source/Projection.cpp:2432-2464), the ratio to the
 * next coarser level, gp (or NULL): the Gradp array that accumulates grad(phi).
 * Vsync (coarse, 3 components, 1 ghost cell) and V_corr (fine: Vsync interpolated with iamrx_sync_interp) are projected with
 * sigma = 1 / rho_crse, 1 / rho_fine and the right-hand side of rhs_sync_reg (SyncRegister::InitRHS); phi_crse / phi_fine (nodal, 1 ghost
 * cell) return the pressure correction, which is also added to pres_crse / pres_fine; vel_* (velocity at vcomp_*) += dt * the projected
 * increments.  crse_sync_reg (NULL on level 0): the register of the interface BELOW the coarse level, which receives the residual of the
 * composite solution on that level's boundary when crse_iteration == crse_dt_ratio (SyncRegister::CompAdd, Source/SyncRegister.cpp:302-348). */
typedef struct iamrx_proj_level { const iamrx_geom* geom; iamrx_layout layout; int lobc[3], hibc[3]; int ratio; iamrx_mf gp; } iamrx_proj_level;
int iamrx_mlsync_project(const iamrx_proj_level* crse, const iamrx_proj_level* fine, iamrx_mf pres_crse, iamrx_mf vel_crse, int vcomp_crse, iamrx_mf pres_fine,
                         iamrx_mf vel_fine, int vcomp_fine, iamrx_mf rho_crse, iamrx_mf rho_fine, iamrx_mf Vsync, iamrx_mf V_corr, iamrx_mf phi_crse,
                         iamrx_mf phi_fine, iamrx_syncreg rhs_sync_reg, iamrx_syncreg crse_sync_reg, double dt, int crse_iteration, int crse_dt_ratio,
                         double sync_tol, double abs_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* NavierStokesBase::SyncInterp with cell_cons_interp (Source/NavierStokesBase.cpp:3071-3276): fine_dst(dcomp..) = conservative-linear
 * interpolant of crse_sync(scomp..) on every cell of the fine level; the caller applies `increment` / dt_clev (:3215-3262) */
int iamrx_sync_interp(iamrx_mf fine_dst, int dcomp, iamrx_mf crse_sync, int scomp, int ncomp, const iamrx_geom* cgeom, const iamrx_geom* fgeom,
                      int ratio, const int* bcrec /* [ncomp][6] */);
/* NavierStokesBase::ComputeAofs with is_sync = true as MacProj::mac_sync_compute calls it (Source/MacProj.cpp:700-731,
 * Source/NavierStokesBase.cpp:4681-4683, 4777, 4826-4832): edge states traced with u_mac, fluxes = edge * Ucorr * area,
 * sync(acomp..) -= -div(F)/vol; flux_* (optional) receive the fluxes for the flux registers */
int iamrx_godunov_compute_aofs_sync(const iamrx_geom* g, iamrx_mf sync, int acomp, iamrx_mf S, int ncomp, iamrx_mf force, iamrx_mf divu,
                                    iamrx_mf umac_x, iamrx_mf umac_y, iamrx_mf umac_z, iamrx_mf ucorr_x, iamrx_mf ucorr_y, iamrx_mf ucorr_z,
                                    const int* iconserv, double dt, const int* bcrec, int is_velocity, int use_forces_in_trans,
                                    iamrx_mf flux_x, iamrx_mf flux_y, iamrx_mf flux_z, int scheme);

/* SyncRegister::CompAdd (Source/SyncRegister.H:45, SyncRegister.cpp:302-348): sync_resid_fine (nodal, on the fine side of r's interface; the
 * residual a sync projection of the levels above leaves on that level) is zeroed on the nodes of the boxes of `finer` (the next finer level,
 * ratio finer_ratio to the residual's level whose geometry is fgeom; periodic images included: upstream's Pgrids) and added like FineAdd
 * with `mult`.  The residual array is modified, as upstream's is. */
int iamrx_syncreg_comp_add(iamrx_syncreg r, iamrx_mf sync_resid_fine, const iamrx_geom* fgeom, iamrx_layout finer, int finer_ratio, double mult);
/* MacProj::mac_sync_compute, the form NavierStokes::mac_sync calls (Source/MacProj.H:60-75, MacProj.cpp:488-731), on caller-owned arrays of one
 * level: the velocity forcing gravity * rho (z) + visc_vel - gradp, divided by rho unless do_mom_diff (:598-640), then ComputeAofs with
 * is_sync = true for the three velocities (Vsync -= update) and for the nscal scalars starting with the density (Ssync -= update), both
 * traced with umac and fluxed with ucorr.  S_vel (3 comps; rho u under do_mom_diff, :536-553) / S_scal (nscal comps): the state at
 * prev_time with 3 filled ghost cells; visc_vel (3) / tforce_scal (nscal, the scalars' forcing as :641-683 assemble it) / gradp (3) / divu
 * (1): 1 ghost cell, visc_vel / tforce_scal / divu may be NULL (zero).  fluxv_* (3 comps) / fluxs_* (nscal comps), optional: the fluxes
 * for the caller's advective registers (CrseInit / FineAdd with the sync sign, Source/NavierStokesBase.cpp:5083-5096; the FineAdd of ucorr
 * to the mac register, MacProj.cpp:707-727, is the caller's as well: iamrx_fluxreg_fineadd). */
int iamrx_mac_sync_compute(const iamrx_geom* g, iamrx_mf ucorr_x, iamrx_mf ucorr_y, iamrx_mf ucorr_z, iamrx_mf Vsync, iamrx_mf Ssync, iamrx_mf S_vel,
                           iamrx_mf S_scal, int nscal, iamrx_mf visc_vel, iamrx_mf tforce_scal, iamrx_mf gradp, iamrx_mf divu, iamrx_mf umac_x,
                           iamrx_mf umac_y, iamrx_mf umac_z, const int* iconserv_scal, int do_mom_diff, double gravity, double dt, const int* bcrec_vel,
                           const int* bcrec_scal, int use_forces_in_trans, int scheme, iamrx_mf fluxv_x, iamrx_mf fluxv_y, iamrx_mf fluxv_z,
                           iamrx_mf fluxs_x, iamrx_mf fluxs_y, iamrx_mf fluxs_z);
/* MacProj::mac_sync_compute, the form with the half-time edge states handed in (Source/MacProj.H:77-94, MacProj.cpp:733-786; one component):
 * flux = edge(edge_comp) * ucorr * area, Sync(sync_indx) -= -div(flux) / vol; flux_* (optional, 1 comp) return the fluxes */
int iamrx_mac_sync_compute_edge(const iamrx_geom* g, iamrx_mf ucorr_x, iamrx_mf ucorr_y, iamrx_mf ucorr_z, iamrx_mf Sync, int sync_indx, iamrx_mf edge_x,
                                iamrx_mf edge_y, iamrx_mf edge_z, int edge_comp, iamrx_mf flux_x, iamrx_mf flux_y, iamrx_mf flux_z);
/* Projection::initialVelocityProject (Source/Projection.H:116-121, Projection.cpp:615-838) on caller-owned arrays of the levels
 * levels[0 .. nlev-1] (coarsest first): pres[l] (nodal, 1 ghost) is zeroed and returns phi; vel[l] (velocity at vcomp[l], 1 ghost cell with
 * the inflow data) is projected on the composite grid, div(sigma grad phi) = div(vel) - <divu>, vel -= sigma grad phi, sigma = 1
 * (rho == NULL: rho_wgt_vel_proj = 0) or 1 / rho[l](rho_comp[l]); divu / divu_comp: the constraint of a variable-divergence run or NULL;
 * levels[l].gp (optional) receives grad phi. */
int iamrx_initial_velocity_project(int nlev, const iamrx_proj_level* levels, const iamrx_mf* vel, const int* vcomp, const iamrx_mf* pres, const iamrx_mf* rho,
                                   const int* rho_comp, const iamrx_mf* divu, const int* divu_comp, double proj_tol, double proj_abs_tol,
                                   const iamrx_mg_opts* o, iamrx_mg_stats* st);
/* Projection::initialSyncProject (Source/Projection.H:123-134, Projection.cpp:970-1185) on caller-owned arrays: vel_new <- (vel_new - vel_old) / dt,
 * sigma = 1 / rho_half, velocities averaged down, rhcc = -(divu_new - divu_old) / dt (NULL: none), composite projection that ACCUMULATES
 * grad phi in levels[l].gp; phi[l] (the caller's old-time pressure array, zeroed first) returns the correction, which is also added to
 * pres_new[l] (may be NULL).  vel_new keeps the projected acceleration (upstream resets the state afterwards, NavierStokesBase::resetState). */
int iamrx_initial_sync_project(int nlev, const iamrx_proj_level* levels, const iamrx_mf* vel_new, const int* vcomp, const iamrx_mf* vel_old, const iamrx_mf* phi,
                               const iamrx_mf* pres_new, const iamrx_mf* rho_half, const iamrx_mf* divu_new, const iamrx_mf* divu_old, const int* divu_comp,
                               double dt, double proj_tol, double proj_abs_tol, const iamrx_mg_opts* o, iamrx_mg_stats* st);

/* ---- multi-level time step ------------------------------------------------------------------------------------
 * One coarse time step of a hierarchy of levels with subcycling = amrex::Amr::coarseTimeStep -> timeStep(level): advance(level),
 * ncycle x timeStep(level+1), NavierStokesBase::post_timestep(level) (Source/NavierStokesBase.cpp:2546-2636):
 *   NavierStokes::reflux (Source/NavierStokes.cpp:1736-1838), avgDown (:1845-1873), mac_sync (:1438-1730) with
 *   MacProj::mac_sync_solve / mac_sync_compute (Source/MacProj.cpp:359-731), NavierStokesBase::level_sync (Source/NavierStokesBase.cpp:1927-2044)
 *   with Projection::MLsyncProject (Source/Projection.cpp:457-607), SyncRegister (Source/SyncRegister.cpp), SyncInterp (:3071-3276);
 * and NavierStokes::post_init for all levels (initialVelocityProject, initialPressureProject, init_iter x {advance, initialSyncProject},
 * Source/NavierStokes.cpp:1254-1432, Source/Projection.cpp:615-1185).
 * layouts[l]: the boxes of level l in the index space of that level (level 0 must cover g0's domain; finer levels must be aligned to
 * the refinement ratio and properly nested).  ratio: 2.  The level handles returned by iamrx_amr_level are borrowed: use them with
 * iamrx_ns_data / iamrx_ns_set_data / iamrx_ns_time / iamrx_ns_stats, do not destroy them. */
int iamrx_amr_create(const iamrx_geom* g0, int nlev, const iamrx_layout* layouts, int ratio, const iamrx_ns_params* p, const iamrx_mg_opts* o, iamrx_amr* out);
int iamrx_amr_destroy(iamrx_amr a);
/* iamrx_ns_set_turb_forcing / iamrx_ns_set_turb_modes for a hierarchy: the table is built once from the level-0 domain and shared by every level
 * (levels made by later regrids included) */
int iamrx_amr_set_turb_forcing(iamrx_amr a, int on, int nmodes, int mode_start, int div_free);
int iamrx_amr_set_turb_modes(iamrx_amr a, int M, const int* kxyz, const double* data, int div_free);
/* ---- regridding: Amr::regrid from level 0 with IAMR's error estimation (amr.refinement_indicators, Source/NS_error.cpp:10-145) and
 * NavierStokesBase::init(AmrLevel&) / init() for the data of the new levels (Source/NavierStokesBase.cpp:1713-1806).
 * comp: state component 0..4 (velocity, density, tracer) or -1 = mag_vort; mode: 0 value_greater, 1 value_less, 2 vorticity_greater
 * (x 2^level), 3 adjacent_difference_greater; value[nvalue]: per level (the last one repeats); tags only on levels < max_level;
 * has_box: in_box_lo / in_box_hi.  regrid_int > 0: iamrx_amr_coarse_step regrids at the start of every regrid_int-th coarse step.
 * After a regrid (check iamrx_amr_nlevels / iamrx_amr_level_boxes, or simply re-fetch after every coarse step) the level handles of
 * iamrx_amr_level must be fetched again: handles given out before stay allocated until iamrx_amr_destroy but are retired -- every
 * iamrx_ns_* call on them returns an error ("stale level handle") instead of touching a freed level. */
typedef struct iamrx_tag_rule { int comp, mode, nvalue, max_level, has_box; double value[8]; double box_lo[3], box_hi[3]; } iamrx_tag_rule;
int iamrx_amr_set_regrid(iamrx_amr a, int max_level, int regrid_int, int blocking_factor, int max_grid_size, double grid_eff, int n_error_buf,
                         int nrules, const iamrx_tag_rule* rules);
/* The regrids of the last iamrx_amr_coarse_step.  As in Amr::timeStep, at the start of every step of every level each level i from there up
 * whose own step count since the grids above it were last rebuilt has reached regrid_int rebuilds the levels above it (regrid(i)), so a
 * regrid can start above level 0 and fall inside a coarse step.  Event e: the base level (the levels up to it kept their grids), the
 * time, the number of rebuilt levels and, level by level from lbase + 1, their boxes (nboxes[l], then 6 ints per box; boxes NULL: sizes
 * only).  For drivers that mirror the hierarchy elsewhere. */
int iamrx_amr_regrid_log_count(iamrx_amr a, int* nevents);
int iamrx_amr_regrid_log_event(iamrx_amr a, int event, int* lbase, double* time, int* nlevels, int* nboxes /* [8] */, int* boxes);
/* amr.compute_new_dt_on_regrid (default 0): 1 = after a regrid from level 0 that changed the grids the time steps are recomputed with
 * NavierStokesBase::computeNewDt(post_regrid_flag = 1) (Source/NavierStokesBase.cpp:971-982), as Amr::timeStep does; 0 = levels that
 * existed keep their dt, new levels start with dt_level[l-1] / n_cycle[l]. */
int iamrx_amr_set_compute_new_dt_on_regrid(iamrx_amr a, int on);
/* NavierStokesBase::manual_tags_placement (Source/NavierStokesBase.cpp:2112-2215; ns.do_refine_outflow = 0, ns.do_derefine_outflow = 1,
 * ns.Nbuf_outflow = 1 are the defaults here as upstream): with an outflow face, either refine the whole layer next to it once it holds a
 * tag, or keep Nbuf_outflow level-0 cells (rounded up to the blocking factor, grown level by level) next to it unrefined.  Call after
 * iamrx_amr_set_regrid. */
int iamrx_amr_set_outflow_tagging(iamrx_amr a, int do_refine_outflow, int do_derefine_outflow, int nbuf_outflow);
int iamrx_amr_regrid(iamrx_amr a, int* changed);
/* install given grids of levels 1 .. nfine_levels (boxes in each level's own index space, 6 ints per box, level by level) and fill them */
int iamrx_amr_install_grids(iamrx_amr a, int nfine_levels, const int* nboxes, const int* boxes, int* changed);
int iamrx_amr_nlevels(iamrx_amr a, int* nlev);
/* a handle of the layout level `lev` currently lives on (release it with iamrx_layout_destroy): for containers that exchange data with the level */
int iamrx_amr_level_layout(iamrx_amr a, int lev, iamrx_layout* out);
int iamrx_amr_level_boxes(iamrx_amr a, int lev, int* nboxes, int* boxes /* NULL: query the count */);
int iamrx_amr_level(iamrx_amr a, int lev, iamrx_ns* out);
int iamrx_amr_post_init(iamrx_amr a, double stop_time);      /* S_new of every level must hold the initial data (iamrx_ns_set_data) */
/* Amr::checkPoint / Amr::restart role for the hierarchy: dt_level, dt_min, n_cycle per level, counters = {level_steps, level_count},
 * stop_time.  set = 0: read, 1: write (instead of iamrx_amr_post_init, after every level has been restored). */
int iamrx_amr_restart_state(iamrx_amr a, int set, double* dt_level, double* dt_min, int* n_cycle, int counters[2], double* stop_time);
/* Amr::level_count of every level (the steps of level i since the last regrid that rebuilt it; Amr::timeStep regrids from level i when it
 * reaches regrid_int), n = amr.max_level + 1 entries as Amr::checkPoint writes them.  set = 0: read (0 beyond the levels that exist) */
int iamrx_amr_level_counts(iamrx_amr a, int set, int* counts, int n);
/* amr.restart takes stop_time from the inputs file, not from the checkpoint (Amr::restart re-reads it): the level's own copy, which
 * clips its time step (NavierStokesBase::computeNewDt, Source/NavierStokesBase.cpp:1011-1023) */
int iamrx_ns_set_stop_time(iamrx_ns ns, double stop_time);
int iamrx_amr_coarse_step(iamrx_amr a, double* dt0);         /* dt0: the level-0 time step used */
int iamrx_amr_time(iamrx_amr a, double* time, double* dt_levels /* [nlev] or NULL */);
/* NavierStokes::sum_integrated_quantities (Source/NavierStokes.cpp:1046-1079; amrex volumeWeightedSum): composite MASS, TRAC and KINETIC
 * ENERGY of the hierarchy now -- every level over the cells the next finer level does not cover, weighted with the cell volume, the levels
 * added coarsest first.  iamrx_amr_last_sum: what the hierarchy itself computed with sum_interval > 0, after post_init
 * (Source/NavierStokes.cpp:1284-1285; *step = 0) and in level 0's post_timestep of every sum_interval-th level-0 step
 * (Source/NavierStokesBase.cpp:2589-2592; *step = that step count); *step = -1: nothing yet. */
int iamrx_amr_sum_integrated(iamrx_amr a, double sums[3]);
/* the same for named fields (the names of iamrx_ns_integrate): out[q] = composite volume-weighted sum of names[q], every level with its
 * own cell volume over the cells the next finer level does not cover, the levels added coarsest first, summed over the ranks */
int iamrx_amr_integrate(iamrx_amr a, int nnames, const char* const* names, double* out);
int iamrx_amr_last_sum(iamrx_amr a, int* step, double* time /* or NULL */, double sums[3]);
/* Plane-averaged profile of the composite state along dir (see iamrx_ns_plane_profile for the quantities and the layout of out).  The bins are
 * the slabs, one cell thick, of the index space of level bin_level (0 .. finest): *nbins = cells of level 0 along dir times 2^bin_level.
 * The value of a bin is the volume-weighted mean over the cells that no finer level covers and that meet the slab: a cell of a level at
 * or above bin_level lies in one bin, a coarser cell counts in each of the 2^(bin_level - l) bins it spans with that share of its volume
 * (piecewise constant; the sum over the bins stays conservative).  Quantity 0, the uncovered volume fraction of the slab, is 1.  Covered
 * cells are skipped, not multiplied by zero.  Error: dir outside 0..2, bin_level outside 0..finest, nbins_cap too small. */
int iamrx_amr_plane_profile(iamrx_amr a, int dir, int bin_level, int nbins_cap, double* out, int* nbins);
/* The spectra of iamrx_ns_spectrum on LEVEL 0 of the hierarchy: after avgDown its covered cells hold the average of the finer data (the
 * role of finestLevel = 0 in derivespect-inputs).  Spectra on finer levels and composite spectra are not built. */
int iamrx_amr_spectrum(iamrx_amr a, int nbins_cap, double* out, long* count, int* nbins);
/* The plane spectra of iamrx_ns_plane_spectrum on LEVEL 0 of the hierarchy, exactly as iamrx_amr_spectrum takes its level. */
int iamrx_amr_plane_spectrum(iamrx_amr a, int dir, int nplanes_cap, int nrings_cap, double* out, long* count, int* nplanes, int* nrings);
/* The budget of iamrx_ns_spectral_budget on LEVEL 0 of the hierarchy, exactly as iamrx_amr_spectrum takes its level. */
int iamrx_amr_spectral_budget(iamrx_amr a, int nbins_cap, double* out, long* count, int* nbins);
/* The a-priori LES analysis of iamrx_ns_sgs on LEVEL 0 of the hierarchy, exactly as iamrx_amr_spectrum takes its level. */
int iamrx_amr_sgs(iamrx_amr a, int kind, double kc, iamrx_mf out, int ocomp, int nout, const int* which, double* stats, long* counts);
/* The structure functions of iamrx_ns_strfn on LEVEL 0 of the hierarchy, exactly as iamrx_amr_spectrum takes its level. */
int iamrx_amr_strfn(iamrx_amr a, int pmax, const int rmax[3], int rcap, double* out, long long* count, double* mean);
/* Composite histograms of the hierarchy (the rule, the names and the layout of counts: iamrx_mf_histogram / iamrx_ns_histogram above).  Level l
 * counts the cells that level l + 1 does not cover, each with the weight 8^(finest - l): the slots are in units of finest-level cell
 * volumes, and all slots of a column together sum to cells(level 0) * 8^finest.  Covered cells are skipped, not multiplied by zero.
 * Error: as above, and a hierarchy for which that total does not stay below 2^53. */
int iamrx_amr_histogram(iamrx_amr a, int nnames, const char* const* names, const double* lo, const double* hi, int nbins, long long* counts);
int iamrx_amr_histogram2(iamrx_amr a, const char* namex, const char* namey, const double lo[2], const double hi[2], const int nbins[2], long long* counts);
/* the pieces of NavierStokesBase::post_timestep(lev) one by one (lev < finest), for a caller that drives the loop itself:
 * NavierStokes::reflux, avgDown, mac_sync (= MacProj::mac_sync_solve + mac_sync_compute + the state update and SyncInterp),
 * NavierStokesBase::level_sync (= SyncInterp + Projection::MLsyncProject) */
int iamrx_amr_reflux(iamrx_amr a, int lev);
int iamrx_amr_avg_down(iamrx_amr a, int lev);
int iamrx_amr_mac_sync(iamrx_amr a, int lev);
int iamrx_amr_level_sync(iamrx_amr a, int lev);
int iamrx_amr_sync_stats(iamrx_amr a, iamrx_mg_stats* sync_project, iamrx_mg_stats* mac_sync);
/* section profile of the coarse steps (synchronising; measurement aid like iamrx_ns_profile).  Reads the accumulated times first, then
 * enable: 1 = reset and start, 0 = stop, -1 = leave as is.  sections_ms[16]: [0] reflux, [1] avgDown, [2] mac_sync_solve, [3] rest of mac_sync
 * (mac_sync_compute, viscous / scalar sync solves, SyncInterp), [4] level_sync (MLsyncProject), [5] regrid, [8 + l] advance of level l;
 * level_sections_ms[8 * l + i]: the sections of iamrx_ns_profile of level l (may be NULL). */
int iamrx_amr_profile(iamrx_amr a, int enable, double sections_ms[16], double level_sections_ms[]);

/* ---- tracer particles (k_particles.hip): the role of AMReX's AmrTracerParticleContainer as IAMR uses it (reference
 * Source/NavierStokesBase.cpp:198-222, 3751-4057; Source/NavierStokes.cpp:672-677).  AMReX is not part of the reference tree, so the
 * container's arithmetic is UNPINNED; tests/particles_numpy.py restates what is implemented.
 * A container lives on nlev levels (coarsest first, level 0 covers the domain, refined by `ratio`); particles are device resident and kept
 * grouped by (level, box).  Attached to a level or a hierarchy (iamrx_ns_set_particles / iamrx_amr_set_particles) it is REBOUND to that
 * object's own boxes, and again after every regrid; box indices then refer to those (merged) boxes.
 *
 * Several ranks (one process per GPU): every rank holds the particles that lie in the boxes it owns; a redistribution sends the others to
 * their owners (one allreduce and one exchange through the installed communicator, whatever the number of particles).
 *   COLLECTIVE -- every rank calls them, also a rank with no particle and no box, with the same level arguments; an error that one rank
 *   finds (a particle that cannot be placed, refused arguments) is returned on every rank and every rank's container stays as it was:
 *     create, add, redistribute, derive_count with which = 1, count_global, iamrx_ns_set_particles / iamrx_amr_set_particles, and the
 *     steps, regrids and derives of the object the container is attached to.
 *   LOCAL -- this rank's particles only, in this rank's storage order; box indices are local ones:
 *     count (per_level, total), read, set_positions, advect, derive_count with which = 0, set_next_id, set_fixed_dir, sample,
 *     set_timestamp, timestamp.
 *   GLOBAL VALUES, equal on every rank: *removed of add and redistribute and *removed_total (sums over the ranks), *next_id, and what
 *     count_global returns.
 * On one rank nothing is collective and every call is what it was. */
int iamrx_particles_create(int nlev, const iamrx_geom* geoms /* [nlev] */, const iamrx_layout* layouts /* [nlev] */, int ratio, iamrx_particles* out);
int iamrx_particles_destroy(iamrx_particles pc);
/* n particles from host arrays: xyz[3 n]; r[3 n], ids[n], cpus[n] may be NULL (zeros; ids from the container's counter, which starts at 1; 0).
 * They are placed by a redistribution over all levels; *removed (may be NULL): how many of all particles fell outside a non-periodic domain.
 * Several ranks: every rank passes its own list, possibly none (n = 0, NULL arrays); the particles go to the owners of their boxes.  Without
 * ids the new ids continue the counter in rank order (rank q's follow rank q - 1's: all positions on rank 0 and none elsewhere give the ids
 * of a one-rank run); with ids the counter becomes the largest id + 1 over the ranks. */
int iamrx_particles_add(iamrx_particles pc, long n, const double* xyz, const double* r, const int* ids, const int* cpus, long* removed);
/* count[l] (l < nlev of the container; may be NULL), *total, *next_id, *removed_total (any may be NULL) */
int iamrx_particles_count(iamrx_particles pc, long* per_level, long* total, int* next_id, long* removed_total);
/* collective: the counts summed over the ranks; per_level[l] (l < nlev; may be NULL), *total (may be NULL) */
int iamrx_particles_count_global(iamrx_particles pc, long* per_level, long* total);
/* (several ranks: to be given the same value on every rank) */
int iamrx_particles_set_next_id(iamrx_particles pc, int next_id);
/* a coordinate the particles never move in (the slab direction of a lifted two-dimensional run); -1: none */
int iamrx_particles_set_fixed_dir(iamrx_particles pc, int dir);
/* every particle to host arrays of `total` entries (any may be NULL): xyz[3 n], r[3 n], id, cpu, level, box; in storage order */
int iamrx_particles_read(iamrx_particles pc, double* xyz, double* r, int* id, int* cpu, int* level, int* box);
/* overwrite the positions from xyz[3 n], in the storage order iamrx_particles_read reports (a caller that moves the particles itself);
 * follow with iamrx_particles_redistribute */
int iamrx_particles_set_positions(iamrx_particles pc, const double* xyz);
/* TracerParticleContainer::AdvectWithUmac for the particles of level lev on caller-owned face arrays (on the level's boxes, the ghost faces
 * the stencils reach filled): pass 1  r = x, x += dt/2 v(x);  pass 2  x = r + dt v(x), r = v;  v_d trilinear in u_mac[d].  Nothing moves between
 * boxes and no periodic wrap is applied between the passes.  At non-periodic domain faces the stencil indices are clamped to the domain. */
int iamrx_particles_advect(iamrx_particles pc, int lev, iamrx_mf umac_x, iamrx_mf umac_y, iamrx_mf umac_z, double dt);
/* Redistribute(lev_min, lev_max, ngrow) for the particles of the levels >= lev_min: periodic wrap; the finest level <= lev_max whose boxes hold
 * the particle's cell; failing that and with ngrow > 0 the box of lev_min with the lowest index whose ngrow-grown region holds it (or a periodic
 * image of it, which the particle then takes; of several images the one shifted in the fewest directions); a particle outside a non-periodic domain is removed and counted in *removed; a particle that
 * cannot be placed is an error (the container stays as it was). */
int iamrx_particles_redistribute(iamrx_particles pc, int lev_min, int lev_max, int ngrow, long* removed);
/* which = 0: particle_count (particles of level lev per valid cell); 1: total_particle_count (plus the finer levels' counts coarsened onto
 * lev, NavierStokesBase.cpp:3996-4048); out: cell-centred on the container's boxes of level lev */
int iamrx_particles_derive_count(iamrx_particles pc, int which, int lev, iamrx_mf out, int ocomp);
/* The components comps[0 .. ncomp) (1 <= ncomp <= 16, any order, repeats allowed) of the cell-centred mf on the container's boxes of level
 * lev at the particles of that level, in storage order: vals[p * ncomp + m], id[p], cpu[p] for p < count[lev] (any may be NULL; all three
 * NULL: the kernel is launched and nothing is read back or waited for).  Trilinear between cell centres: per direction
 * l = (x - prob_lo) / dx - 0.5, cells floor(l) and floor(l) + 1 with the weights 1 - w and w = l - floor(l), nested as a + w (b - a) in x,
 * then y, then z.  The stencil is clamped to the array's own index range and NOT to the domain: fill the ghost cells the particles'
 * stencils reach (one layer for particles inside their boxes) with what the boundary conditions say.  A particle with id <= 0 gets zeros. */
int iamrx_particles_sample(iamrx_particles pc, int lev, iamrx_mf mf, int ncomp, const int* comps, double* vals, int* id, int* cpu);
/* Timestamp files (NavierStokesBase::post_timestep_particle, NavierStokesBase.cpp:3881-3951).  basename NULL or "": off (the default).
 * indices[n] (n <= 16): the State_Type components that the steps of the object the container is attached to sample after each of their
 * redistributions (FillPatched from the new state); they then call iamrx_particles_timestamp for every level that holds particles. */
int iamrx_particles_set_timestamp(iamrx_particles pc, const char* basename, int n, const int* indices);
/* appends one line per particle of level lev with id > 0, sorted by (id, cpu), to <basename>_<two digits of rank % 64> (append mode; a rank
 * without such particles touches no file):   id cpu x y z time r0 r1 r2 v_0 .. v_{n-1}   -- single blanks, reals as %.10e; v_m is
 * component m of mf at the particle (mf: cell-centred on the level's boxes, at least n components; NULL: the line ends after r2).  With a
 * fixed direction d (iamrx_particles_set_fixed_dir) the coordinate d and r_d are left out. */
int iamrx_particles_timestamp(iamrx_particles pc, int lev, iamrx_mf mf, double time);
/* attach (pc = NULL: detach).  A level on its own advects its particles at the end of every advance but the initial one and redistributes in
 * iamrx_ns_step; a hierarchy follows NavierStokes::advance / post_timestep_particle / post_regrid.  iamrx_ns_derive knows "particle_count"
 * and "total_particle_count" while a container is attached.  The container must outlive the attachment or be detached first. */
int iamrx_ns_set_particles(iamrx_ns ns, iamrx_particles pc);
int iamrx_amr_set_particles(iamrx_amr a, iamrx_particles pc);
int iamrx_ns_get_particles(iamrx_ns ns, iamrx_particles* pc /* NULL handle: none; not to be destroyed by the caller unless it created it */);
int iamrx_amr_get_particles(iamrx_amr a, iamrx_particles* pc);

#ifdef __cplusplus
}
#endif
#endif
