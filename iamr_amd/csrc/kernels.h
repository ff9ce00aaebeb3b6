// iamr_amd/csrc/kernels.h -- host-callable launchers of the hand-written HIP kernels (gfx950).
#pragma once
#include "core.h"
#include "mf.h"

namespace iamrx {

// ---- k_basic.hip --------------------------------------------------------------------------
void launch_fill(double* p, size_t n, double v, hipStream_t s);
void launch_copy_plan(const CopyDesc* d, int nd, long maxpts, const FabD* src, const FabD* dst, int scomp, int dcomp, int nc, hipStream_t s, bool add = false);
void launch_pack(const CopyDesc* d, int nd, long maxpts, const FabD* src, double* buf, long pts_total, int scomp, int nc, hipStream_t s);
void launch_unpack(const CopyDesc* d, int nd, long maxpts, const FabD* dst, const double* buf, long pts_total, int dcomp, int nc, hipStream_t s, bool add = false);
// the same three over a flat work list (mf.h CopyWork: nw entries (descriptor, chunk)): one workgroup per COPY_CHUNK points that exist
void launch_copy_plan_w(const CopyDesc* d, const int2* w, int nw, const FabD* src, const FabD* dst, int scomp, int dcomp, int nc, hipStream_t s, bool add);
void launch_pack_w(const CopyDesc* d, const int2* w, int nw, const FabD* src, double* buf, long pts_total, int scomp, int nc, hipStream_t s);
void launch_unpack_w(const CopyDesc* d, const int2* w, int nw, const FabD* dst, const double* buf, long pts_total, int dcomp, int nc, hipStream_t s, bool add);
// global: combined over the ranks (on the device, before the single read-back) unless the layout is replicated
double reduce_norm0(const MultiFab& mf, int comp, int nc, int ng, bool global = false);
void reduce_norm0_comps(const MultiFab& mf, int comp, int nc, int ng, double* out, bool global = false);   // per-component maxima, one read-back
void reduce_minmax(const MultiFab& mf, int comp, int ng, double& mn, double& mx, bool global = true);   // one pass, one read-back
double reduce_sum_unique(const MultiFab& mf, int comp, const Geometry& g, bool global = false);   // sum over owner copies
// this rank's sums of density, tracer and kinetic energy over the valid cells where cov (may be null) is zero: one pass over the state
void reduce_sum_integrated(const MultiFab& S, int rho_comp, int trac_comp, const MultiFab* cov, double out[3]);
// this rank's sums of the components comps[0 .. n) of a cell-centred array over the valid cells where cov (may be null) is zero; the
// tiling and the summation order of reduce_sum_integrated (the same call gives the same bits), SUM_COMPS_MAX components per pass
constexpr int SUM_COMPS_MAX = 8;
void reduce_sum_comps(const MultiFab& mf, int n, const int* comps, const MultiFab* cov, double* out);
// nout simultaneous dot products over the valid region, owner-masked for nodal data: out[q] = <x_q, y_q>
void reduce_dots(int nout, const MultiFab* const* x, const MultiFab* const* y, int comp, int nc, const Geometry& g, double* out, bool local = false);
// ... with the results left on the device (no read-back): krylov.h
void reduce_dots_dev(int nout, const MultiFab* const* x, const MultiFab* const* y, int comp, int nc, const Geometry& g, double* d_out, bool local = false);
// y = a*x + b*y etc. (valid region + ng)
// HIP-event probe around the k_nodal_gs4 launches of levels with >= min_nodes nodes per box (see k_nodal.hip)
// HIP-event probes around the launches of one kernel family on levels with at least min_points cells / nodes per box (every stride-th one)
enum { PROBE_NODAL_GS4 = 0, PROBE_ABEC_GSRB = 1, PROBE_GOD_Z = 2, PROBE_PRED_Z = 3, PROBE_COUNT = 4 };
void kernel_probe_start(int which, long min_points, int stride);
void kernel_probe_stop(int which, double* total_ms, long* launches);
void kernel_probes_pause(bool on);      // no probe events while a launch sequence is being captured into a graph
bool kernel_probe_begin(int which, long points);     // true: the start event was recorded, call kernel_probe_end after the launch
void kernel_probe_end(int which);
void gs4_probe_start(long min_nodes, int stride);
void gs4_probe_stop(double* total_ms, long* launches);
void mf_lincomb(MultiFab& dst, double a, const MultiFab& x, double b, const MultiFab& y, int comp, int nc, int ng);   // dst = a*x + b*y
void mf_saxpy(MultiFab& y, double a, const MultiFab& x, int xcomp, int ycomp, int nc, int ng);                          // y += a*x
void mf_add_scalar(MultiFab& y, double a, int comp, int nc, int ng);
double mf_add_scalar_norm0(MultiFab& y, double a, int comp, int ng);      // y(comp) += a and the max norm of the result (norm0's), one pass
void mf_mult(MultiFab& y, double a, int comp, int nc, int ng);
// the same on the ng ghost layers only (the valid region is not touched): one launch over the shell of every box
void mf_mult_ghosts(MultiFab& y, double a, int comp, int nc, int ng);
void mf_half_sum_ghosts(MultiFab& h, const MultiFab& a, const MultiFab& b, int ng);   // h = 0.5 * (a + b) on the ghost shell, component 0
// ---- the dense image of a level (k_basic.hip): what the spectra and the structure functions work on ----
// throws "<who>: ..." unless the boxes of the layout lie inside the domain of g and hold as many cells as it
void dense_check_cover(const char* who, const Geometry& g, const Layout& lay);
// the valid cells of THIS rank's boxes of component comp of a cell-centred array -> their place in the index space of the domain of g
// (x fastest; ghost cells are never read): dst[o] = f, or with cplx dst[2 o] = f, dst[2 o + 1] = 0.  Cells of other ranks are not written.
void dense_pack(const Geometry& g, const MultiFab& S, int comp, double* dst, bool cplx);
// the same cells into the imaginary parts alone, dst[2 o + 1] = f: the second field of a packed pair (k_spectrum.hip)
void dense_pack_imag(const Geometry& g, const MultiFab& S, int comp, double* dst);
// the whole field as a real array on every rank.  One rank (or a replicated layout): dense_pack.  Several: every rank packs its boxes
// into the zeroed array and the arrays are summed through the communicator (exact: a cell has one owner) -- a gather, collective.
void dense_gather(const Geometry& g, const MultiFab& S, int comp, double* R);
bool dense_needs_gather(const MultiFab& S);      // several ranks and a layout that is not replicated
// the inverse of dense_pack with cplx: the valid cells of THIS rank's boxes of component comp take scale * the real part src[2 o] of
// their place in the complex image of the domain (the whole image is on every rank); ghost cells are not written
void dense_unpack(const Geometry& g, MultiFab& S, int comp, const double* src, double scale);

// ---- k_stats.hip: on-the-fly velocity statistics (NS_average.cpp, NS_derive.cpp:11-45) ------
// avg(0..2) += dt_avg * vel; fluct: avg(3..5) += dt_avg * (vel - avg(0..2) / t_sum)^2 with the updated avg(0..2); vel = S(vcomp..)
void stats_accumulate(MultiFab& avg, const MultiFab& S, int vcomp, double dt_avg, double t_sum, bool fluct);
// out(ocomp..ocomp+2) = avg(0..2) / t_mean, out(ocomp+3..ocomp+5) = sqrt(avg(3..5) / t_fluct); a zero divisor counts as 1
void stats_derive_vel_avg(MultiFab& out, int ocomp, const MultiFab& avg, double t_mean, double t_fluct);

// ---- k_profile.hip: plane-averaged profiles of the state along one axis ----------------------
// the quantities, in this order: 1, u, v, w, rho, c, uu, vv, ww, uv, uw, vw, rho rho, c c
constexpr int PROFILE_NQ = 14;
// one level of the hierarchy: its state, the mask of the cells a finer level covers (cov != 0 there; null: none) and its geometry
struct ProfileLevel { const MultiFab* S; const MultiFab* cov; const Geometry* g; };
int profile_nbins(const Geometry& g0, int dir, int bin_level);      // cells of level 0 along dir, times 2^bin_level
// out[q * nbins + b] = volume-weighted mean of quantity q over the uncovered cells of levels 0 .. nlev - 1 (ratio 2) that meet slab b of
// the index space of level bin_level along dir; a cell coarser than the bins counts in every bin it spans.  One launch per level, sums in
// a fixed order (the same call gives the same bits), one all-reduce of the bins over the ranks (a replicated level counts once); every
// rank receives the result.  A NaN in a counted cell reaches the bins of that cell only; a covered cell is skipped.
void profile_reduce(int nlev, const ProfileLevel* L, int dir, int bin_level, int rho_comp, int trac_comp, double* out);

// ---- k_spectrum.hip: shell-summed power spectra of a triply periodic level -------------------
// the columns the level and hierarchy entries return: P_u, P_v, P_w, P_c (c: the first tracer)
constexpr int SPECTRUM_NQ = 4;
// the number of shells of the geometry (include/iamrx.h); throws, naming the reason, if a direction is not periodic or an extent is
// not a power of two in 4 .. 1024
int spectrum_nbins(const Geometry& g);
// out[q * nbins + s] = sum over the modes of shell s of |F(m)|^2 of component comps[q] of S (cell-centred; its boxes tile the domain of
// g; ghost cells are never read), count[s] (or null) = modes of shell s.  nbins = spectrum_nbins(g).  One component at a time through
// one complex work array from the arena; sums in a fixed order (the same call gives the same bits, however the level is cut into
// boxes).  Collective on several ranks: the field is gathered on every rank, every rank transforms it and receives the same bits; with
// SPECTRUM_DIST = 1 the slab-decomposed transform below instead (the same bits again; an ineligible call throws on every rank).
void spectrum_compute(const Geometry& g, const MultiFab& S, int nq, const int* comps, int nbins, double* out, long* count);
// measurement aid (tools/bench_spectrum.py): reps times the five passes of one component -- pack, x, y, z, shell sums -- with an event
// between them; ms[5 * r + p] = milliseconds of pass p in repeat r
void spectrum_bench(const Geometry& g, const MultiFab& S, int comp, int reps, float* ms);
// ---- co-spectra: two real fields through ONE packed transform Z = a + i b ----
// a pair of cell-centred components; the two arrays tile the domain, may be the same array and may live on different layouts
struct SpecPair { const MultiFab* a; int acomp; const MultiFab* b; int bcomp; };
// the columns of a pair, in this order: C_ab(s) = sum over shell s of Re(F_a conj F_b), P_a, P_b, W_a(s) = sum of k(m)^2 |F_a(m)|^2 with
// k(m)^2 = (2 pi / L_max)^2 kappa^2 (the spectral |grad a|^2, not the solver's discrete one)
constexpr int COSPEC_NV = 4;
// out[(COSPEC_NV * q + v) * nbins + s] = column v of pair q; count as in spectrum_compute.  The transforms, the fixed-order sums (the
// same call gives the same bits, whatever the box layouts) and the gather on several ranks are those of spectrum_compute.
void cospectrum_compute(const Geometry& g, int npair, const SpecPair* pairs, int nbins, double* out, long* count);
// out[q * nbins + s] = W(s) of component comps[q] of S alone (one plain transform per component)
void spectrum_k2_compute(const Geometry& g, const MultiFab& S, int nq, const int* comps, int nbins, double* out);
// measurement aid (tools/bench_budget.py): the five passes of one packed pair -- pack, x, y, z, the shell sums with the mirror read --
// timed as spectrum_bench times its five
void cospectrum_bench(const Geometry& g, const MultiFab& A, int acomp, const MultiFab& B, int bcomp, int reps, float* ms);
// ---- plane spectra: ring-summed 2-D spectra along a normal axis (include/iamrx.h: iamrx_mf_plane_spectrum; k_spectrum.hip) ----
// the columns the level and hierarchy entries return: P_u, P_v, P_w, P_rho, P_c (c: the first tracer)
constexpr int PLANE_SPECTRUM_NQ = 5;
constexpr int PLANE_SPECTRUM_BENCH_NP = 4;          // pack, the two transform passes, the ring sums
struct PlaneSpecDims { int nplanes, nrings; };
// the checks of the plane spectra of n fields (or packed pairs: b set), by name and in the order of include/iamrx.h -- dir, cell-centred,
// components, the two transformed directions periodic, their extents, the lengths, the rings, the cover -- before anything is allocated
// -> the planes along dir and the rings.  The normal direction may have any boundary type and any extent.
PlaneSpecDims plane_spectrum_check(const Geometry& g, int dir, int n, const SpecPair* f);
// plain fields (every b null): out[(q * nplanes + p) * nrings + s] = sum over the modes of ring s of |F_p|^2 of field q; one packed pair
// (n = 1, b set): out[(v * nplanes + p) * nrings + s], v = 0, 1, 2: C_ab, P_a, P_b.  count[s] (or null): the modes of ring s, the same in
// every plane.  dims = plane_spectrum_check(g, dir, n, f).  Fixed-order sums without floating-point atomics: the same bits on a repeated
// call, for any box layout and any rank count.  Collective on several ranks: the gather of spectrum_compute, whatever SPECTRUM_DIST says.
void plane_spectrum_compute(const Geometry& g, int n, const SpecPair* f, int dir, PlaneSpecDims dims, double* out, long* count);
// measurement aid (tools/bench_plane_spectrum.py): ms[PLANE_SPECTRUM_BENCH_NP * r + p] of pack, the first and the second transform pass
// and the ring sums (with their slot sum) of one component
void plane_spectrum_bench(const Geometry& g, const MultiFab& S, int comp, int dir, int reps, float* ms);
// ---- the slab-decomposed transform of several ranks (SPECTRUM_DIST = 1; include/iamrx.h, k_spectrum.hip) ----
// a box cut by a z-slab: kind 0 the piece stays on the rank, 1 sent to peer, 2 received from peer; off: doubles, in the buffer of that
// peer (-1 for kind 0)
struct SpecSlabRow { int kind, peer, box; int lo[3], hi[3]; long off; };
// host only: is the slab path eligible on nranks ranks (why: the reason if not), and the scatter plan of `rank`.  Rows: the kept
// pieces, then per peer in rank order its send rows and its receive rows, each in box order
bool spectrum_slab_plan(const BoxD& domain, const std::vector<BoxD>& boxes, const std::vector<int>& owner, int rank, int nranks, std::string* why,
                        std::vector<SpecSlabRow>* rows);
// the last shell-sum call of this rank (include/iamrx.h: iamrx_spectrum_slab_info)
struct SpecSlabInfo { long path = 0, ranks = 1, max_image = 0, per_pass = 0, sent = 0, received = 0, transforms = 0; };
SpecSlabInfo spectrum_slab_info();
// measurement aid (tools/bench_spectrum_slab.py): the kernels one rank of R runs for one plain transform, the exchanges left out
constexpr int SPEC_SLAB_BENCH_NP = 10;
void spectrum_slab_bench(const Geometry& g, int R, int reps, float* ms);
// ---- the way back from mode space (include/iamrx.h): filters, the solenoidal projection, a synthetic isotropic field ----
// f = conj(FFT(conj(N F))) / N through the forward passes; the conjugation and 1 / N ride on the mode-space pass k_spec_mul<Op>
constexpr int SPECOP_NKIND = 4;             // identity, sharp, Gaussian, box
constexpr int SPECOP_NWAVE = 2;             // exact, centred
constexpr int SPECOP_BENCH_NP = 17;
// white noise of (seed, c, global cell index) in the valid cells of S(comp + c), c < ncomp; any domain whose boxes S tiles
void specop_noise(const Geometry& g, MultiFab& S, int comp, int ncomp, unsigned long long seed);
// dst(dcomp + q) = G * src(scomp + q); the checks of the spectra on both arrays, then kind and kc, before anything is written
void specop_filter(const Geometry& g, MultiFab& dst, int dcomp, const MultiFab& src, int scomp, int ncomp, int kind, double kc);
void specop_solenoidal(const Geometry& g, MultiFab& dst, int dcomp, const MultiFab& src, int scomp, int wavenumber);
void specop_synthesize(const Geometry& g, MultiFab& dst, int dcomp, unsigned long long seed, int nbins, const double* E_target, int wavenumber);
void specop_bench(const Geometry& g, MultiFab& dst, const MultiFab& src, int scomp, int kind, double kc, int wavenumber, int reps, float* ms);
// ---- a-priori LES analysis (include/iamrx.h: iamrx_mf_sgs): the driver beside specop_filter, its own kernels in k_sgs.hip ----
constexpr int SGS_NSTAT = 16;               // the means of include/iamrx.h
constexpr int SGS_NFIELD = 10;              // tau_xx tau_xy tau_xz tau_yy tau_yz tau_zz k_sgs sgs_flux filtered_strain smag_flux
constexpr int SGS_MAXWG = 1024;             // workgroups (= slots per statistic) of k_sgs_point: a function of N alone
constexpr int SGS_BENCH_NP = 6;
// the nine dense images of a call after their inverse transforms.  U: the filtered velocities, read at the face neighbours; P: the
// filtered products xx xy xz yy yz zz, read at the cell itself and overwritten by the fields of `mask` (bit f: field f; tau_ij over the
// real part of P[ij], fields 6 .. 9 into the imaginary parts of P[0 .. 3]).  ln: log2 of the extents; dxi: 1 / dx; delta2: Delta^2
struct SgsPoint {
    const double2* U[3];
    double2* P[6];
    int ln[3];
    double dxi[3];
    double delta2;
    int mask;
};
// the valid cells of S(ci) * S(cj) of THIS rank's boxes -> their place in the dense image: dense_pack on a product (no array of products)
void sgs_pack_product(const Geometry& g, const MultiFab& S, int ci, int cj, double* dst, bool cplx);
int sgs_nwg(long N);
// k_sgs_point and its finish kernel: slots holds SGS_NSTAT * sgs_nwg(N) doubles, neg one counter (zeroed here), stats SGS_NSTAT + 1
// doubles -- the means, then the bits of the count of cells with Pi < 0
void sgs_point(const SgsPoint& a, double* slots, unsigned long long* neg, double* stats);
// stats[SGS_NSTAT], counts[2] = {N, cells with Pi < 0} of vel(vcomp .. vcomp + 2) under the filter (kind, kc); out (null with nout = 0:
// statistics only) takes field which[q] in component ocomp + q of its valid cells.  Every check before anything is written.
void sgs_compute(const Geometry& g, const MultiFab& vel, int vcomp, int kind, double kc, MultiFab* out, int ocomp, int nout, const int* which,
                 double* stats, long* counts);
// measurement aid (tools/bench_sgs.py): ms[SGS_BENCH_NP * r + p], p = 0 the three plain packs, 1 the six product packs, 2 the 54 transform
// passes and nine multipliers, 3 k_sgs_point with its finish, 4 the unpack of the nout fields, 5 one dense_pack of vel(vcomp) alone
void sgs_bench(const Geometry& g, MultiFab* out, const MultiFab& vel, int vcomp, int kind, double kc, int nout, const int* which, int reps, float* ms);

// ---- k_convect.hip: the skew-symmetric centred nonlinear term ----------------------------------
// out(ocomp + i) = N_i = 0.5 sum_d [u_d delta_d u_i + delta_d(u_d u_i)] of vel(vcomp .. vcomp + 2) on the valid cells (the evaluation
// order: k_convect.hip); vel: cell-centred, same layout, at least one FILLED ghost layer (only the face neighbours of a cell are read)
void convective_term(const Geometry& g, MultiFab& out, int ocomp, const MultiFab& vel, int vcomp);
// measurement aid: ms[r] = one launch into out(0 .. 2) between two events, nothing read back
void convective_bench(const Geometry& g, MultiFab& out, const MultiFab& vel, int vcomp, int reps, float* ms);
// the columns of the spectral budget of a level: E, T, D, F (include/iamrx.h)
constexpr int BUDGET_NQ = 4;

// ---- k_strfn.hip: structure functions and two-point correlations along the axes --------------
// the components the level and hierarchy entries take: u, v, w and the first tracer
constexpr int STRFN_NQ = 4;
constexpr int STRFN_PMAX = 8;               // moments 1 .. pmax <= 8
constexpr int STRFN_MAX_EXTENT = 1024;      // cells along an axis that is not skipped
int strfn_ncol(int pmax);                   // 1 + pmax + ceil(pmax / 2); throws on pmax outside 1 .. STRFN_PMAX
// the separations of a call: rmax[d] = -1 -> the largest allowed (n_d / 2 periodic, n_d - 1 otherwise), 0 -> the axis is skipped;
// throws, naming the axis, on a larger request, on one below -1 and on an extent above STRFN_MAX_EXTENT of an axis that is not skipped
void strfn_resolve_rmax(const Geometry& g, const int rmax[3], int out[3]);
// pairs of axis d at separation r (include/iamrx.h): N periodic, (n_d - r) N / n_d otherwise
long long strfn_count(const Geometry& g, int d, int r);
// out[((d * nq + c) * ncol + col) * rcap + r] = column col of component comps[c] of S (cell-centred; its boxes tile the domain of g; ghost
// cells are never read) along axis d at separation r <= rmax[d] (resolved, <= rcap - 1), zero beyond; mean[c] (or null) = <f_c>.  One
// component at a time through one dense real array from the arena (dense_gather: the only step that sees boxes or ranks), one pair
// launch per axis; sums in a fixed order, no floating-point atomics: the same call gives the same bits for any box layout and any
// number of ranks.  Collective on several ranks.
void strfn_compute(const Geometry& g, const MultiFab& S, int nq, const int* comps, int pmax, const int rmax[3], int rcap, double* out, double* mean);
// measurement aid (tools/bench_strfn.py): reps times the four passes of one component -- pack, x, y, z (each pair launch with its finish
// kernel) -- with an event between them; ms[4 * r + p] = milliseconds of pass p in repeat r (0 for a skipped axis)
void strfn_bench(const Geometry& g, const MultiFab& S, int comp, int pmax, const int rmax[3], int reps, float* ms);

// ---- k_hist.hip: histograms of cell-centred components (integer counts, exact) ----------------
// The binning rule per column (lo < hi finite, inv = nbins / (hi - lo) in double): NaN -> slot nan, v < lo -> below, v > hi -> above,
// otherwise bin min((int)((v - lo) * inv), nbins - 1).  Slots of a column: the nbins bins, then below, above, nan.
constexpr int HIST_NBINS_MAX = 4096;        // bins of a column
constexpr int HIST2_SLOTS_MAX = 16384;      // nbx * nby of a joint histogram
void hist_check_range(const char* who, double lo, double hi, int nbins, int nbins_max);        // throws on what the rule excludes
// zeroed device slots; hist_add / hist_add2 add the cells of this rank's boxes of one level to them (cov: cells with cov != 0 are skipped,
// null: none; ghost cells are never read), every counted cell `weight`; hist_end brings them to the host, sums them over the ranks (as
// doubles: every slot and their total must stay below 2^53).  A level every rank holds in full is counted once.
DevBuf<unsigned long long> hist_begin(size_t nslots);
// d_counts[q * (nbins + 3) + s] += ... for the columns q = 0 .. ncol - 1 = components comps[q] of S
void hist_add(const MultiFab& S, int ncol, const int* comps, const MultiFab* cov, const double* lo, const double* hi, int nbins,
              unsigned long long weight, unsigned long long* d_counts);
// joint: d_counts[bx * nby + by] += ..., d_counts[nbx * nby] (`outside`) takes a cell that is NaN or out of range on either axis
void hist_add2(const MultiFab& X, int compx, const MultiFab& Y, int compy, const MultiFab* cov, const double lo[2], const double hi[2],
               const int nbins[2], unsigned long long weight, unsigned long long* d_counts);
void hist_end(const unsigned long long* d_counts, size_t nslots, long long* out);
// the device slots of one histogram call: hist_begin here, hist_end in finish(); freed with the call, also when an error unwinds past them
struct HistSlots {
    size_t n; DevBuf<unsigned long long> d;
    explicit HistSlots(size_t nslots) : n(nslots), d(hist_begin(nslots)) {}
    void finish(long long* counts) { hist_end(d, n, counts); }
};
// the checks of a joint histogram: both ranges, and nbins[0] * nbins[1] <= HIST2_SLOTS_MAX (diagnostics.hip)
void hist2_check(const char* who, const double lo[2], const double hi[2], const int nbins[2]);
// measurement aid: ms[r] = the launches of one hist_add (nby = 0) or hist_add2 (ncol = 2, nby > 0) between two events, nothing read back
void hist_bench(const MultiFab& S, int ncol, const int* comps, const MultiFab* cov, const double* lo, const double* hi, int nbins, int nby,
                int reps, float* ms);

// ---- k_velgrad.hip: derived fields of the velocity-gradient tensor ---------------------------
// the quantity ids, in this order: diveru, vort_x, vort_y, vort_z, enstrophy, strain_rate, dissipation, q_criterion, r_invariant, helicity
// (the definitions: k_velgrad.hip)
constexpr int VELGRAD_NQ = 10;
// out(ocomp + q) = quantity which[q] (q < nq <= VELGRAD_NQ) of the centred gradient of vel(vcomp .. vcomp + 2) on the valid cells; vel:
// cell-centred, same layout, at least one FILLED ghost layer (only the face neighbours of a cell are read); mu: the dynamic viscosity of
// "dissipation".  path 0: the marching form where the level's largest box holds a full 32 x 8 tile, else the plain form; 1 / 2 force
// the marching / plain form (1 on a level without a full tile is an error).  The two forms give the same bits.
void derive_velgrad(const Geometry& g, MultiFab& out, int ocomp, int nq, const int* which, const MultiFab& vel, int vcomp, double mu, int path = 0);
int velgrad_path(const Layout& l, int path);        // the form a call takes: 1 marching, 2 plain
// measurement aid: ms[r] = one launch of nq outputs into out(0 .. nq) (split: nq single-output launches) between two events, nothing
// read back
void velgrad_bench(const Geometry& g, MultiFab& out, int nq, const int* which, const MultiFab& vel, int vcomp, double mu, int path, bool split,
                   int reps, float* ms);

struct DomainBC;
// ---- k_bc.hip -----------------------------------------------------------------------------
// physical-BC fill of cell-centred ghost cells outside the domain; extdir_lo/hi[n*3+d] constant ext_dir values
void fill_physbc_cc(const Geometry& g, MultiFab& mf, int scomp, int ncomp, const BCRec* bc, const double* extdir_lo, const double* extdir_hi);

void nodal_reflect_bc(const Geometry& g, MultiFab& mf, const DomainBC& bc, hipStream_t on = nullptr);   // ghost nodes: even reflection about Neumann walls
void cc_mirror_bc(const Geometry& g, MultiFab& mf);                           // cell-centred mirror across all non-periodic walls

// ---- k_abec.hip ---------------------------------------------------------------------------
struct AbecCoef {
    double alpha, beta;
    const MultiFab* a;        // cell, 1 comp (may be null)
    const MultiFab* b[3];     // face, ncomp comps (or 1 comp broadcast if b_ncomp == 1)
    int tensor;               // add MLTensorOp cross terms in apply/residual
    int tensor_eta = 0;       // b[d] hold the 1-component face viscosity eta_d; the kernels apply b_d(comp) = eta_d * (comp == d ? 4/3 : 1)
    // sig != null: b[d] was made by mac_bcoef(b, *sig, sig_comp, sig_scale) and the smoother / residual kernels may recompute the face
    // value sig_scale / (0.5 (sig(cell - e_d) + sig(cell))) from the cell-centred array instead of reading three face arrays (the same
    // expression, hence the same doubles; one array of HBM traffic instead of three).  sig has >= 1 ghost cell, filled.
    // b[d] may then be null (CellMG::prepare: no consumer of the level reads the arrays, so none were made).
    const MultiFab* sig = nullptr;
    int sig_comp = 0;
    double sig_scale = 1.0;
    // b_uniform: every entry of the one-component b[d] equals bu[d] (constant viscosity / diffusivity: mf_uniform_value found it so);
    // the smoother and residual kernels use the constants instead of reading the three face arrays
    int b_uniform = 0;
    double bu[3] = {0.0, 0.0, 0.0};
};
// every valid entry of component 0 of m equals one value (on all ranks): returns true and the value
bool mf_uniform_value(const MultiFab& m, double* v);
// the tensor operator's residual / apply in ONE launch where its viscosity is constant (k_tensor.hip); false: use abec_residual
bool tensor_residual_fused(const Geometry& g, const AbecCoef& c, MultiFab& out, const MultiFab& vel, const MultiFab* rhs, double* norm_out);
struct DomainBC {             // linear-operator BC of the level's domain
    int lo[3], hi[3];         // LinOpBC per face
    int maxorder;
};
// Coarse/fine faces of a level that does not cover the domain (MLLinOp::setCoarseFineBC): Dirichlet data half a coarse cell behind
// the face.  c[d][NX-2][m]: Lagrange weights of the ghost formula through x = {-loc/dx, 0.5, 1.5, 2.5} (m = 0: the coarse datum),
// NX = min(box length + 1, maxorder).
struct CfTab { double c[3][3][4]; int maxorder; };
CfTab cf_make_tab(const double loc[3], const double dx[3], int maxorder);
// cell mask, ghost cells included: 0 = cell of the level (valid, neighbour box or periodic image), 1 = coarse/fine ghost cell,
// 2 = outside the physical domain
void cf_build_mask(const Geometry& g, MultiFab& cfm);
// ghost cells with mask 1 next to a box face: phi = c[0] * bcval (inhomog) + sum_m c[m] * phi(m-th cell inside)   (mllinop_apply_bc)
// edges: also the edge / corner coarse-fine ghost cells (tensor operator): bcval there (cf_interp_edges) or zero
void cf_fill_ghosts(MultiFab& phi, const MultiFab& cfm, const CfTab& tab, bool inhomog, const MultiFab* bcval, bool edges = false);
void cf_interp_edges(MultiFab& bcval, const MultiFab& cpatch, const MultiFab& cfm, int ratio, const Geometry& cgeom);
// bcval(ghost cells with mask 1) = coarse data of cpatch (coarsened layout, 1 ghost cell) interpolated in the tangential directions
// (InterpBndryData::setBndryValues, third order, ratio 2); cfm needs 2 ghost cells
void cf_interp_bndry(MultiFab& bcval, const MultiFab& cpatch, const MultiFab& cfm, int ratio);
// ---- the smoother path of a cell-centred multigrid level ----
// What the choice rests on, as host data (no array, no device).  boxes is the level's GLOBAL box list: the path is decided from it, so
// every rank takes the same one (a rank without a box launches nothing).  max_len / nlocal: Layout's.
struct AbecLevel {
    const std::vector<BoxD>* boxes = nullptr;
    int nlocal = 0, max_len[3] = {0, 0, 0};
    int ncomp = 1;
    int phi_ngrow = 1, rhs_ngrow = 0, sig_ngrow = 0, a_ngrow = 0;      // ghost widths: correction, right-hand side, density, a-term
    bool sig = false, b_uniform = false, has_a = false, tensor_eta = false;      // the coefficient form (AbecCoef); has_a: a given and alpha != 0
    bool tensor = false;                                                // the level belongs to a tensor solve (no coarse/fine maintenance)
    int b_ncomp = 1;
    int nbc = 0;
    const DomainBC* bcs = nullptr;         // nbc sets: one per component, or one for all; null: fully periodic levels only
    bool has_cf = false;                   // coarse/fine faces (mask and table at hand)
    bool finest = true;                    // level 0 of its hierarchy
};
AbecLevel abec_level(const AbecCoef& c, const MultiFab& phi, int rhs_ngrow, int nbc, const DomainBC* bcs, bool has_cf = false, bool finest = true);
// One colour pass (abec_gsrb): the kernel and what it is told.  Filled by abec_smooth_plan, or by abec_colour_form for a caller that fills
// the ghost cells itself.
struct AbecColourForm {
    enum Kernel { GENERAL, GSRB1, GSRB2, GSRB2_PER_COMP } kernel = GENERAL;
    int mode = 0;                 // GSRB1 / GSRB2 coefficients: 0 stored face arrays, 1 recomputed from the density, 2 the constants bu
    int np = 1;                   // GSRB1: planes in flight (1, 2 or 4)
    bool gen_mc = false;          // the general kernel's <MC, mode> (also what a shell pass runs whatever `kernel` says)
    int gen_mode = 0;
    bool has_cf = false, maintain = false, allcf = false;     // coarse/fine faces; the passes keep their ghost cells current; all ghost cells are such
    bool wrap = false;            // one box spanning a periodic domain: images read from the valid cells, no ghost fill
    bool walls_inkernel = false;  // one box spanning a domain with walls: the pass applies them (WallK), the caller fills periodic ghost cells only
    bool zero_ok = false;         // the first pass may be told that phi is zero instead of phi being set to zero (no ghost cell is read)
};
struct AbecSmoothPlan {
    enum Path { COLOUR, RB_BOX, RB_CF, RB_NBR, FUSED_SHELL } path = COLOUR;
    AbecColourForm colour;        // COLOUR, and the shell pass of FUSED_SHELL
    int nw = 16;                  // RB_*: wavefronts per workgroup (12 or 16)
    bool nbr_splits = false;      // RB_NBR: the sweep can be issued in two parts (tiles that read no ghost cell / the others)
    bool zero_first = false;      // the first sweep of a smoothing call on this level may start from zero
    int ncomp = 1, phi_ngrow = 1, rhs_ngrow = 0;      // what the plan was made for (the launchers assert it)
    bool sweep_kernel() const { return path == RB_BOX || path == RB_CF || path == RB_NBR; }
    bool made_for(const MultiFab& phi, const MultiFab& rhs) const { return phi.ncomp == ncomp && phi.ngrow == phi_ngrow && rhs.ngrow == rhs_ngrow; }
};
// THE decision: which of the five ways a smoothing call on this level runs, made once per level per solve
AbecSmoothPlan abec_smooth_plan(const Geometry& g, const AbecLevel& lv);
// the colour-pass part alone.  wrap: the level is one periodic box (periodic_wrap_ok); walls_inkernel: the passes may apply the walls
// themselves where they can (false: the caller fills every ghost cell)
AbecColourForm abec_colour_form(const Geometry& g, const AbecLevel& lv, bool wrap = false, bool walls_inkernel = false);
// one red (0) or black (1) pass.  bcs: nbc DomainBC entries (nbc == 1: same BC for all components; nbc == ncomp: one per component,
// MLTensorOp::setDomainBC).  shell_only: the black cells on box surfaces only (behind abec_gsrb_fused).  phi_is_zero: needs f.zero_ok.
void abec_gsrb(const Geometry& g, const AbecCoef& c, const AbecColourForm& f, MultiFab& phi, const MultiFab& rhs, int redblack, double omega,
               const DomainBC* bcs, int nbc, bool shell_only = false, bool phi_is_zero = false, const MultiFab* cfm = nullptr, const CfTab* cftab = nullptr);
// the last two levels of a cell-centred V-cycle in one single-workgroup launch (k_abec_tail, k_abec.hip): pre-smoothing from zero, residual,
// restriction, bottom solve, prolongation, post-smoothing -- the doubles of the launches it replaces
bool abec_tail_ok(const Geometry& gF, const Layout& lF, const Geometry& gC, const Layout& lC, const AbecCoef& cF, const DomainBC* bcs, int nbc, int ncomp);
void abec_tail_solve(const Geometry& gF, const AbecCoef& cF, MultiFab& corF, const MultiFab& resF, const Geometry& gC, const AbecCoef& cC,
                     const DomainBC& bc, bool singular, double eps_rel, int maxiter, int nub, int nuf, int nu1, int nu2, double omega, int* d_iters);
// ---- k_abec_legs.hip: a coarse level of the cell-centred V-cycle in two launches ----
// Down leg: nu1 red-black sweeps from zero, the residual and its restriction; up leg: prolongation and nu2 sweeps (the doubles of the
// launches they replace).  A workgroup holds a tile grown by a halo of 2 nu cells in an LDS array of LEG_R^3 cells.
constexpr int LEG_R = 16;
struct AbecLegPlan {
    bool on = false;              // the level takes legs
    int mode = 0;                 // coefficients: 0 stored face arrays, 2 the constants bu
    int tile_down[3] = {0, 0, 0}, tile_up[3] = {0, 0, 0};     // tile lengths of the two launches
    int halo_down = 0, halo_up = 0;                           // 2 nu1, 2 nu2
};
// THE decision for level `level` (>= 1) of a hierarchy, a sibling of abec_smooth_plan (host data only): one component, no tensor solve, no
// coarse/fine faces, one box spanning a fully periodic domain and held by this rank, stored or uniform coefficients, no slab /
// agglomeration transition to the next level, nu1, nu2 >= 1 with the grown tile inside the LDS array, at most IAMRX_MG_LEGS_MAX_CELLS
// cells, IAMRX_MG_LEGS (1) on.  The caller adds what only the hierarchy knows (not the coarsest level, no fused tail, no sweep-only solve).
AbecLegPlan abec_leg_plan(const Geometry& g, const AbecLevel& lv, int level, int nu1, int nu2, bool slab_transition, bool agg_transition);
// buf = S^nu1(0) on the level, crse_rhs = R(rhs - A buf); c: the level's coefficients
void abec_leg_down(const Geometry& g, const AbecCoef& c, const AbecLegPlan& p, MultiFab& buf, const MultiFab& rhs, MultiFab& crse_rhs, int nu1, double omega);
// cor = S^nu2(buf + P crse_cor)
void abec_leg_up(const Geometry& g, const AbecCoef& c, const AbecLegPlan& p, MultiFab& cor, const MultiFab& buf, const MultiFab& rhs, const MultiFab& crse_cor, int nu2,
                 double omega);
// restriction of the residual rhs - A phi straight onto the coarsened layout (one pass, the fine residual is not stored): usable if ..._ok
bool abec_residual_reads_no_ghosts(const Geometry& g, const AbecCoef& c, const MultiFab& out, const MultiFab& phi, const MultiFab& rhs, bool restrict_form);
bool abec_resid_restrict_ok(const AbecCoef& c, const MultiFab& phi, const MultiFab& rhs);
void abec_resid_restrict(const Geometry& g, const AbecCoef& c, MultiFab& crse, const MultiFab& phi, const MultiFab& rhs);
// one red + black sweep in ONE launch, out of place (pin -> pout), on a level that is one box spanning its domain (k_abec_gsrb_rb: the
// doubles of the two colour passes, a third of their HBM traffic); zero: pin is identically zero and is not read.  p: RB_BOX, or RB_CF
// with cf, the level's coarse/fine ghost formula, evaluated inside the kernel (a refined box strictly inside its domain)
// (acc: pout is the SOLUTION of the running solve and receives pout + the swept correction -- the last sweep of a V-cycle, k_abec.hip ACC)
void abec_gsrb_rb(const Geometry& g, const AbecCoef& c, const AbecSmoothPlan& p, const MultiFab& pin, MultiFab& pout, const MultiFab& rhs, double omega,
                  bool zero, const DomainBC* bcs = nullptr, int nbc = 0, const CfTab* cf = nullptr, bool acc = false);
// the same sweep on a level of several boxes that covers its domain (RB_NBR: a chopped level, the boxes of a sharded level): k_abec_rb_ghost +
// k_abec_gsrb_rb<.., NBR>, one two-layer ghost fill of phi per sweep in front of it (the caller's).
// sel 0: the whole sweep; 1: only the tiles that read no ghost cell (no k_abec_rb_ghost launch); 2: k_abec_rb_ghost + the other tiles
// (p.nbr_splits: parts 1 and 2 are both non-empty and the level has no ghost columns in x); on: the stream (null: the context's)
void abec_gsrb_rb_nbr(const Geometry& g, const AbecCoef& c, const AbecSmoothPlan& p, MultiFab& pin, MultiFab& pout, const MultiFab& rhs, double omega,
                      bool zero, const DomainBC* bcs, int nbc, int sel = 0, hipStream_t on = nullptr, bool acc = false);
// the planner's answer for the arrays at hand (the finest level of a hierarchy).  level_ok: for the widths the sweep on several boxes wants
// (phi two ghost layers, rhs and the a-term one, the density two), before the arrays exist
bool abec_gsrb_rb_ok(const Geometry& g, const AbecCoef& c, const MultiFab& phi, int nbc, const DomainBC* bcs = nullptr);
bool abec_gsrb_rb_cf_ok(const Geometry& g, const AbecCoef& c, const MultiFab& phi);
bool abec_gsrb_rb_nbr_ok(const Geometry& g, const AbecCoef& c, const MultiFab& phi, const MultiFab& rhs, int nbc, const DomainBC* bcs);
bool abec_gsrb_rb_nbr_level_ok(const Geometry& g, const Layout& l, int ncomp, bool sig_form, bool has_a, int nbc, const DomainBC* bcs);
// fused red+black sweep, out of place; see k_abec.hip (the caller refreshes the ghosts of phi_out and finishes the black cells
// on box surfaces with abec_gsrb(..., 1, ..., shell_only = true))
void abec_gsrb_fused(const Geometry& g, const AbecCoef& c, const MultiFab& phi_in, MultiFab& phi_out, const MultiFab& rhs, double omega,
                     const DomainBC* bcs, int nbc);
// out = rhs - L(phi)  (rhs == nullptr: out = L(phi))
void abec_residual(const Geometry& g, const AbecCoef& c, MultiFab& out, const MultiFab& phi, const MultiFab* rhs, double* norm_out = nullptr);
// bottom solve (BiCGStab + post-smoothing, CellMG::bottom_solve) of a single-box level of at most 8^3 cells in one single-workgroup launch
bool abec_bottom_device_ok(const Geometry& g, const Layout& l, const DomainBC* bcs, int nbc, int ncomp, bool cf = false);
void abec_bottom_solve(const Geometry& g, const AbecCoef& c, MultiFab& cor, const MultiFab& res, const DomainBC& bc, bool singular,
                       double eps_rel, int maxiter, int nub, int nuf, double omega, int* d_iters, const CfTab* cftab = nullptr);
void abec_apply_domain_bc(const Geometry& g, MultiFab& phi, const DomainBC& bc, bool inhomog, const MultiFab* bcval, int comp0 = 0, int ncomp = -1);
void abec_apply_domain_bc_percomp(const Geometry& g, MultiFab& phi, const DomainBC* bcs, int ncomp, bool inhomog, const MultiFab* bcval);
void cc_restrict(MultiFab& crse, const MultiFab& fine);          // average of 8
void cc_prolong_add(MultiFab& fine, const MultiFab& crse);       // piecewise constant
void face_avgdown(MultiFab& crse, const MultiFab& fine, int dir);
// flux_d = -beta*b_d*dphi/dx_d ; if add_to != nullptr: add_to[d] += flux_d instead of storing
void abec_flux(const Geometry& g, const AbecCoef& c, const MultiFab& phi, MultiFab* const flux[3], MultiFab* const add_to[3]);
// rhs = S - div(umac); sum != null: also rhs.sum_unique(g, 0), its bits, out of the same pass (k_basic.hip)
void mac_rhs(const Geometry& g, MultiFab& rhs, const MultiFab* const umac[3], const MultiFab* S, double* sum = nullptr);
void mac_bcoef(MultiFab* const b[3], const MultiFab& rho, int rho_comp, double scale);                 // b = scale / avg_face(rho)
// the same doubles without the arrays b: crse = face_avgdown of mac_bcoef(rho) in direction dir; abec_flux (one component) in one launch
void mac_bcoef_avgdown(MultiFab& crse, const MultiFab& rho, int rho_comp, double scale, int dir);
void abec_flux_sig(const Geometry& g, double beta, const MultiFab& rho, int rho_comp, double scale, const MultiFab& phi, MultiFab* const flux[3],
                   MultiFab* const add_to[3]);
void mac_divergence(const Geometry& g, MultiFab& div, const MultiFab* const umac[3]);

// ---- k_godunov.hip ------------------------------------------------------------------------
// Godunov::ExtrapVelToFaces (PLM): vel has >=3 comps and >=3 filled ghost cells, force 3 comps >=1 ghost
// scheme: ns.advection_scheme, 0 Godunov_PLM (4th-order limited slopes), 1 Godunov_PPM -- an argument of every call, no process-wide mode
void godunov_extrap_vel_to_faces(const Geometry& g, const MultiFab& vel, const MultiFab* force, MultiFab* const umac[3],
                                 double dt, const BCRec* bc, bool use_forces_in_trans, int scheme = 0);
// ComputeFluxesOnBoxFromState + ComputeDivergence(-1) + ComputeConvectiveTerm, aofs(acomp..) = -update.
// S: ncomp comps, >=3 ghosts; umac: >=1 ghost (filled); force/divu: >=1 ghost or null
void godunov_compute_aofs(const Geometry& g, MultiFab& aofs, int acomp, const MultiFab& S, int ncomp, const MultiFab* force,
                          const MultiFab* divu, MultiFab* const umac[3], const int* iconserv, double dt, const BCRec* bc,
                          bool is_velocity, bool use_forces_in_trans, MultiFab* const edge_out[3], MultiFab* const flux_out[3], int scheme = 0);
// host data only: the launches a call of the fused kernels (pred: k_pred_z, else k_god_z) would issue on these boxes, and their tiles --
// god_z_plan and god_tile_lists_host flattened for iamrx_host_godunov_plan (layout of the outputs: at the definition)
void godunov_plan_host(bool pred, const std::vector<BoxD>& boxes, const Geometry& g, int scheme, bool has_force, bool fit, bool has_divu, bool edge_out,
                       bool flux_out, int ncomp, const int* iconserv, int head[5], std::vector<int>& launch, std::vector<int>& starts, std::vector<int>& tiles);


// ---- k_nodal.hip --------------------------------------------------------------------------
// Image reading (residual: x, restriction: fine): the array's level is one box spanning its domain (nodal_wrap_or_reflect_ok), so a node
// outside the box is the periodic image -- in the directions of refl (bit d): the mirror image about the Neumann wall -- of a valid node.
// on: the kernel reads that node instead of the ghost node, which then needs no fill (FillBoundary + nodal_reflect_bc); the same doubles.
struct NodalImages { bool on = false; int refl = 0; };
bool nodal_residual(const Geometry& g, MultiFab& out, const MultiFab& x, const MultiFab& sig, const MultiFab* rhs, double* norm_out = nullptr,
                    const NodalImages& img = NodalImages());
void nodal_gs_color(const Geometry& g, MultiFab& x, const MultiFab& rhs, const MultiFab& sig, int color, const MultiFab* dmask = nullptr);
// ---- the smoother and bottom path of a nodal multigrid level ----
// What the choice rests on, as host data (no array, no device).  boxes is the level's GLOBAL box list; max_len / nlocal: Layout's (max_len
// is the largest LOCAL extent).  has_mask: the level has a Dirichlet mask, as wide as the correction.
struct NodalLevel {
    const std::vector<BoxD>* boxes = nullptr;
    int nlocal = 0, max_len[3] = {0, 0, 0};
    const DomainBC* bc = nullptr;
    int cor_ngrow = 0, rhs_ngrow = 0;                      // ghost widths: correction, right-hand side (the level's residual)
    bool has_mask = false;
    int nodal_smoother = 0, bottom_smoother_only = 0, device_bottom = 1, nodal_sweeps = 2;      // MGOpts
    bool coarsest = false;
};
struct NodalSmoothPlan {
    // JACOBI; COLOUR8: eight colour passes, each behind a ghost fill; SMALL: every sweep of the call in one single-workgroup launch
    // (k_nodal_smooth_small); GS4 / GSR: two plane-fused passes per sweep (k_nodal_gs4 / the register-resident k_nodal_gsr)
    enum Path { JACOBI, COLOUR8, SMALL, GS4, GSR } path = COLOUR8;
    // how the coarsest level is solved (NONE: not the coarsest): nuf smoothing calls; k_nodal_bottom (fully periodic); k_nodal_bottom_g
    // (walls / Dirichlet mask / refined patch); BiCGStab driven from the host
    enum Bottom { NONE, SMOOTHER_ONLY, DEVICE_PERIODIC, DEVICE_GENERAL, HOST_KRYLOV } bottom = NONE;
    int ngrow = 1;                // what the correction, the residual, sigma and the mask are allocated with (4: the fused passes recompute their halo)
    bool wrap = false;            // one box spanning its domain, no Dirichlet nodes: the fused passes read images instead of ghost nodes -- periodic
    int refl = 0;                 // ones, or mirror images about Neumann walls in the directions of refl (bit d); no ghost fill in front of a pass
    bool images = false;          // ... and so do the residual and the restriction: no ghost fill inside a cycle (NodalImages)
    bool written_first = false;   // every array of the level is written before it is read: no zero fill behind the allocation
    bool zero_start = false;      // the first sweep of a call on a zero correction is told so instead of the correction being set to zero
    bool par_fill = false;        // in front of a pass, only the ghost nodes of the planes of the parity it reads are refreshed
    bool splits = false;          // GSR: a pass behind a ghost fill can be issued in two parts (tiles that read no ghost node / the others)
    int sweeps = 2;               // Gauss-Seidel sweeps (Jacobi steps) per smoothing call
    int cor_ngrow = 0, rhs_ngrow = 0;      // what the plan was made for (the launchers assert it)
    bool fused() const { return path == GS4 || path == GSR; }
    static bool on_device(Bottom b) { return b == DEVICE_PERIODIC || b == DEVICE_GENERAL; }       // single-workgroup launch, no host synchronisation
    NodalImages img() const { return NodalImages{images, images ? refl : 0}; }
    bool made_for(const MultiFab& x, const MultiFab& rhs) const { return x.ngrow == cor_ngrow && rhs.ngrow == rhs_ngrow; }
};
// THE decision: how a smoothing call and the bottom solve run on this level, made once per level per solve
NodalSmoothPlan nodal_smooth_plan(const Geometry& g, const NodalLevel& lv);
// the ghost width every plan asks for (IAMRX_NODAL_FUSED), before a level's arrays and mask exist
int nodal_plan_ngrow();
// the bottom part alone (what the plan of a coarsest level says): the hierarchy stops coarsening at the first level whose kind, without a
// mask, is a device kind
NodalSmoothPlan::Bottom nodal_bottom_kind(const Geometry& g, const NodalLevel& lv);
// the fused-pass part alone (GS4 or GSR), for a caller that fills the ghost nodes itself or vouches for the index wrap
NodalSmoothPlan nodal_pass_form(const MultiFab& x, const MultiFab& rhs, bool wrap = false);
// one k-parity pass of the plane-fused 8-colour GS (arrays need ngrow >= 4 / 3), out of place: plane k from xc, planes
// k+-1 from xn, result to xo (xo != xc; xn may be either).  p: the level's plan (GS4 / GSR, wrap, refl).  zero_flags (GSR only): bit 0: xc,
// bit 1: xn is identically zero and is not read
// sel (GSR only): 1 = the tiles that read no ghost node of x (footprint and planes inside the box), 2 = the others, 0 = all; on: the
// stream of the launch (null: the context's)
void nodal_gs_fused_pass(const Geometry& g, const NodalSmoothPlan& p, const MultiFab& xc, const MultiFab& xn, MultiFab& xo, const MultiFab& rhs,
                         const MultiFab& sig, int kpar, const MultiFab* dmask = nullptr, const double* csig = nullptr, int zero_flags = 0,
                         int sel = 0, hipStream_t on = nullptr);
void nodal_zero_masked(MultiFab& mf, const MultiFab& dmask);
void nodal_build_dmask(const Geometry& g, MultiFab& dm, const MultiFab& cov, const DomainBC& bc);
bool periodic_wrap_ok(const Geometry& g, const Layout& l, int min_len);
bool nodal_wrap_or_reflect_ok(const Geometry& g, const Layout& l, const DomainBC& bc, int min_len, int* refl);
// all sweeps x 8 colours of a small single-box periodic level in one single-workgroup launch (false: not applicable)
bool nodal_smooth_small(const Geometry& g, MultiFab& x, const MultiFab& rhs, const MultiFab& sig, int nsweeps);
void nodal_jacobi(const Geometry& g, MultiFab& xnew, const MultiFab& x, const MultiFab& rhs, const MultiFab& sig, const MultiFab* dmask = nullptr);
void nodal_restrict(MultiFab& crse, const MultiFab& fine, const NodalImages& img = NodalImages());
void nodal_interp_add(MultiFab& fine, const MultiFab& crse, const MultiFab& sig_fine);
void nodal_divu(const Geometry& g, MultiFab& rhs, const MultiFab& vel, int vcomp, const DomainBC* bc);
// vel(vcomp..) -= sig*grad(phi) (vel may be null); gp (may be null) = or += grad(phi)
// vel_scale: the velocity is stored times this factor (the caller's scaling pass over the valid cells, folded in)
void nodal_mknewu(const Geometry& g, MultiFab* vel, int vcomp, const MultiFab& phi, const MultiFab* sig, MultiFab* gp, bool gp_increment, double vel_scale = 1.0);

// ---- k_tensor.hip -------------------------------------------------------------------------
void tensor_bcoef(MultiFab& b3, const MultiFab& eta, int dir);
// extensive face fluxes of the tensor operator (Diffusion::computeExtensiveFluxes): fac * area * (-eta (4/3) du_n/dx_d + cross terms)
void tensor_extensive_flux(const Geometry& g, const MultiFab& vel, const MultiFab* const eta[3], MultiFab* const flux[3], double fac, bool add);
void tensor_cross_terms_sub(const Geometry& g, const AbecCoef& c, MultiFab& out, const MultiFab& vel, double sign, unsigned long long* normout = nullptr);
void fill_tensor_corners(const Geometry& g, MultiFab& phi, const DomainBC& bc, bool inhomog, const MultiFab* bcval, int comp0 = 0, int ncomp = -1);

// ---- k_les.hip ----------------------------------------------------------------------------
// LES eddy viscosity on faces, one launch: mu[d] (face d, comp 0) = base + mu_t of model 0 (Smagorinsky) / 1 (Sigma) with constant Cs, from
// the velocity in vel(vcomp .. vcomp + 2) and its ghost cells as they are (one layer, face and edge cells): the model loops of
// NavierStokesBase::calc_mut_LES (Source/NS_LES.cpp:105-222) on the gradients of MLTensorOp::compVelGrad (:97)
void les_mut(const Geometry& g, const MultiFab& vel, int vcomp, int model, double Cs, double base, MultiFab* const mu[3]);

// ---- k_turb.hip ---------------------------------------------------------------------------
// Turbulent forcing (Tutorials/HIT): the table of M Fourier modes -- integer wavevector and the 17 values FTX, TAT, FPX, FPY, FPZ, FAX, FAY,
// FAZ, FPXX, FPXY, FPXZ, FPYX, FPYY, FPYZ, FPZX, FPZY, FPZZ per mode -- shared by the levels of a hierarchy
struct TurbTable {
    int M = 0, div_free = 1;
    std::vector<int> kxyz;                      // [3 m + d]
    std::vector<double> data;                   // [17 m + q]
    mutable int* d_kxyz = nullptr;              // device copy, made by the first evaluation
    mutable double* d_data = nullptr;
    ~TurbTable();
};
using TurbTableP = std::shared_ptr<const TurbTable>;
// host only: TurbulentForcing::init_turbulent_forcing (Tutorials/HIT/TurbulentForcing_def.H:21-366) as the list of the modes its loops write
void turb_host_modes(const double problo[3], const double probhi[3], int nmodes, int mode_start, int div_free, std::vector<int>& kxyz, std::vector<double>& data);
TurbTableP turb_make_table(const Geometry& g, int nmodes, int mode_start, int div_free);
TurbTableP turb_make_table(int M, const int* kxyz, const double* data, int div_free);      // a caller's table
// out(ocomp .. ocomp + 2) = the acceleration f(x, time) of NS_getForce.cpp:553-686 on the cells and every ghost cell of out
void turb_force(const Geometry& g, const TurbTable& tt, double time, MultiFab& out, int ocomp);

}  // namespace iamrx
