// iamr_amd/csrc/nodalmg.hip -- nodal multigrid driver (MLMG on MLNodeLaplacian semantics) over the HIP
// kernels of k_nodal.hip.  Reference call site: Source/Projection.cpp:2512-2542 (NodalProjector::project
// with Gauss-Seidel on, harmonic average off, max_fmg_iter 0, proj_tol 1e-12 / sync_tol 1e-10).
#include "mlmg.h"
#include "launch.h"
#include "krylov.h"
#include <chrono>
#include <cmath>
#include <cstdlib>

namespace iamrx {

// kernels (k_nodal.hip)
void nodal_interp_add(MultiFab& fine, const MultiFab& crse, const MultiFab& sig_fine);

void nodal_bottom_solve(const Geometry& g, MultiFab& cor, const MultiFab& res, const MultiFab& sig, bool singular, double eps_rel, int maxiter,
                        int nsweeps, int nub, int nuf, int* d_iters);
void nodal_bottom_solve_general(const Geometry& g, MultiFab& cor, const MultiFab& res, const MultiFab& sig, const MultiFab* dmask, bool singular,
                                double eps_rel, int maxiter, int nsweeps, int nub, int nuf, int* d_iters);
// unique nodes of a level: the unknowns behind the Krylov iteration cap (krylov_maxiter)
static long nodal_unknowns(const Geometry& g)
{
    long n = 1;
    for (int d = 0; d < 3; ++d) n *= g.domain.len(d) + (g.periodic[d] ? 0 : 1);
    return n;
}

NodalMG::NodalMG(const Geometry& g, LayoutP layout, const DomainBC& bc_in, const MGOpts& o) : m_g(g), m_bc(bc_in), m_o(o)
{
    ProfScope ps_prof_("nmg_ctor");
    // the operator does not distinguish inflow faces from walls (the difference is in div(u), nodal_divu)
    for (int d = 0; d < 3; ++d) { if (m_bc.lo[d] == lo_inflow) m_bc.lo[d] = lo_neumann; if (m_bc.hi[d] == lo_inflow) m_bc.hi[d] = lo_neumann; }
    const DomainBC& bc = m_bc;
    for (int d = 0; d < 3; ++d) {
        if (!g.periodic[d])
            for (int t : {bc.lo[d], bc.hi[d]})
                if (t != lo_neumann && t != lo_dirichlet) throw Error("iamrx NodalMG: domain boundaries must be periodic, Neumann (wall / inflow) or Dirichlet (outflow)");
        // Neumann-wall nodes carry weight 1/2 in sums and dot products (doubled rows, MLNodeLinOp dot mask)
        m_g.half_lo[d] = (!g.periodic[d] && bc.lo[d] == lo_neumann) ? 1 : 0;
        m_g.half_hi[d] = (!g.periodic[d] && bc.hi[d] == lo_neumann) ? 1 : 0;
    }
    m_lev.resize(1);
    m_lev[0].g = m_g;
    m_lev[0].layout = std::move(layout);
    while ((int)m_lev.size() <= m_o.max_coarsening_level) {
        Level& f = m_lev.back();
        // a single box of at most 8^3 cells is solved by a single-workgroup device bottom solver (k_nodal_bottom / k_nodal_bottom_g): the
        // coarsest level (the Dirichlet masks do not exist yet: the kind without one)
        if (NodalSmoothPlan::on_device(nodal_bottom_kind(f.g, describe(f, true, false, 0)))) break;
        Level c;
        if (!mg_coarsen_level(f, m_o, c)) break;     // (mlmg.hip: isotropic, slab or agglomerated level)
        m_lev.push_back(std::move(c));
    }
    // Dirichlet nodes: on Dirichlet (outflow) domain faces and on the boundary of a level that does not cover the domain
    // (coarse/fine boundary of an AMR level).  They keep their value, carry no residual and take no correction.
    bool need_mask = false;
    for (int d = 0; d < 3; ++d) if (!g.periodic[d] && (bc.lo[d] == lo_dirichlet || bc.hi[d] == lo_dirichlet)) need_mask = true;
    if (m_lev[0].layout->total_cells() != g.domain.npts()) need_mask = true;
    // (4 ghost layers where the plane-fused Gauss-Seidel is on: it recomputes its halo instead of exchanging it per colour)
    const int ng = nodal_plan_ngrow();
    for (auto& L : m_lev) {
        if (L.agg) L.tmp_d.define(L.dist, node_type(), 1, 1);
        if (L.slab) L.vres.define(L.virt, node_type(), 1, 0);
        L.sig.define(L.layout, cell_type(), 1, ng);
        L.cor.define(L.layout, node_type(), 1, ng);
        L.res.define(L.layout, node_type(), 1, ng);
        L.rescor.define(L.layout, node_type(), 1, 1);
    }
    for (auto& L : m_lev) {
        if (!need_mask) break;
        MultiFab cov(L.layout, cell_type(), 1, 1);
        cov.setVal(0.0);
        mf_add_scalar(cov, 1.0, 0, 1, 0);
        cov.FillBoundary(L.g);
        L.dm.define(L.layout, node_type(), 1, ng);
        L.dm.setVal(1.0);                                  // ghost nodes outside the level: never updated
        nodal_build_dmask(L.g, L.dm, cov, m_bc);
        if (L.dm.norm0(0, 1, 0) == 0.0) L.dm = MultiFab();
        else {
            m_masked = true;
            L.dm.FillBoundary(L.g);
            nodal_reflect_bc(L.g, L.dm, m_bc);
        }
    }
    if (m_masked) {
        m_singular = false;
        for (auto& L : m_lev) IAMRX_ASSERT(L.dm.defined());
    }
    const int ov_mode = (int)tune("HALO_OVERLAP", 1);
    for (auto& L : m_lev) {
        // how the level is smoothed and -- the coarsest -- solved: decided here, once the masks exist (kernels.h)
        L.plan = nodal_smooth_plan(L.g, describe(L, &L == &m_lev.back(), L.dm.defined(), ng));
        const NodalSmoothPlan& p = L.plan;
        IAMRX_ASSERT(p.ngrow == ng && p.made_for(L.cor, L.res));
        // Overlap (IAMRX_HALO_OVERLAP as for the cell-centred sweep, CellMG::smooth_n; round 6): a pass of k_nodal_gsr whose ghost nodes have
        // to be refreshed first is issued in two parts -- the tiles whose footprint and planes lie inside their box on the main stream; the
        // exchange, the wall reflection and the remaining tiles on the context's side stream behind a fork -- and joined: the messages
        // travel while the interior tiles run.  The two parts write disjoint nodes; the same doubles as the one-piece pass.
        if (p.splits && ov_mode != 0) {
            const int ngv[3] = {ng, ng, 1};
            // (the plans are built and uploaded here, in front of any fork)
            bool peers = false;
            for (int kp = -1; kp <= 1; ++kp) peers = !fill_boundary_plan(*L.layout, node_type(), ng, L.g, ngv, kp).peers.empty() || peers;
            L.overlap = ov_mode == 2 || peers;
        }
        // The zero fills below give a value to what nobody writes: ghost cells beyond a coarse/fine boundary (setSigma fills valid cells,
        // neighbours / periodic images and wall mirrors; the prolongation forms sigma-weighted averages at the masked boundary nodes before
        // they are zeroed: keep them finite) and ghost nodes outside the level.  A level without Dirichlet nodes that is one box spanning
        // its domain (plan.wrap) and goes to k_nodal_gsr has neither: its kernels read valid data and the ghost layers fillbc /
        // setSigma fill completely; sig and res are written (copy / residual / restriction) before they are read, rescor by the residual,
        // and cor starts from zero inside the first sweep or is zeroed by smooth() / vcycle().  There the four fills are skipped
        // (plan.written_first, IAMRX_NODAL_SKIP_FILLS; IAMRX_POISON_ALLOC = 1 / 2 must not change a result).
        if (p.written_first) continue;
        L.sig.setVal(0.0);
        L.cor.setVal(0.0); L.res.setVal(0.0); L.rescor.setVal(0.0);
    }
}

// the level as nodal_smooth_plan / nodal_bottom_kind see it
NodalLevel NodalMG::describe(const Level& L, bool coarsest, bool has_mask, int ng) const
{
    NodalLevel lv;
    lv.boxes = &L.layout->boxes; lv.nlocal = L.layout->nlocal();
    for (int d = 0; d < 3; ++d) lv.max_len[d] = L.layout->max_len[d];
    lv.bc = &m_bc;
    lv.cor_ngrow = lv.rhs_ngrow = ng;
    lv.has_mask = has_mask;
    lv.nodal_smoother = m_o.nodal_smoother; lv.bottom_smoother_only = m_o.bottom_smoother_only; lv.device_bottom = m_o.device_bottom;
    lv.nodal_sweeps = m_o.nodal_sweeps;
    lv.coarsest = coarsest;
    return lv;
}

void NodalMG::setSigma(const MultiFab& sig, int comp)
{
    ProfScope ps_prof_("nmg_setsigma");
    MultiFab::Copy(m_lev[0].sig, sig, comp, 0, 1, 0);
    m_lev[0].sig.FillBoundary(m_lev[0].g);
    cc_mirror_bc(m_lev[0].g, m_lev[0].sig);                // mlndlap_fillbc_cc: mirror sigma across walls
    for (size_t l = 1; l < m_lev.size(); ++l) {
        // arithmetic average (harmonic averaging off); agglomerated level: on its distributed form, then gathered; slab level: onto the
        // one-plane virtual level, duplicated
        {
            Level& C = m_lev[l];
            MultiFab sd, sv;
            if (C.agg) sd.define(C.dist, cell_type(), 1, 0);
            if (C.slab) sv.define(C.virt, cell_type(), 1, 0);
            mg_restrict_to(C, C.sig, sd, sv, [&](MultiFab& target) { cc_restrict(target, m_lev[l - 1].sig); });
        }
        m_lev[l].sig.FillBoundary(m_lev[l].g);
        cc_mirror_bc(m_lev[l].g, m_lev[l].sig);
    }
    // Constant sigma (constant-density flow, the common IAMR case): every coarsened level then holds the same constant (the average
    // of 8 equal numbers is exact) and periodic / mirrored ghost cells too, so the smoother can take sigma from a register instead
    // of staging two sigma planes per node plane.  Same expression tree => bit-identical results.  IAMRX_NODAL_CSIG=0 disables.
    const bool csig_on = tune("NODAL_CSIG", 1) != 0;
    m_csig = false;
    if (csig_on && !m_masked) {
        // (largest and smallest value in one pass and one read-back: sigma changes with every projection, the test runs in front of each)
        double smin, smax;
        reduce_minmax(m_lev[0].sig, 0, 0, smin, smax);
        if (smax > 0.0 && smin == smax) { m_csig = true; m_csig_val = smax; }
    }
}

// ghost nodes: same-level + periodic images, then even reflection about Neumann walls
void NodalMG::fillbc(int l, MultiFab& x, int kpar, hipStream_t on)
{
    // the plane-fused smoother recomputes a 4-node halo in-plane but reaches only one plane up and down: exchange 1 plane in z
    const int ngv[3] = {x.ngrow, x.ngrow, 1};
    x.FillBoundary(m_lev[l].g, 0, x.ncomp, ngv, kpar, on);
    nodal_reflect_bc(m_lev[l].g, x, m_bc, on);
}

// one smoothing call (plan.sweeps sweeps) on the level's correction with its residual as right-hand side, as the level's plan says
void NodalMG::smooth(int l, bool x_is_zero, bool leave_ghosts)
{
    Level& L = m_lev[l];
    const NodalSmoothPlan& p = L.plan;
    MultiFab& x = L.cor;
    const MultiFab& rhs = L.res;
    const MultiFab* dmk = L.dmask();
    // a correction that starts from zero: on a level the register-resident kernel smooths (plan.zero_start) the first sweep is told so and
    // reads no x -- the zero fill and a third of the first sweep's traffic; everywhere else x is zeroed here (with index wrap or on
    // ghost-filled boxes, with or without a Dirichlet mask: the ghost nodes of a zero array are zero as well -- images, reflections at
    // walls -- so the fill in front of the first pass goes too)
    const bool zero_start = x_is_zero && p.zero_start;
    if (x_is_zero && !zero_start) x.setVal(0.0);
    if (p.path == NodalSmoothPlan::SMALL) {
        const bool took = nodal_smooth_small(L.g, x, rhs, L.sig, p.sweeps);
        IAMRX_ASSERT(took);
        if (!p.images) fillbc(l, x);          // (the kernel writes the periodic duplicates itself)
        return;
    }
    if (p.fused()) {
        // colours 0-3 (k even) in one pass, colours 4-7 (k odd) in a second one: identical arithmetic to the eight
        // sequential colour passes below.  Each sweep goes from one buffer to the other (see k_nodal_gs4).
        if (!L.xb.defined()) L.xb.define(L.layout, node_type(), 1, x.ngrow);
        // the right-hand side is unchanged within a V-cycle: fill its ghosts once (plan.wrap: the kernel takes images from the valid data)
        if (!p.wrap && !L.res_filled) { fillbc(l, L.res); L.res_filled = true; }
        MultiFab* a = &x;
        MultiFab* b = &L.xb;
        // Ghost traffic: the even pass changes even planes only and reads the odd planes next to them, the odd pass the reverse.
        // After the first (full) fill it is therefore enough to refresh the ghost nodes of the planes of ONE parity in front of each
        // pass (plan.par_fill): the odd planes before the even pass, the even planes before the odd pass (half the halo volume; on boxes
        // stacked in z, where one ghost plane is exchanged, every second message disappears).
        auto& ctx = Context::get();
        auto pass = [&](MultiFab& filled, int fill_kpar, bool do_fill, const MultiFab& xc_, const MultiFab& xn_, MultiFab& xo_, int kpar, int zf) {
            const double* cs = m_csig ? &m_csig_val : nullptr;
            if (do_fill && L.overlap) {          // in two parts around the exchange (NodalMG ctor)
                ctx.fork_side();
                nodal_gs_fused_pass(L.g, p, xc_, xn_, xo_, rhs, L.sig, kpar, dmk, cs, zf, 1, ctx.stream);
                fillbc(l, filled, fill_kpar, ctx.side);
                nodal_gs_fused_pass(L.g, p, xc_, xn_, xo_, rhs, L.sig, kpar, dmk, cs, zf, 2, ctx.side);
                ctx.join_side();
                return;
            }
            if (do_fill) fillbc(l, filled, fill_kpar);
            nodal_gs_fused_pass(L.g, p, xc_, xn_, xo_, rhs, L.sig, kpar, dmk, cs, zf);
        };
        for (int ns = 0; ns < p.sweeps; ++ns) {
            const bool z = zero_start && ns == 0;
            // even planes: a -> b (ghost nodes of a refreshed first: all planes in front of the first sweep, then the odd ones)
            pass(*a, (ns == 0 || !p.par_fill) ? -1 : 1, !p.wrap && !z, *a, *a, *b, 0, z ? 3 : 0);
            // odd planes: centre from a, neighbours from b (the ghost images of b's new even planes first)
            pass(*b, p.par_fill ? 0 : -1, !p.wrap, *a, *b, *b, 1, z ? 1 : 0);
            std::swap(a, b);
        }
        if (a != &x) MultiFab::Copy(x, *a, 0, 0, 1, 0);
        // (a level of image readers: every later reader of x takes images; without index wrap each pass above fills what it reads)
        if (!leave_ghosts && !p.images) fillbc(l, x);
        return;
    }
    for (int ns = 0; ns < p.sweeps; ++ns) {
        if (p.path == NodalSmoothPlan::COLOUR8) {
            for (int color = 0; color < 8; ++color) {
                fillbc(l, x);
                nodal_gs_color(L.g, x, rhs, L.sig, color, dmk);
            }
        } else {
            if (!L.tmp.defined()) L.tmp.define(L.layout, node_type(), 1, 1);
            fillbc(l, x);
            nodal_jacobi(L.g, L.tmp, x, rhs, L.sig, dmk);
            MultiFab::Copy(x, L.tmp, 0, 0, 1, 0);
        }
    }
    fillbc(l, x);
}

void NodalMG::residual(int l, MultiFab& r, MultiFab& x, const MultiFab& b, double* norm, bool x_filled)
{
    const NodalImages img = m_lev[l].plan.img();
    if (!x_filled && !img.on) fillbc(l, x);
    const bool masked = (bool)m_lev[l].dmask();
    const bool have = nodal_residual(m_lev[l].g, r, x, m_lev[l].sig, &b, (norm && !masked) ? norm : nullptr, img);
    if (masked) nodal_zero_masked(r, m_lev[l].dm);
    if (norm && !have) *norm = r.norm0(0, 1, 0);
}

void NodalMG::subtract_mean(int l, MultiFab& mf)
{
    const Geometry& g = m_lev[l].g;
    double cnt = 1.0;
    for (int d = 0; d < 3; ++d) cnt *= (double)g.domain.len(d);   // sum of weights: n unique nodes (periodic) or (n-1) + 2*(1/2) (walls)
    const double s = mf.sum_unique(g, 0);
    mf_add_scalar(mf, -s / cnt, 0, 1, 0);
}

// krylov.h: the initial residual and the operator application of the level, handed to the loop both solvers share
int NodalMG::bicgstab(int l, MultiFab& sol, const MultiFab& rhs, double eps_rel, double eps_abs, int& niters)
{
    Level& L = m_lev[l];
    return bottom_bicgstab(L.layout, node_type(), 1, L.g, sol, nodal_unknowns(L.g), m_o.bottom_maxiter, eps_rel, eps_abs,
                           [&](MultiFab& r) { residual(l, r, sol, rhs); },
                           [&](MultiFab& out, MultiFab& in) {
                               fillbc(l, in);
                               nodal_residual(L.g, out, in, L.sig, nullptr);
                               if (L.dmask()) nodal_zero_masked(out, L.dm);
                           }, niters);
}

void NodalMG::vcycle(MGStats& st)
{
    const int nl = (int)m_lev.size();
    for (int l = 0; l < nl - 1; ++l) {
        Level& L = m_lev[l];
        if (m_o.nodal_nu1 <= 0) L.cor.setVal(0.0);
        for (int i = 0; i < m_o.nodal_nu1; ++i) smooth(l, i == 0);
        residual(l, L.rescor, L.cor, L.res, nullptr, m_o.nodal_nu1 > 0);          // (smooth() has just filled the ghost nodes, or the level reads images: no fill)
        Level& C = m_lev[l + 1];
        const NodalImages rimg = (!C.slab && !C.agg) ? L.plan.img() : NodalImages();
        if (!rimg.on) fillbc(l, L.rescor);
        mg_restrict_to(C, C.res, C.tmp_d, C.vres, [&](MultiFab& target) { nodal_restrict(target, L.rescor, rimg); });
        m_lev[l + 1].res_filled = false;
        if (m_lev[l + 1].dmask()) nodal_zero_masked(m_lev[l + 1].res, m_lev[l + 1].dm);   // mlndlap_restriction: 0 on Dirichlet nodes
    }
    {
        const int l = nl - 1;
        Level& B = m_lev[l];
        B.cor.setVal(0.0);
        const int maxiter = krylov_maxiter(m_o.bottom_maxiter, nodal_unknowns(B.g));
        switch (B.plan.bottom) {
        case NodalSmoothPlan::SMOOTHER_ONLY:
            for (int i = 0; i < m_o.nuf; ++i) smooth(l);
            break;
        case NodalSmoothPlan::DEVICE_PERIODIC:          // fully periodic: the wrap-only kernel
            nodal_bottom_solve(B.g, B.cor, B.res, B.sig, m_singular, m_o.bottom_reltol, maxiter, m_o.nodal_sweeps, m_o.nub, m_o.nuf,
                               mg_bottom_iters_dev());
            break;
        case NodalSmoothPlan::DEVICE_GENERAL:           // walls / Dirichlet mask / refined patch
            nodal_bottom_solve_general(B.g, B.cor, B.res, B.sig, B.dmask(), m_singular, m_o.bottom_reltol, maxiter, m_o.nodal_sweeps, m_o.nub,
                                       m_o.nuf, mg_bottom_iters_dev());
            break;
        default: {
            MultiFab rb(B.layout, node_type(), 1, 0);
            MultiFab::Copy(rb, B.res, 0, 0, 1, 0);
            if (m_singular) subtract_mean(l, rb);
            int nit = 0;
            const int ret = bicgstab(l, B.cor, rb, m_o.bottom_reltol, -1.0, nit);
            st.bottom_iters_total += nit;
            if (ret != 0) {
                B.cor.setVal(0.0);
                for (int i = 0; i < m_o.nuf; ++i) smooth(l);
            }
            const int nn = ret == 0 ? m_o.nub : m_o.nuf;
            for (int i = 0; i < nn; ++i) smooth(l);
        }
        }
    }
    for (int l = nl - 2; l >= 0; --l) {
        Level& L = m_lev[l];
        // (a level that was smoothed on the way up comes with its ghost nodes filled; the bottom level comes from its solver)
        // (the interpolation reads valid coarse nodes only, periodic duplicates included: the smoothers and the bottom kernels write them)
        if ((l + 1 == nl - 1 || m_o.nodal_nu2 <= 0) && !m_lev[l + 1].plan.images) fillbc(l + 1, m_lev[l + 1].cor);
        nodal_interp_add(L.cor, mg_correction_of(m_lev[l + 1], m_lev[l + 1].cor, 1), L.sig);
        if (L.dmask()) nodal_zero_masked(L.cor, L.dm);                  // mlndlap_interpadd: Dirichlet nodes take no correction
        // the finest level's correction is added to the solution node by node: nobody reads its ghost nodes
        for (int i = 0; i < m_o.nodal_nu2; ++i) smooth(l, false, l == 0 && i == m_o.nodal_nu2 - 1);
    }
}

void NodalMG::vcycle_correction(MultiFab& e, const MultiFab& r, MGStats& st)
{
    Level& L0 = m_lev[0];
    MultiFab::Copy(L0.res, r, 0, 0, 1, 0);
    if (L0.dmask()) nodal_zero_masked(L0.res, L0.dm);
    if (m_singular) subtract_mean(0, L0.res);
    L0.res_filled = false;
    vcycle(st);
    MultiFab::Copy(e, L0.cor, 0, 0, 1, 0);
    e.FillBoundary(L0.g);
    nodal_reflect_bc(L0.g, e, m_bc);
}

// the same on the solver's own arrays: the caller has written r to the valid nodes of res(0) and reads e from cor(0) (valid nodes + one
// layer of ghost nodes) -- no copy in, no copy out (the composite solver calls this once per level correction)
void NodalMG::vcycle_correction_inplace(MGStats& st)
{
    Level& L0 = m_lev[0];
    if (L0.dmask()) nodal_zero_masked(L0.res, L0.dm);
    if (m_singular) subtract_mean(0, L0.res);
    L0.res_filled = false;
    vcycle(st);
    const int ngv[3] = {1, 1, 1};
    L0.cor.FillBoundary(L0.g, 0, 1, ngv, -1);
    nodal_reflect_bc(L0.g, L0.cor, m_bc);
}

MGStats NodalMG::solve(MultiFab& phi, const MultiFab& rhs_in, double rtol, double atol, bool rhs_is_temporary)
{
    ProfScope ps_prof_("nmg_solve");
    auto& ctx = Context::get();
    MGStats st;
    st.nlevels = (int)m_lev.size();
    Level& L0 = m_lev[0];
    // the solve changes its right-hand side (Dirichlet nodes, mean): on a copy, unless the caller gives its array away
    const bool inplace = rhs_is_temporary && tune("NODAL_RHS_INPLACE", 1) != 0;
    MultiFab rhs_copy;
    if (!inplace) {
        rhs_copy.define(L0.layout, node_type(), 1, 0);
        MultiFab::Copy(rhs_copy, rhs_in, 0, 0, 1, 0);
    }
    MultiFab& rhs = inplace ? const_cast<MultiFab&>(rhs_in) : rhs_copy;
    if (L0.dmask()) nodal_zero_masked(rhs, L0.dm);
    if (m_singular) subtract_mean(0, rhs);
    residual(0, L0.res, phi, rhs, &st.resnorm0);
    L0.res_filled = false;
    st.rhsnorm0 = rhs.norm0(0, 1, 0);
    const double max_norm = st.rhsnorm0 >= st.resnorm0 ? st.rhsnorm0 : st.resnorm0;
    // a NaN or inf in the right-hand side or the initial residual (the norms report both as +inf) leaves nothing to converge to, and with
    // res_target = +inf every convergence test below would pass
    if (!std::isfinite(max_norm)) throw Error("iamrx nodal MLMG: the right-hand side or the initial residual is not finite");
    const double res_target = std::max(atol, std::max(rtol, 1.e-16) * max_norm);
    st.resnorm = st.resnorm0;
    if (m_o.verbose) printf("iamrx nodal MLMG: rhs %.6e resid0 %.6e levels %d (smoother path of the finest level %d, ghost width %d)\n",
                            st.rhsnorm0, st.resnorm0, st.nlevels, (int)L0.plan.path, L0.cor.ngrow);
    double vc_ms = 0.0;
    cycle_timer().used = 0;
    const bool bdev = NodalSmoothPlan::on_device(m_lev.back().plan.bottom);
    if (bdev) IAMRX_HIP_CHECK(hipMemsetAsync(mg_bottom_iters_dev(), 0, sizeof(int), ctx.stream));
    if (m_o.fixed_iters <= 0 && st.resnorm0 <= res_target) st.converged = 1;
    else {
        const int maxit = m_o.fixed_iters > 0 ? m_o.fixed_iters : m_o.max_iters;
        std::vector<double> hist;
        for (int iter = 0; iter < maxit; ++iter) {
            // see CellMG::solve: the mean of the residual of a singular system is removed in front of the first cycle only
            const bool all_per = L0.g.periodic[0] && L0.g.periodic[1] && L0.g.periodic[2] && !L0.dmask();
            // (levels with Neumann walls keep amrex::MLMG's per-iteration removal: ADVICE round 3)
            if (m_singular && (!all_per || tune("MG_RES_MEAN", 0) != 0)) { subtract_mean(0, L0.res); L0.res_filled = false; }
            cycle_timer().mark(ctx.stream);
            vcycle(st);
            cycle_timer().mark(ctx.stream);
            mf_saxpy(phi, 1.0, L0.cor, 0, 0, 1, 0);
            residual(0, L0.res, phi, rhs, &st.resnorm);
            L0.res_filled = false;
            st.iters = iter + 1;
            if (m_o.verbose) printf("iamrx nodal MLMG: iter %d resid %.6e\n", iter + 1, st.resnorm);
            if (m_o.fixed_iters <= 0 && st.resnorm <= res_target) { st.converged = 1; break; }
            if (!(st.resnorm < 1.e20 * max_norm)) throw Error("iamrx nodal MLMG: failing to converge (residual blow-up)");
            // stalled at the fp64 round-off floor just above the tolerance: see composite_project (amrns.hip); converged = 2
            hist.push_back(st.resnorm);
            if (m_o.fixed_iters <= 0 && mg_stalled_at_floor(hist, st.resnorm0, res_target, tune("MG_STALL_FAST", 1) != 0)) {
                st.converged = 2;
                fprintf(stderr, "iamrx nodal MLMG: WARNING: residual %.3e stalled at the round-off floor above the target %.3e after %d cycles; accepted (converged = 2)\n",
                        st.resnorm, res_target, st.iters);
                break;
            }
        }
        if (m_o.fixed_iters <= 0 && !st.converged) throw Error("iamrx nodal MLMG: failed to converge after max_iters");
    }
    vc_ms = cycle_timer().total_ms();          // the last residual norm has synchronised the stream
    if (st.iters > 0) st.vcycle_ms = vc_ms / st.iters;
    if (bdev && st.iters > 0) {
        int h = 0;
        IAMRX_HIP_CHECK(hipMemcpyAsync(&h, mg_bottom_iters_dev(), sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
        ctx.sync();
        st.bottom_iters_total = h;
    }
    fillbc(0, phi);
    return st;
}

}  // namespace iamrx
