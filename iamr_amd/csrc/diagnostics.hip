// iamr_amd/csrc/diagnostics.hip -- the host side of the diagnostics of named fields (derive / derive_fields, integrals, histograms, plane
// profiles, the three integrated quantities) for a level and a hierarchy: the field table (every name, its kind, who takes it), the
// resolver (names -> {array, component}) and ONE implementation of each diagnostic over a list of levels.
// Kernels: k_basic.hip (sums), k_hist.hip, k_profile.hip, k_stats.hip, k_velgrad.hip.
#include "operators.h"
#include "particles.h"
#include "launch.h"
#include "amrns.h"
#include <string_view>

namespace iamrx {

// ---- the field table
enum class FieldKind { State, Pointwise, Velgrad, VelAvg, ParticleCount };
enum FieldUse : unsigned { DERIVE = 1, FIELDS = 2, REDUCE = 4, ALL = 7 };      // derive(); derive_fields(); histogram, histogram2 and integrate
enum { TRACER2_SLOT = 5, TEMP_SLOT = 6 };      // state entries beyond Tracer: NavierStokes::Tracer2 / Temp say where they are (-1: absent)
enum { ENERGY, MAG_VORT, AVG_PRESSURE };
struct FieldEntry { std::string_view name; FieldKind kind; int id; unsigned uses; };          // (a view: a lookup compares the lengths first)
static const FieldEntry FIELD_TABLE[] = {
    {"x_velocity", FieldKind::State, Xvel, FIELDS | REDUCE}, {"y_velocity", FieldKind::State, Yvel, FIELDS | REDUCE},
    {"z_velocity", FieldKind::State, Zvel, FIELDS | REDUCE}, {"density", FieldKind::State, Density, FIELDS | REDUCE},
    {"tracer", FieldKind::State, Tracer, FIELDS | REDUCE}, {"tracer2", FieldKind::State, TRACER2_SLOT, FIELDS | REDUCE},
    {"temp", FieldKind::State, TEMP_SLOT, FIELDS | REDUCE},
    {"energy", FieldKind::Pointwise, ENERGY, ALL}, {"mag_vort", FieldKind::Pointwise, MAG_VORT, ALL}, {"avg_pressure", FieldKind::Pointwise, AVG_PRESSURE, ALL},
    {"velocity_average", FieldKind::VelAvg, 0, DERIVE},               // six components: derive() alone
    {"particle_count", FieldKind::ParticleCount, 0, DERIVE | FIELDS}, {"total_particle_count", FieldKind::ParticleCount, 1, DERIVE | FIELDS},
    // the ids of k_velgrad.hip, in their order
    {"diveru", FieldKind::Velgrad, 0, ALL}, {"vort_x", FieldKind::Velgrad, 1, ALL}, {"vort_y", FieldKind::Velgrad, 2, ALL}, {"vort_z", FieldKind::Velgrad, 3, ALL},
    {"enstrophy", FieldKind::Velgrad, 4, ALL}, {"strain_rate", FieldKind::Velgrad, 5, ALL}, {"dissipation", FieldKind::Velgrad, 6, ALL},
    {"q_criterion", FieldKind::Velgrad, 7, ALL}, {"r_invariant", FieldKind::Velgrad, 8, ALL}, {"helicity", FieldKind::Velgrad, 9, ALL},
};

int NavierStokes::state_comp(const FieldEntry& e) const { return e.id == TRACER2_SLOT ? Tracer2 : (e.id == TEMP_SLOT ? Temp : e.id); }

// the entry of a name that the entry point `use` takes and this run has; anything else is an error that lists the names it could have been
const FieldEntry& NavierStokes::find_field(const std::string& name, unsigned use, const char* who) const
{
    auto taken = [&](const FieldEntry& e) {
        return (e.uses & use) && !(e.kind == FieldKind::State && state_comp(e) < 0) && !(e.kind == FieldKind::VelAvg && !has_average()) &&
               !(e.kind == FieldKind::ParticleCount && !particles);
    };
    for (const FieldEntry& e : FIELD_TABLE) if (name == e.name && taken(e)) return e;
    std::string known;
    for (const FieldEntry& e : FIELD_TABLE) if (taken(e)) known += (known.empty() ? "" : ", ") + std::string(e.name);
    throw Error(std::string(who) + (use == DERIVE ? ": unknown derived quantity '" : ": unknown field '") + name + "' (" + known + ")");
}

// ---- the resolver
// energy (derkeng, NS_derive.cpp:266-295), mag_vort (dermgvort on FillPatched velocities: grow_box_by_two upstream, the stencil reads one
// cell), avg_pressure (deravgpres, NS_derive.cpp:51-80), the particle counts (NavierStokesBase::ParticleDerive, NavierStokesBase.cpp:3996-4048)
void NavierStokes::derive_pointwise(const FieldEntry& e, MultiFab& out, int ocomp)
{
    auto& ctx = Context::get();
    const FabD* ot = out.d_tab;
    if (e.kind == FieldKind::ParticleCount) {
        if (e.id == 0) particles->particle_count(level, out, ocomp); else particles->total_particle_count(level, out, ocomp);
    } else if (e.id == ENERGY) {
        const FabD* st = S[inew].d_tab;
        for_each(*layout, cell_type(), 0, ctx.stream, [=] __device__(int i, int j, int k, int f) {
            const FabD s = st[f];
            const double vx = s(i, j, k, Xvel), vy = s(i, j, k, Yvel), vz = s(i, j, k, Zvel);
            ot[f](i, j, k, ocomp) = 0.5 * s(i, j, k, Density) * (vx * vx + vy * vy + vz * vz);
        });
    } else if (e.id == MAG_VORT) {
        MultiFab vel(layout, cell_type(), 3, 1);
        fillpatch(vel, S[inew], Xvel, 3, bc_vel);
        derive_mag_vort(g, out, ocomp, vel, 0);
    } else {
        const FabD* pt = P[pnew].d_tab;
        for_each(*layout, cell_type(), 0, ctx.stream, [=] __device__(int i, int j, int k, int f) {
            const FabD p = pt[f];
            ot[f](i, j, k, ocomp) = 0.125 * (p(i + 1, j, k) + p(i, j, k) + p(i + 1, j + 1, k) + p(i, j + 1, k)
                                           + p(i + 1, j, k + 1) + p(i, j, k + 1) + p(i + 1, j + 1, k + 1) + p(i, j + 1, k + 1));
        });
    }
}

// ref[q] = where the single-component field names[q] is: a state name refers to the new-time state in place; ALL velocity-gradient names
// share one fillpatch of the velocity and one derive_velgrad launch into consecutive components; a pointwise name takes one launch.
// What is formed goes to `direct` (field q at component dcomp + q: derive_fields' output) where the caller has one and the
// velocity-gradient names stand together, else to `scratch`, defined here with exactly the components that takes.
std::vector<FieldRef> NavierStokes::resolve_fields(int n, const std::string* names, unsigned use, const char* who, MultiFab& scratch, MultiFab* direct, int dcomp)
{
    std::vector<const FieldEntry*> e(n);
    std::vector<int> vq, vid;          // the velocity-gradient names: their places in the list and their ids
    int npw = 0;
    for (int q = 0; q < n; ++q) {
        e[q] = &find_field(names[q], use, who);
        if (e[q]->kind == FieldKind::Velgrad) { vq.push_back(q); vid.push_back(e[q]->id); }
        else if (e[q]->kind != FieldKind::State) ++npw;
    }
    const int nv = (int)vq.size();
    const bool vel_direct = direct && nv > 0 && vq.back() - vq.front() == nv - 1;
    int next = vel_direct ? 0 : nv;          // in the scratch array the pointwise fields follow the velocity-gradient ones
    if (next + (direct ? 0 : npw) > 0) scratch.define(layout, cell_type(), next + (direct ? 0 : npw), 0);
    std::vector<FieldRef> ref(n);
    for (int q = 0; q < n; ++q) {
        if (e[q]->kind == FieldKind::State) ref[q] = FieldRef{&S[inew], state_comp(*e[q])};
        else if (e[q]->kind != FieldKind::Velgrad) {
            MultiFab& t = direct ? *direct : scratch;
            ref[q] = FieldRef{&t, direct ? dcomp + q : next++};
            derive_pointwise(*e[q], t, ref[q].comp);
        }
    }
    if (nv > 0) {
        MultiFab vel(layout, cell_type(), 3, 1);
        fillpatch(vel, S[inew], Xvel, 3, bc_vel);
        MultiFab& t = vel_direct ? *direct : scratch;
        const int c0 = vel_direct ? dcomp + vq.front() : 0;
        derive_velgrad(g, t, c0, nv, vid.data(), vel, 0, p.visc_coef, 0);
        for (int s = 0; s < nv; ++s) ref[vq[s]] = FieldRef{&t, c0 + s};
    }
    return ref;
}

// out(ocomp + q) = field names[q]: the resolver forms in place what it can; the rest (state names, scattered velocity-gradient names) is copied
void NavierStokes::form_fields(int n, const std::string* names, unsigned use, const char* who, MultiFab& out, int ocomp)
{
    IAMRX_ASSERT(out.type.cell() && out.layout->id == layout->id);
    if (ocomp < 0 || ocomp + n > out.ncomp) throw Error(std::string(who) + ": " + std::to_string(n) + " fields from component " + std::to_string(ocomp) + " do not fit the array's " + std::to_string(out.ncomp));
    MultiFab scratch;
    const std::vector<FieldRef> ref = resolve_fields(n, names, use, who, scratch, &out, ocomp);
    for (int q = 0; q < n; ++q)
        if (ref[q].mf != &out) MultiFab::Copy(out, *ref[q].mf, ref[q].comp, ocomp + q, 1, 0);
}

void NavierStokes::derive(const std::string& name, MultiFab& out, int ocomp)
{
    if (find_field(name, DERIVE, "NavierStokes::derive").kind != FieldKind::VelAvg) { form_fields(1, &name, DERIVE, "NavierStokes::derive", out, ocomp); return; }
    IAMRX_ASSERT(out.type.cell() && out.layout->id == layout->id && ocomp + 6 <= out.ncomp);
    stats_derive_vel_avg(out, ocomp, Savg, time_avg, time_avg_fluct);          // der_vel_avg, NS_derive.cpp:11-45: 6 components
}

void NavierStokes::derive_fields(int n, const std::string* names, MultiFab& out, int ocomp)
{
    if (n < 1 || !names) throw Error("NavierStokes::derive_fields: no field names");
    for (int q = 0; q < n; ++q) if (names[q] == "velocity_average") throw Error("NavierStokes::derive_fields: velocity_average has six components; ask derive() for it");
    form_fields(n, names, FIELDS, "NavierStokes::derive_fields", out, ocomp);
}

// this rank's sums of cell values -> volume-weighted sums over the ranks
void NavierStokes::finish_sums(int n, double* out) const
{
    const double vol = g.dx[0] * g.dx[1] * g.dx[2];
    for (int q = 0; q < n; ++q) out[q] *= vol;
    auto& comm = Context::get().comm;
    if (comm && comm->nranks > 1 && !layout->replicated) comm->allreduce(out, n, ReduceOp::Sum);
}

// this level's part of integrate, histogram and histogram2: the cells where cov (this level's layout; null: none) is zero
void NavierStokes::integrate_level(int n, const std::string* names, const MultiFab* cov, double* out)
{
    MultiFab scratch;
    const std::vector<FieldRef> ref = resolve_fields(n, names, REDUCE, "integrate", scratch);
    std::vector<int> comps(n), at(n);          // one pass (and one read-back) per array, wherever its names stand in the list
    std::vector<double> r(n);
    for (const MultiFab* mf : {(const MultiFab*)&S[inew], (const MultiFab*)&scratch}) {
        int m = 0;
        for (int q = 0; q < n; ++q) if (ref[q].mf == mf) { comps[m] = ref[q].comp; at[m++] = q; }
        if (m > 0) reduce_sum_comps(*mf, m, comps.data(), cov, r.data());
        for (int s = 0; s < m; ++s) out[at[s]] = r[s];
    }
    finish_sums(n, out);
}

void NavierStokes::hist_add_names(int n, const std::string* names, const MultiFab* cov, const double* lo, const double* hi, int nbins,
                                  unsigned long long weight, unsigned long long* d_counts)
{
    MultiFab scratch;
    const std::vector<FieldRef> ref = resolve_fields(n, names, REDUCE, "histogram", scratch);
    std::vector<int> comps(n);
    for (int q = 0; q < n; ++q) comps[q] = ref[q].comp;
    for (int q = 0, m; q < n; q += m) {          // one pass per run of consecutive names in the same array (the slots of a pass are consecutive)
        for (m = 1; q + m < n && ref[q + m].mf == ref[q].mf; ++m) {}
        hist_add(*ref[q].mf, m, comps.data() + q, cov, lo + q, hi + q, nbins, weight, d_counts + (size_t)q * (nbins + 3));
    }
}

void NavierStokes::hist_add2_names(const std::string& namex, const std::string& namey, const MultiFab* cov, const double lo[2], const double hi[2],
                                   const int nbins[2], unsigned long long weight, unsigned long long* d_counts)
{
    MultiFab scratch;
    const std::string names[2] = {namex, namey};
    const std::vector<FieldRef> ref = resolve_fields(2, names, REDUCE, "histogram2", scratch);
    hist_add2(*ref[0].mf, ref[0].comp, *ref[1].mf, ref[1].comp, cov, lo, hi, nbins, weight, d_counts);
}

// ---- the loop over levels
// the levels of a diagnostic, coarsest first, each with the mask of the cells the next finer one covers (null for the finest); the weights
// of a composite histogram: level l counts 8^(finest - l) per cell, so that the slots are in units of finest-level cell volumes and
// together sum to cells(level 0) * 8^finest, which must stay below 2^53 (the transport between the ranks carries doubles)
struct NavierStokes::Levels {
    const std::vector<NavierStokes*>& lev;
    std::vector<MultiFab> cov;
    explicit Levels(const std::vector<NavierStokes*>& l) : lev(l), cov(l.size() - 1)
    {
        for (size_t k = 0; k + 1 < lev.size(); ++k) cov[k] = fine_coverage(lev[k]->layout, lev[k + 1]->layout, lev[k]->g, lev[k + 1]->ratio);
    }
    int fin() const { return (int)lev.size() - 1; }
    const MultiFab* mask(int l) const { return l < fin() ? &cov[l] : nullptr; }
    unsigned long long weight(int l) const { return 1ULL << (3 * (fin() - l)); }
    void check_weights(const char* who) const
    {
        if (3 * fin() >= 53) throw Error(std::string(who) + ": too many levels for counts below 2^53");
        const double total = (double)lev[0]->g.domain.npts() * (double)weight(0);
        if (!(total < 9007199254740992.0)) throw Error(std::string(who) + ": cells(level 0) * 8^finest = " + std::to_string(total) + " does not stay below 2^53");
    }
    // out[q] = sum over the levels, level 0 first, of what part(level, mask, v) leaves in v[0 .. n)
    template <class F>
    void sum(int n, double* out, F&& part) const
    {
        double few[16];
        std::vector<double> many(n > 16 ? n : 0);
        double* v = n > 16 ? many.data() : few;
        for (int q = 0; q < n; ++q) out[q] = 0.0;
        for (int l = 0; l <= fin(); ++l) {
            part(*lev[l], mask(l), v);
            for (int q = 0; q < n; ++q) out[q] += v[q];
        }
    }
};

// NavierStokes::sum_integrated_quantities (NavierStokes.cpp:1046-1079; amrex volumeWeightedSum: the cells under the finer level do not
// count, the weight is the cell volume): per level one fused reduction (k_basic.hip), then one sum over the ranks
void NavierStokes::sum_integrated_of(const LevelList& lev, double out[3])
{
    Levels(lev).sum(3, out, [](NavierStokes& s, const MultiFab* cov, double* v) { reduce_sum_integrated(s.S[s.inew], Density, Tracer, cov, v); s.finish_sums(3, v); });
}

void NavierStokes::integrate_of(const LevelList& lev, int n, const std::string* names, double* out)
{
    if (n < 1 || !names || !out) throw Error("integrate: no field names");
    for (int q = 0; q < n; ++q) lev[0]->find_field(names[q], REDUCE, "integrate");          // (an unknown name: before anything is built)
    Levels(lev).sum(n, out, [&](NavierStokes& s, const MultiFab* cov, double* v) { s.integrate_level(n, names, cov, v); });
}

int NavierStokes::plane_profile_of(const LevelList& lev, int dir, int bin_level, double* out, int cap)
{
    const int fin = (int)lev.size() - 1;
    if (dir < 0 || dir > 2) throw Error("plane_profile: dir must be 0, 1 or 2, not " + std::to_string(dir));
    if (bin_level < 0 || bin_level > fin) throw Error("plane_profile: bin_level " + std::to_string(bin_level) + " outside 0 .. " + std::to_string(fin));
    const int nbins = profile_nbins(lev[0]->g, dir, bin_level);
    if (cap < nbins) throw Error("plane_profile: the profile has " + std::to_string(nbins) + " bins, the caller's array holds " + std::to_string(cap));
    const Levels L(lev);
    std::vector<ProfileLevel> pl;
    for (int l = 0; l <= fin; ++l) pl.push_back(ProfileLevel{&lev[l]->S[lev[l]->inew], L.mask(l), &lev[l]->g});
    profile_reduce((int)pl.size(), pl.data(), dir, bin_level, Density, Tracer, out);
    return nbins;
}

void NavierStokes::histogram_of(const LevelList& lev, int n, const std::string* names, const double* lo, const double* hi, int nbins, long long* counts)
{
    if (n < 1) throw Error("histogram: no field names");
    for (int q = 0; q < n; ++q) { lev[0]->find_field(names[q], REDUCE, "histogram"); hist_check_range("histogram", lo[q], hi[q], nbins, HIST_NBINS_MAX); }
    const Levels L(lev);
    L.check_weights("histogram");
    HistSlots slots((size_t)n * (nbins + 3));
    for (int l = 0; l <= L.fin(); ++l) lev[l]->hist_add_names(n, names, L.mask(l), lo, hi, nbins, L.weight(l), slots.d);
    slots.finish(counts);
}

void NavierStokes::histogram2_of(const LevelList& lev, const std::string& namex, const std::string& namey, const double lo[2], const double hi[2],
                                 const int nbins[2], long long* counts)
{
    lev[0]->find_field(namex, REDUCE, "histogram2"); lev[0]->find_field(namey, REDUCE, "histogram2");
    hist2_check("histogram2", lo, hi, nbins);
    const Levels L(lev);
    L.check_weights("histogram2");
    HistSlots slots((size_t)nbins[0] * nbins[1] + 1);
    for (int l = 0; l <= L.fin(); ++l) lev[l]->hist_add2_names(namex, namey, L.mask(l), lo, hi, nbins, L.weight(l), slots.d);
    slots.finish(counts);
}

void hist2_check(const char* who, const double lo[2], const double hi[2], const int nbins[2])
{
    for (int a = 0; a < 2; ++a) hist_check_range(who, lo[a], hi[a], nbins[a], HIST2_SLOTS_MAX);
    if ((long)nbins[0] * nbins[1] > HIST2_SLOTS_MAX)
        throw Error(std::string(who) + ": nbins = " + std::to_string(nbins[0]) + " x " + std::to_string(nbins[1]) + " exceeds " + std::to_string(HIST2_SLOTS_MAX) + " slots");
}

}  // namespace iamrx
