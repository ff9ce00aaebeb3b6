// iamr_amd/csrc/particles.h -- passive tracer particles on a level or a hierarchy (k_particles.hip): the role of AMReX's
// AmrTracerParticleContainer as IAMR uses it (reference Source/NavierStokesBase.cpp:198-222, 3751-4057, NavierStokes.cpp:672-677).
// The arithmetic of the container belongs to AMReX, which is not part of the reference tree: this row is UNPINNED (DESIGN.md section 2
// and section 7 row f8); tests/particles_numpy.py restates what is implemented here.
//
// Storage: structure of arrays on the device -- x, y, z, three reals r0..r2 (the velocity the particle was last moved with; the saved
// position between the two passes of advect), id, cpu, level and local box index -- kept grouped by (level, box), so that ONE launch per
// level serves all its boxes through the level's FabD table.  Grouping is a count / prefix / scatter with integer vector atomics; the
// order inside a box is not part of the contract.
//
// Several ranks (Context::comm->nranks > 1): every rank holds the particles of the boxes it owns.  A particle is placed against the
// level's GLOBAL box list (Layout::boxes), so every rank finds the same (level, box) for it; redistribute() then sends the particles
// whose box another rank owns to that rank (one allreduce of the send counts, one pack kernel, one Comm::exchange, one filing kernel)
// and scatters stayers and arrivals together.  Collective on several ranks: define, add, redistribute, total_particle_count,
// global_count -- every rank calls them, also one without particles or boxes; an error one rank finds is thrown on all of them.  Local:
// read, set_positions, size, count_at_level, advect, particle_count.  One rank: no collective is issued and the launches are the ones
// of the single-process container.
#pragma once
#include "mf.h"
#include <vector>
#include <memory>
#include <string>

namespace iamrx {

struct PLevelD {
    const int* tab;          // box lookup: index in the level's global box list (or -1) of every block of gran^3 cells of the level's domain
    const BoxD* boxes;       // the level's local valid boxes (Layout::d_boxes)
    const BoxD* gboxes;      // all boxes of the level (Layout::boxes); one rank: the same array as `boxes`
    const int* owner;        // [ngbox] owner rank of a global box; one rank: null (every box is local and global index == local index)
    const int* lidx;         // [ngbox] local index of a global box on its owner
    int ngbox;
    int tn[3];               // blocks per direction
    int gran;                // cells per block and direction: divides every box corner and length of the level
    int dlo[3], n[3];        // domain low corner and extent (cells)
    double dx[3];
    int key0, nbox;          // first group key of the level, its number of boxes
};
struct PHierD {
    static constexpr int MAXLEV = 8;
    PLevelD L[MAXLEV];
    int nlev;
    double plo[3], phi[3];
    int per[3];
};
struct PArrays {
    double* x[3] = {nullptr, nullptr, nullptr};
    double* r[3] = {nullptr, nullptr, nullptr};
    int *id = nullptr, *cpu = nullptr, *lev = nullptr, *box = nullptr;
};

class Particles {
public:
    // geoms[l] / layouts[l]: the levels, coarsest first, refined by `ratio` from one to the next; layouts[0] covers the domain
    Particles(const std::vector<Geometry>& geoms, const std::vector<LayoutP>& layouts, int ratio);
    ~Particles();
    Particles(const Particles&) = delete;
    Particles& operator=(const Particles&) = delete;
    // new levels under the particles the container holds (a level or a hierarchy takes the container over; a regrid): every particle keeps
    // its position; those of the leading levels whose Layout objects stay keep their place, the others wait on the last such level (or
    // level 0) until the caller's redistribute, from that level or below, places them
    void define(const std::vector<Geometry>& geoms, const std::vector<LayoutP>& layouts, int ratio);
    int nlevels() const { return (int)m_layouts.size(); }
    const LayoutP& layout(int l) const { return m_layouts[l]; }
    const Geometry& geom(int l) const { return m_geoms[l]; }
    long size() const { return m_np; }
    long count_at_level(int l) const { return m_lev_n.at(l); }
    // n particles from host arrays: xyz (n x 3); r (n x 3), ids, cpus may be null (zeros, ids from the container's counter, 0).  They are
    // placed by redistribute(0, finest, 0); returns what that returns.  Several ranks: collective -- every rank passes its own list, possibly
    // none (n = 0, null arrays), and the particles go to the owners of their boxes.  Without ids the new ids continue the counter in rank
    // order (rank q's after rank q - 1's), so all positions on rank 0 give the ids of a one-rank run; with ids the counter becomes the
    // largest id + 1 over the ranks
    long add(long n, const double* xyz, const double* r, const int* ids, const int* cpus);
    // every particle to host arrays of size() entries (any may be null): xyz, r (n x 3), id, cpu, level, box
    void read(double* xyz, double* r, int* id, int* cpu, int* lev, int* box) const;
    // overwrite the positions, in storage order (a caller that moves the particles itself); the caller redistributes
    void set_positions(const double* xyz);
    // TracerParticleContainer::AdvectWithUmac for the particles of level `lev`: umac[d] face-centred in d on the level's layout, with the
    // ghost faces the particles' stencils reach already filled (one layer on level 0; see particles_grow_umac)
    void advect(int lev, const MultiFab* const umac[3], double dt);
    // returns the number of particles removed beyond non-periodic domain faces (summed over the ranks); throws -- on every rank -- when a
    // particle of any rank cannot be placed, and the container then holds what it held
    long redistribute(int lev_min, int lev_max, int ngrow);
    void particle_count(int lev, MultiFab& out, int ocomp);
    // several ranks: collective; the finer levels' counts reach coarse boxes of other owners (level by level: counted on the finer level,
    // summed onto its coarsened boxes, copied across; a fine cell counts where every level in between has a box under it)
    void total_particle_count(int lev, MultiFab& out, int ocomp);
    // collective: the counts summed over the ranks (per_level: nlevels() entries, may be null)
    void global_count(long* per_level, long* total) const;
    // ---- state sampled at the particles, and the timestamp files (NavierStokesBase::post_timestep_particle, NavierStokesBase.cpp:3881-3951,
    // and AMReX's cell-centred cic_interpolate / Timestamp: not in the reference tree, UNPINNED like the rest; tests/timestamp_numpy.py
    // restates what is implemented).  All three are LOCAL to the rank.
    static constexpr int MAX_SAMPLE = 16;
    // the components comps[0 .. M) (any order, 1 <= M <= 16) of the cell-centred mf on the level's boxes, trilinearly interpolated between
    // cell centres to the particles of level lev, in storage order: host_vals[p * M + m], id[p], cpu[p] for p < count_at_level(lev) (any
    // may be null; a particle with id <= 0 gets zeros).  The stencil is clamped to the array only: mf arrives with its ghost cells filled
    // (FillPatch), and they hold what the boundary conditions say.  host_vals, id and cpu all null: the kernel is launched and nothing is
    // read back or waited for (tools/bench_particles.py times that)
    void sample(int lev, const MultiFab& mf, const int* comps, int M, double* host_vals, int* id, int* cpu);
    // basename empty: off (the default).  indices: the state components the step samples (AmrNS::post_timestep, NavierStokes::step); the
    // container itself only needs their number
    void set_timestamp(const std::string& basename, std::vector<int> indices);
    bool timestamps_on() const { return !m_ts_base.empty(); }
    const std::vector<int>& timestamp_indices() const { return m_ts_indices; }
    // appends one line per particle of level lev with id > 0, sorted by (id, cpu), to basename + "_" + two digits of rank % 64 (opened in
    // append mode per call, as upstream: a restart continues the file; no particle: no file is touched):
    //   id cpu x y z time r0 r1 r2 v_0 .. v_{M-1}      reals %.10e (scientific, precision 10), single blanks
    // v_m: component m of mf (the first indices.size() components) at the particle; mf null: no values.  With fixed_dir = d the
    // coordinate d and r_d are left out
    void timestamp(int lev, const MultiFab* mf, double time);
    int next_id = 1;              // equal on all ranks
    long n_removed = 0;           // removed beyond non-periodic faces since creation, summed over the ranks
    int fixed_dir = -1;           // a coordinate advect leaves alone (the slab direction of a lifted two-dimensional run), -1: none
    int ratio() const { return m_ratio; }

private:
    std::vector<Geometry> m_geoms;
    std::vector<LayoutP> m_layouts;
    int m_ratio = 2;
    PHierD m_h;
    std::vector<int*> m_tabs;
    PArrays m_a;
    void* m_block = nullptr;
    long m_np = 0, m_cap = 0;
    int m_nkeys = 0;
    std::vector<long> m_lev_n, m_lev_start;
    std::string m_ts_base;
    std::vector<int> m_ts_indices;
    static void carve(PArrays& a, void* block, long cap);
    void reserve(long cap);
    void free_tables();
    long redistribute_ranks(int lev_min, int lev_max, int ngrow);
    void add_local(long n, const double* xyz, const double* r, const int* ids, const int* cpus);
    void add_finer_counts_ranks(int lev, MultiFab& out, int ocomp);
};
using ParticlesP = std::shared_ptr<Particles>;

// The face velocities of a refined level on ng ghost layers, for the particles that stay on the level up to ncycle - 1 cells outside its
// boxes between the sub-steps of a coarse step (umac_n_grow = ncycle, NavierStokesBase.cpp:625-628).  ug[d]: scratch arrays (defined here,
// ng ghost layers).  Valid faces and the first ghost layer (with IAMR's divergence fix) are the level's u_mac; further out, fine and
// periodic neighbours where they exist and the FaceLinear interpolation of the coarse faces (create_umac_grown) elsewhere.
void particles_grow_umac(MultiFab ug[3], const MultiFab* const umac_fine[3], const MultiFab* const umac_crse[3], const Geometry& cgeom,
                         const Geometry& fgeom, int ratio, int ng);

}  // namespace iamrx
