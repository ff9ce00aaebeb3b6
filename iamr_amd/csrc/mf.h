// iamr_amd/csrc/mf.h -- device-resident patch containers (the MultiFab/BoxArray/DistributionMapping
// role of SURVEY 2.2 a19), ghost-exchange plans and the communicator abstraction.
//
// MI355X-first choices: every local FAB of a level lives in ONE HBM allocation; kernels are launched
// once per level over a device-resident descriptor table (not once per FAB); ghost exchange is a
// precomputed copy plan executed by a single batched kernel (local) plus packed peer messages (remote).
#pragma once
#include <functional>
#include "core.h"
#include <vector>
#include <memory>
#include <map>
#include <array>

namespace iamrx {

// ------------------------------------------------------------------ communicator
enum class ReduceOp { Sum, Max, Min };

struct Message {
    int peer;
    double* dev_ptr;   // device buffer (packed)
    size_t count;      // doubles
};

// One process per GPU.  Serial by default; RCCL backend in comm_rccl.cpp; callback backend for tests.
struct Comm {
    int rank = 0, nranks = 1;
    virtual ~Comm() = default;
    virtual void allreduce(double* host_vals, int n, ReduceOp op) { (void)host_vals; (void)n; (void)op; }
    // in place on a DEVICE buffer, ordered on stream s, no host synchronisation: the reductions of the solvers (norms, dot products)
    // finish on the device, are combined across ranks where they are, and are read back once (k_basic.hip finish_to_host)
    virtual void allreduce_device(double* dev_vals, int n, ReduceOp op, hipStream_t s) { (void)dev_vals; (void)n; (void)op; (void)s; }
    // exchange packed device buffers with peers (all sends/recvs posted together)
    virtual void exchange(const std::vector<Message>& sends, const std::vector<Message>& recvs, hipStream_t s)
    {
        (void)s;
        if (!sends.empty() || !recvs.empty()) throw Error("serial Comm cannot exchange with peers");
    }
};

// ------------------------------------------------------------------ context
struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::unique_ptr<Comm> comm;
    // caching device allocator (hipMalloc/hipFree synchronise; never call them inside a time step)
    std::multimap<size_t, void*> free_blocks;
    std::map<void*, size_t> live_blocks;
    size_t bytes_live = 0, bytes_cached = 0;
    // round 6: the blocks are carved out of large chunks and a freed block merges with its free neighbours (IAMRX_ARENA, mf.hip): free_addr
    // holds the same free blocks by address, chunk_end the end of every chunk by its start (blocks never merge across chunks)
    std::map<char*, size_t> free_addr;
    std::map<char*, char*> chunk_end;
    bool arena = true;
    size_t bytes_chunks = 0;
    size_t n_device_malloc = 0;    // hipMalloc calls (cache misses): must stay flat inside the time loop
    size_t n_stream_sync = 0;      // host waits on the stream (Context::sync): reductions read back, plan uploads
    double* d_scratch = nullptr;   // reduction scratch
    double* h_scratch = nullptr;   // pinned
    size_t scratch_n = 0;

    static Context& get();
    void init(int dev);
    void* alloc(size_t bytes);
    void free(void* p);
    void release_cache();
    void sync();
    void ensure_scratch(size_t n);
    void upload_async(void* dst, const void* src, size_t bytes);
    char* h_ring = nullptr;
    size_t ring_off = 0;
    // Second stream: halo exchanges that run beside interior work.  fork_side(): everything issued on `side` from
    // here on sees what `stream` has been given so far; join_side(): `stream` continues after what `side` has been given.  Device blocks
    // that side-stream work returns to the caching allocator are parked until the join (the cache is ordered by `stream` only).
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // peer exchanges issued (execute_plan calls with messages) and doubles sent, by stream: [0] main (in front of the work that needs
    // them: exposed), [1] side (beside interior work: hidden as far as that work lasts) -- tools/count_comm.py
    size_t n_exchange[2] = {0, 0}, exchange_doubles[2] = {0, 0};
    std::vector<void*> parked;
    void fork_side();
    void join_side();
    void free_on(hipStream_t s, void* p) { if (s == stream) free(p); else parked.push_back(p); }
    // n doubles at device address d, brought to the pinned scratch behind everything `stream` has been given: valid until the next use of h_scratch
    const double* read_back(const double* d, size_t n);
};

// ------------------------------------------------------------------ scoped owners of a call's device scratch
// One Context::alloc block of n elements T, freed when the owner dies.  A freed block may be handed out again at once: that is safe only
// because ALL work that touches such a block is ordered on ctx.stream (the next user's work runs behind the last reader's).  Context::free
// is host bookkeeping and makes no HIP call, so freeing while an error unwinds is safe whatever failed, and the destructor adds no
// synchronisation.  Never for a block that work on another stream touches (Context::free_on).
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    explicit DevBuf(size_t n) : p((T*)Context::get().alloc(n * sizeof(T))) {}
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    ~DevBuf() { Context::get().free(p); }
    T* get() const { return p; }
    operator T*() const { return p; }
};

// The n events around the n - 1 passes of a measurement aid: mark() records the next one on ctx.stream, finish() waits for the last and
// writes the n - 1 times between neighbours (milliseconds), after which the next repeat marks from the first again.  A body that runs
// timed and untimed takes a PassTimer* and marks through mark(t): null, so do not time.
struct PassTimer {
    std::vector<hipEvent_t> ev;
    size_t next = 0;
    explicit PassTimer(int n)
    {
        ev.reserve(n);
        for (int q = 0; q < n; ++q) { hipEvent_t e; IAMRX_HIP_CHECK(hipEventCreate(&e)); ev.push_back(e); }
    }
    PassTimer(const PassTimer&) = delete;
    ~PassTimer() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void mark() { IAMRX_ASSERT(next < ev.size()); IAMRX_HIP_CHECK(hipEventRecord(ev[next++], Context::get().stream)); }
    static void mark(PassTimer* t) { if (t) t->mark(); }
    void finish(float* ms)
    {
        IAMRX_ASSERT(next == ev.size());
        IAMRX_HIP_CHECK(hipEventSynchronize(ev.back()));
        for (size_t q = 0; q + 1 < ev.size(); ++q) IAMRX_HIP_CHECK(hipEventElapsedTime(&ms[q], ev[q], ev[q + 1]));
        next = 0;
    }
};

// ------------------------------------------------------------------ tuning registry
// Every run-time switch of the library is a key of ONE registry: filled once, at iamrx_init, from the environment
// variables IAMRX_<KEY> that are set, changed afterwards only through iamrx_tuning_set, and read by the code at the point of use
// (tune(key, default)) -- no function-local static caches a choice for the life of the process.
double tune(const char* key, double dflt);             // key: a string LITERAL (looked up by address, mf.hip)
double tune_by_name(const char* key, double dflt);     // any string
void trace_blas_site(const char* what, long points);   // IAMRX_BLAS_TRACE (mf.hip)
void tuning_set(const char* key, double value);
void tuning_count(const char* key);     // registry entry key += 1: a counter of the library's, read with iamrx_tuning_get
void tuning_load_environment();          // called by Context::init

// ------------------------------------------------------------------ scoped profiler (measurement aid)
// ProfScope p("name") accumulates the wall time of the scope (stream drained at both ends) under its name while profiling is enabled
// (iamrx_scope_profile); nested scopes are reported with their path "outer/inner".  Off: two predictable branches, no synchronisation.
struct ProfScope {
    static bool enabled;
    bool on;
    std::string key;
    double t0 = 0.0;
    explicit ProfScope(const char* name);
    ~ProfScope();
};
#define PROF_NEXT(var, name) do { (var).reset(); (var) = std::make_unique<::iamrx::ProfScope>(name); } while (0)
void scope_profile_enable(bool on, bool reset);
std::string scope_profile_report();

// ------------------------------------------------------------------ layout
// All boxes of one level (cell-centred, non-overlapping) + owner rank of each.
// Caches keyed by a layout id (copy plans, descriptor lists, masks, derived layouts) register an evictor; a layout that dies -- or that a
// regrid replaces (AmrNS::install_grids calls evict_layout_caches explicitly: a cached mask keeps its layout alive) -- takes its entries
// with it, so that a regridding run does not accumulate device memory (ADVICE / VERDICT round 1).
void register_layout_evictor(std::function<void(uint64_t)> f);
void evict_layout_caches(uint64_t layout_id);

struct Layout {
    std::vector<BoxD> boxes;
    std::vector<int> owner;
    std::vector<int> local;      // global indices of the boxes owned by this rank
    std::vector<int> local_of;   // global -> local index or -1
    BoxD* d_boxes = nullptr;     // device copy of the LOCAL valid boxes
    int max_len[3] = {0, 0, 0};  // max local box extent (cells)
    bool all_lo_even[3] = {true, true, true};   // every local box starts on an even, non-negative index
    uint64_t id = 0;
    // replicated: every rank holds ALL boxes (MG levels below the agglomeration level); nothing on such a layout communicates
    bool replicated = false;
    uint64_t replicated_of = 0;   // id of the distributed layout it was made from

    Layout(const std::vector<BoxD>& b, const std::vector<int>& own, int myrank);
    ~Layout();
    int nlocal() const { return (int)local.size(); }
    const BoxD& lbox(int li) const { return boxes[local[li]]; }
    long local_cells() const;
    long total_cells() const;
    // memoised: the multigrid hierarchies of successive solves share the same coarse Layout objects, so their
    // ghost-exchange plans (keyed by layout id) are built once
    std::shared_ptr<Layout> coarsened(int ratio) const;
    mutable std::shared_ptr<Layout> m_coarse;
    mutable int m_coarse_ratio = 0;
    bool coarsenable(int ratio, int min_width) const;
    // Slab levels (2-D inputs lifted onto a y-periodic slab): every box is two cells thick in y, which cannot
    // be coarsened any further; x and z still can.  The next multigrid level is the coarsening by 2 in x and z with y KEPT at two cells
    // (slab_coarsened), dx doubled in every direction; the transfers go through the ordinary coarsening by 2 (`coarsened(2)`: one cell
    // in y, the "virtual" level) and duplicate its plane (slab_duplicate) -- valid for fields that do not vary along the slab.
    bool slab_coarsenable(int min_width) const;
    std::shared_ptr<Layout> slab_coarsened() const;
    mutable std::shared_ptr<Layout> m_slab;
    // same boxes, all of them owned by this rank (on every rank)
    std::shared_ptr<Layout> make_replicated() const;
    mutable std::shared_ptr<Layout> m_repl;
};
using LayoutP = std::shared_ptr<Layout>;
// The boxes a rank owns, merged into as few rectangular boxes as share full faces (same cells, same owners): one process drives one GPU
// with 288 GB, so nothing is gained from small boxes inside a rank, and every level-wide kernel runs fastest on few large ones (no ghost
// fills between colour passes, index wrap on periodic domains).  The level objects (NavierStokes, AmrNS) work on the merged layout and
// translate to the caller's boxes at their data accessors.  Returns l itself if nothing merges or IAMRX_COALESCE = 0.
LayoutP coalesce_layout(const LayoutP& l);
size_t coalesce_merge_count();     // calls of coalesce_layout that merged boxes so far (the test suite's two-mode runner asks, tests/conftest.py)

struct IndexType {
    int t[3];
    bool operator<(const IndexType& o) const { return std::lexicographical_compare(t, t + 3, o.t, o.t + 3); }
    bool cell() const { return !t[0] && !t[1] && !t[2]; }
};
inline IndexType cell_type() { return {{0, 0, 0}}; }
inline IndexType node_type() { return {{1, 1, 1}}; }
inline IndexType face_type(int d) { IndexType t{{0, 0, 0}}; t.t[d] = 1; return t; }

// ------------------------------------------------------------------ copy plans
struct CopyDesc {
    int src_fab, dst_fab;   // local fab indices (or buffer offsets for remote segments)
    BoxD region;            // destination index region
    int shift[3];           // src index = dst index + shift
    long buf_off;           // offset (in doubles, per component block) in a packed message buffer
    int kstep = 1;          // 2: only every second z-plane of the region, starting at region.lo[2] (parity-filtered fills)
    __host__ __device__ int nk() const { return (region.hi[2] - region.lo[2]) / kstep + 1; }
    __host__ __device__ long npts() const { return (long)region.len(0) * region.len(1) * nk(); }
};

// Flat work list of a descriptor list (built on first use, execute_plan): entry (descriptor, chunk of COPY_CHUNK points).  The plain launch
// gives EVERY descriptor as many workgroups as the largest one needs; a ghost exchange of a regridded level has tens of thousands of
// descriptors of very different sizes (40 k for the nodal data of 431 boxes), so most of those workgroups found nothing to do (round 6).
constexpr int COPY_CHUNK = 1024;
struct CopyWork { int2* d = nullptr; int n = 0; bool built = false; };
struct CopyPlan {
    std::vector<CopyDesc> local;           // host copy
    CopyDesc* d_local = nullptr;
    long max_local_pts = 0;
    mutable CopyWork w_local;
    // remote: per peer, pack list (src_fab regions -> send buffer) and unpack list (recv buffer -> dst_fab)
    struct Peer {
        int rank;
        std::vector<CopyDesc> pack, unpack;
        CopyDesc *d_pack = nullptr, *d_unpack = nullptr;
        long send_pts = 0, recv_pts = 0, max_pack_pts = 0, max_unpack_pts = 0;
        mutable CopyWork w_pack, w_unpack;
    };
    std::vector<Peer> peers;
    ~CopyPlan();
};

// ------------------------------------------------------------------ MultiFab
class MultiFab {
public:
    LayoutP layout;
    IndexType type;
    int ncomp = 0, ngrow = 0;
    double* base = nullptr;          // single allocation for all local fabs
    size_t total_doubles = 0;
    std::vector<FabD> h_tab;         // one entry per local fab
    FabD* d_tab = nullptr;

    MultiFab() = default;
    MultiFab(LayoutP l, IndexType t, int nc, int ng);
    ~MultiFab();
    MultiFab(const MultiFab&) = delete;
    MultiFab& operator=(const MultiFab&) = delete;
    MultiFab(MultiFab&& o) noexcept;
    MultiFab& operator=(MultiFab&& o) noexcept;

    void define(LayoutP l, IndexType t, int nc, int ng);
    // zero-copy view of caller-owned device FABs (one pointer per LOCAL box, each fab contiguous in the Array4 layout incl. ghost
    // cells): the library never frees or moves them (amrex::MultiFab alias over The_Arena memory)
    void alias(LayoutP l, IndexType t, int nc, int ng, double* const* fab_ptrs);
    bool is_alias = false;
    // components [comp, comp + nc) of src as a MultiFab of their own (same boxes, same ghost width, the same memory): lets an operator
    // that works on whole MultiFabs solve in place on part of a state array
    void view_of(const MultiFab& src, int comp, int nc);
    void clear();
    bool defined() const { return base != nullptr || (layout && layout->nlocal() == 0); }
    int nlocal() const { return layout->nlocal(); }
    BoxD validbox(int li) const { return convert(layout->lbox(li), type.t); }
    BoxD fabbox(int li) const { return grow(validbox(li), ngrow); }

    void setVal(double v);                              // all comps, incl. ghosts
    // the OWNER's promise that every entry is v and stays v (constant viscosity / diffusivity arrays of a level): consumers that would
    // otherwise scan the array for uniformity (CellMG::prepare: a pass + a host synchronisation per array and solve) take the mark
    // The mark describes the data: define / alias / view_of / clear drop it, a move takes it along, setVal with another value, a Copy
    // from an array without the same mark and copy_from_host end it; kernels that write through d_tab are the owner's business.
    // IAMRX_CHECK_UNIFORM = 1 makes CellMG::prepare verify the promise.
    void mark_uniform(double v) { uniform_marked = true; uniform_value = v; }
    bool uniform_marked = false;
    double uniform_value = 0.0;
    // the opposite statement of the owner: the array varies in space (the LES face viscosities) -- consumers take their array-coefficient
    // paths without scanning it for uniformity.  Never wrong for the result (the array holds the data either way); dropped like the mark above.
    void mark_varying() { varying_marked = true; uniform_marked = false; }
    bool varying_marked = false;
    // max norms of nc components in ONE reduction / host synchronisation: out[n] = max |comp + n|
    void norm0_comps(int comp, int nc, int ng, double* out, bool local = false) const;
    void setVal(double v, int comp, int nc, int ng);
    void FillBoundary(const Geometry& g);               // same-level + periodic ghost exchange (all comps)
    // ngv: ghost depth per direction (<= ngrow); on: the stream the exchange is issued on (null: the context's; Context::side between fork_side / join_side)
    void FillBoundary(const Geometry& g, int comp, int nc, const int* ngv = nullptr, int kpar = -1, hipStream_t on = nullptr);
    // FillBoundary of cell-centred data whose boxes ALSO hand on the first `ext` ghost layers they hold beyond the non-periodic sides of the
    // domain (a boundary fill their owner made): afterwards the edge / corner ghost cells beyond a wall next to a box-box face equal the
    // face ghost cells of the box next door (CellMG's two-layer density copy)
    void FillBoundaryWallExt(const Geometry& g, int ext);
    // valid + ng ghost cells
    static void Copy(MultiFab& dst, const MultiFab& src, int scomp, int dcomp, int nc, int ng);
    // dst = a*x + b*y style helpers live in blas (kernels.h)
    double norm0(int comp, int nc, int ng, bool local = false) const;     // max |.| over valid (+ng) region
    double sum_unique(const Geometry& g, int comp, bool local = false) const;   // sum over owner copies (nodal aware)

    void copy_to_host(int li, double* dst) const;      // whole fab (all comps, with ghosts)
    void copy_from_host(int li, const double* src);

private:
    void release();
};

// Uniform bin index over a list of boxes (host): the boxes that meet a region without a scan of the whole list (round 6: the copy-plan
// builders visited every (box, box, periodic shift) triple -- quadratic in the number of boxes of a regridded level).
struct BoxBins {
    std::vector<BoxD> b;
    BoxD bbox;
    int bsz[3] = {4, 4, 4}, nbin[3] = {1, 1, 1};
    std::vector<std::vector<int>> bins;
    mutable std::vector<int> stamp;
    mutable int stamp_id = 0;
    explicit BoxBins(std::vector<BoxD> boxes);
    // indices (ascending) of the boxes that intersect q
    void query(const BoxD& q, std::vector<int>& out) const;
};

// host-only plan construction (no device access; unit-testable on CPU)
void build_fill_plan_host(const std::vector<BoxD>& boxes, const std::vector<int>& owner, const std::vector<int>& local_of, int me,
                          IndexType t, int ng, const Geometry& g, CopyPlan& plan, std::map<int, CopyPlan::Peer>& peers, const int* ngv = nullptr,
                          int kpar = -1, int wall_ext = 0);

// plan cache: FillBoundary plans keyed by (layout id, type, ngrow, periodicity, domain)
// kpar = 0 / 1: only the z-planes of that parity (global index) are exchanged
const CopyPlan& fill_boundary_plan(const Layout& l, IndexType t, int ng, const Geometry& g, const int* ngv = nullptr, int kpar = -1, int wall_ext = 0);
// add: dst += src instead of dst = src (the regions of one plan must then not overlap in dst)
void execute_plan(const CopyPlan& plan, MultiFab& dst, const MultiFab& src, int scomp, int dcomp, int nc, bool add = false, hipStream_t on = nullptr);
// multigrid agglomeration: all-gather of the valid regions into a replicated copy of the level / pick-out of the own boxes
// dst (a slab level: two cells / three nodes in y) = the one y-plane of src (the virtual level, same boxes in x and z) in every y-plane
void slab_duplicate(MultiFab& dst, const MultiFab& src);
void gather_to_replicated(MultiFab& repl, const MultiFab& dist);
void scatter_from_replicated(MultiFab& dist, const MultiFab& repl, int ng);

}  // namespace iamrx
