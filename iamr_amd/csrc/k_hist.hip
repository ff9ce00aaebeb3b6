// iamr_amd/csrc/k_hist.hip -- histograms of the components of a cell-centred MultiFab (this library's own diagnostic: the probability
// density functions of iamr_amd/pdf.py; beside the profiles of k_profile.hip and the spectra of k_spectrum.hip).
//
// The binning rule (include/iamrx.h: iamrx_mf_histogram), per column with lo < hi and inv = nbins / (hi - lo) formed once on the host:
//   NaN -> slot nan, v < lo -> slot below, v > hi -> slot above, otherwise bin min((int)((v - lo) * inv), nbins - 1).
// A subtraction followed by a multiplication (this file is compiled with -ffp-contract=off like every other): numpy forms the same bits.
//
//   k_hist   one launch per group of columns whose counters fit the LDS together (16384 32-bit counters = 64 KiB, what a launch may ask
//            for without an attribute; at most 16 columns).  The grid is bounded by the device, not by the level: a workgroup loops over
//            the tiles of the level's flat tile list (launch.h; x fastest across the wavefront, 8 cells in z per thread, all 8 loads of a
//            column unconditional and issued before the first is used) and counts into its own LDS counters with 32-bit integer adds.
//            A lane carries a run length along its z-march and adds it when the bin changes; at the end of the march a wavefront whose
//            lanes all hold the same counter adds their runs with ONE LDS add (a constant or smooth field would otherwise send 64
//            lanes to one address).
//            At its end the workgroup hands its non-zero counters, times the level's weight in 64 bits, to the caller's slots with
//            integer adds to global memory.  Integer addition is associative: the same bits on every call, for every box layout and
//            every rank count.  No floating-point atomics.
//   k_hist2  the joint histogram of two columns: the same march, slot = bx * nby + by; a cell that is NaN or out of range on either axis
//            is counted in a register and reaches the slot `outside` by one wavefront sum.
// A covered cell (cov != 0) is skipped, not multiplied by zero; ghost cells are never read.
#include "kernels.h"
#include "launch.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace iamrx {

namespace {

constexpr int HIST_TZ = 8;                  // cells a thread marches in z per tile (the tz of the tile list)
constexpr int HIST_LDS = 16384;             // 32-bit counters of a workgroup: 64 KiB
constexpr int HIST_MAXCOL = 16;             // columns of one launch

struct HistCols {
    int ncol, nbins, nby;                   // k_hist: ncol columns of nbins bins; k_hist2: columns 0 (x, nbins bins) and 1 (y, nby bins)
    int comp[HIST_MAXCOL];
    double lo[HIST_MAXCOL], hi[HIST_MAXCOL], inv[HIST_MAXCOL];
};

// bins 0 .. nbins - 1, then below, above, nan
__device__ __forceinline__ int hist_bin(double v, double lo, double hi, double inv, int nbins)
{
    if (v != v) return nbins + 2;
    if (v < lo) return nbins;
    if (v > hi) return nbins + 1;
    const int b = (int)((v - lo) * inv);
    return b < nbins - 1 ? b : nbins - 1;
}

// end of a lane's march: every lane of the wavefront arrives with (counter, run length), run = 0: nothing to add
__device__ __forceinline__ void hist_flush(unsigned* h, int cur, unsigned run)
{
    const unsigned long long act = __ballot(run > 0);
    if (act == 0) return;
    const int first = __shfl(cur, __builtin_ctzll(act), 64);
    if (__all(run == 0 || cur == first)) {
        for (int off = 32; off > 0; off >>= 1) run += __shfl_down(run, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&h[first], run);
    } else if (run > 0) atomicAdd(&h[cur], run);
}

// the thread's column of tile `it`: (i, j) clamped into the box (a thread outside it reads the box's last column and counts nothing),
// first plane ka, planes nk (the same for the whole tile); bit m of the result: cell (i, j, ka + m) is counted.  Every load of the
// march is unconditional and inside the box (plane min(m, nk - 1)), so that all of them are in flight together.
template <bool MASK>
__device__ __forceinline__ unsigned hist_cells(const int4 it, const BoxD& b, const FabD* __restrict__ cov, int& i, int& j, int& ka, int& nk)
{
    const int bxs = it.w >> 26;
    i = b.lo[0] + it.y + ((int)threadIdx.x & ((1 << bxs) - 1));
    j = b.lo[1] + it.z + ((int)threadIdx.x >> bxs);
    ka = b.lo[2] + (it.w & ((1 << 26) - 1));
    nk = min(HIST_TZ, b.hi[2] - ka + 1);
    const bool in = i <= b.hi[0] && j <= b.hi[1];
    i = min(i, b.hi[0]); j = min(j, b.hi[1]);
    unsigned live = in ? (1u << nk) - 1u : 0u;
    if (MASK) {
        const FabD c = cov[it.x];
        const auto cp = c.gp() + c.off(i, j, ka);
        const long cks = (long)c.n[0] * c.n[1];
        double cv[HIST_TZ];
#pragma unroll
        for (int m = 0; m < HIST_TZ; ++m) cv[m] = cp[min(m, nk - 1) * cks];
#pragma unroll
        for (int m = 0; m < HIST_TZ; ++m)
            if (cv[m] != 0.0) live &= ~(1u << m);
    }
    return live;
}

template <bool MASK>
__global__ void __launch_bounds__(256) k_hist(const int4* __restrict__ tiles, int ntiles, const BoxD* __restrict__ boxes, const FabD* __restrict__ st,
                                              const FabD* __restrict__ cov, HistCols hc, unsigned long long weight, unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned hist_lds[];
    const int nslot = hc.nbins + 3, ntot = hc.ncol * nslot;
    for (int s = threadIdx.x; s < ntot; s += 256) hist_lds[s] = 0u;
    __syncthreads();
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int4 it = tiles[t];
        const BoxD b = boxes[it.x];
        int i, j, ka, nk;
        const unsigned live = hist_cells<MASK>(it, b, cov, i, j, ka, nk);
        const FabD s = st[it.x];
        const long ks = (long)s.n[0] * s.n[1];
        const long o = s.off(i, j, ka);
        for (int q = 0; q < hc.ncol; ++q) {
            const auto p = s.gp() + o + s.cs * hc.comp[q];
            double v[HIST_TZ];
#pragma unroll
            for (int m = 0; m < HIST_TZ; ++m) v[m] = p[min(m, nk - 1) * ks];
            const double lo = hc.lo[q], hi = hc.hi[q], inv = hc.inv[q];
            unsigned* h = hist_lds + q * nslot;
            int cur = 0;
            unsigned run = 0u;
#pragma unroll
            for (int m = 0; m < HIST_TZ; ++m) {
                if (!(live >> m & 1u)) continue;
                const int bn = hist_bin(v[m], lo, hi, inv, hc.nbins);
                if (bn != cur) { if (run) atomicAdd(&h[cur], run); cur = bn; run = 0u; }
                ++run;
            }
            hist_flush(h, cur, run);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < ntot; s += 256) {
        const unsigned c = hist_lds[s];
        if (c) atomicAdd(&counts[s], (unsigned long long)c * weight);
    }
}

template <bool MASK>
__global__ void __launch_bounds__(256) k_hist2(const int4* __restrict__ tiles, int ntiles, const BoxD* __restrict__ boxes, const FabD* __restrict__ stx,
                                               const FabD* __restrict__ sty, const FabD* __restrict__ cov, HistCols hc, unsigned long long weight,
                                               unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned hist_lds[];
    const int ntot = hc.nbins * hc.nby;
    for (int s = threadIdx.x; s < ntot; s += 256) hist_lds[s] = 0u;
    __syncthreads();
    unsigned outside = 0u;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int4 it = tiles[t];
        const BoxD b = boxes[it.x];
        int i, j, ka, nk;
        const unsigned live = hist_cells<MASK>(it, b, cov, i, j, ka, nk);
        const FabD sx = stx[it.x], sy = sty[it.x];
        const long kx = (long)sx.n[0] * sx.n[1], ky = (long)sy.n[0] * sy.n[1];
        const auto px = sx.gp() + sx.off(i, j, ka) + sx.cs * hc.comp[0];
        const auto py = sy.gp() + sy.off(i, j, ka) + sy.cs * hc.comp[1];
        double x[HIST_TZ], y[HIST_TZ];
#pragma unroll
        for (int m = 0; m < HIST_TZ; ++m) { x[m] = px[min(m, nk - 1) * kx]; y[m] = py[min(m, nk - 1) * ky]; }
        int cur = 0;
        unsigned run = 0u;
#pragma unroll
        for (int m = 0; m < HIST_TZ; ++m) {
            if (!(live >> m & 1u)) continue;
            const int bx = hist_bin(x[m], hc.lo[0], hc.hi[0], hc.inv[0], hc.nbins), by = hist_bin(y[m], hc.lo[1], hc.hi[1], hc.inv[1], hc.nby);
            if (bx >= hc.nbins || by >= hc.nby) { ++outside; continue; }
            const int bn = bx * hc.nby + by;
            if (bn != cur) { if (run) atomicAdd(&hist_lds[cur], run); cur = bn; run = 0u; }
            ++run;
        }
        hist_flush(hist_lds, cur, run);
    }
    for (int off = 32; off > 0; off >>= 1) outside += __shfl_down(outside, off, 64);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&counts[ntot], (unsigned long long)outside * weight);
    __syncthreads();
    for (int s = threadIdx.x; s < ntot; s += 256) {
        const unsigned c = hist_lds[s];
        if (c) atomicAdd(&counts[s], (unsigned long long)c * weight);
    }
}

// workgroups of a launch: enough to fill the device a few times over, never more than there are tiles
int hist_grid(int ntiles)
{
    static const int ncu = [] {
        int dev = 0, n = 0;
        IAMRX_HIP_CHECK(hipGetDevice(&dev));
        IAMRX_HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        return std::max(n, 1);
    }();
    return std::max(1, std::min(ntiles, 4 * ncu));
}

void hist_column(HistCols& hc, int q, int comp, double lo, double hi, int nbins)
{
    hc.comp[q] = comp; hc.lo[q] = lo; hc.hi[q] = hi; hc.inv[q] = (double)nbins / (hi - lo);
}

// this rank counts the level?  (a level every rank holds in full is counted once)
bool hist_counts_here(const Layout& l)
{
    auto& ctx = Context::get();
    const int nranks = ctx.comm ? ctx.comm->nranks : 1, rank = ctx.comm ? ctx.comm->rank : 0;
    return l.nlocal() > 0 && !(l.replicated && nranks > 1 && rank != 0);
}

void hist_check_arrays(const char* who, const MultiFab& S, const MultiFab* cov)
{
    if (!S.type.cell()) throw Error(std::string(who) + ": the array is not cell-centred");
    if (cov && (!cov->type.cell() || cov->layout->id != S.layout->id)) throw Error(std::string(who) + ": the coverage array is not a cell-centred array on the layout of the data");
}

}  // namespace

void hist_check_range(const char* who, double lo, double hi, int nbins, int nbins_max)
{
    if (nbins < 1 || nbins > nbins_max) throw Error(std::string(who) + ": nbins = " + std::to_string(nbins) + " outside 1 .. " + std::to_string(nbins_max));
    if (!std::isfinite(lo) || !std::isfinite(hi)) throw Error(std::string(who) + ": the bounds lo = " + std::to_string(lo) + ", hi = " + std::to_string(hi) + " must be finite");
    if (!(hi > lo)) throw Error(std::string(who) + ": hi = " + std::to_string(hi) + " must be greater than lo = " + std::to_string(lo));
    if (!std::isfinite(hi - lo)) throw Error(std::string(who) + ": hi - lo overflows");
}

DevBuf<unsigned long long> hist_begin(size_t nslots)
{
    DevBuf<unsigned long long> d(nslots);
    IAMRX_HIP_CHECK(hipMemsetAsync(d, 0, nslots * sizeof(unsigned long long), Context::get().stream));
    return d;
}

void hist_add(const MultiFab& S, int ncol, const int* comps, const MultiFab* cov, const double* lo, const double* hi, int nbins,
              unsigned long long weight, unsigned long long* d_counts)
{
    hist_check_arrays("histogram", S, cov);
    for (int q = 0; q < ncol; ++q) {
        hist_check_range("histogram", lo[q], hi[q], nbins, HIST_NBINS_MAX);
        if (comps[q] < 0 || comps[q] >= S.ncomp) throw Error("histogram: component " + std::to_string(comps[q]) + " outside the array's " + std::to_string(S.ncomp));
    }
    if (!hist_counts_here(*S.layout)) return;
    auto& ctx = Context::get();
    int ntiles = 0;
    const int4* tiles = level_tile_list(*S.layout, cell_type(), 0, HIST_TZ, &ntiles);
    if (ntiles == 0) return;
    const int nslot = nbins + 3, per = std::min(HIST_MAXCOL, HIST_LDS / nslot);
    const dim3 g((unsigned)hist_grid(ntiles)), blk(256);
    for (int q0 = 0; q0 < ncol; q0 += per) {            // columns that do not fit the LDS together: one pass over memory per group
        HistCols hc;
        hc.ncol = std::min(per, ncol - q0); hc.nbins = nbins; hc.nby = 0;
        for (int q = 0; q < hc.ncol; ++q) hist_column(hc, q, comps[q0 + q], lo[q0 + q], hi[q0 + q], nbins);
        const size_t lds = (size_t)hc.ncol * nslot * sizeof(unsigned);
        unsigned long long* out = d_counts + (size_t)q0 * nslot;
        if (cov) hipLaunchKernelGGL((k_hist<true>), g, blk, lds, ctx.stream, tiles, ntiles, S.layout->d_boxes, S.d_tab, cov->d_tab, hc, weight, out);
        else hipLaunchKernelGGL((k_hist<false>), g, blk, lds, ctx.stream, tiles, ntiles, S.layout->d_boxes, S.d_tab, (const FabD*)nullptr, hc, weight, out);
    }
}

void hist_add2(const MultiFab& X, int compx, const MultiFab& Y, int compy, const MultiFab* cov, const double lo[2], const double hi[2],
               const int nbins[2], unsigned long long weight, unsigned long long* d_counts)
{
    hist_check_arrays("histogram2", X, cov);
    hist_check_arrays("histogram2", Y, nullptr);
    if (X.layout->id != Y.layout->id) throw Error("histogram2: the two arrays live on different layouts");
    for (int a = 0; a < 2; ++a) hist_check_range("histogram2", lo[a], hi[a], nbins[a], HIST2_SLOTS_MAX);
    if ((long)nbins[0] * nbins[1] > HIST2_SLOTS_MAX)
        throw Error("histogram2: nbins = " + std::to_string(nbins[0]) + " x " + std::to_string(nbins[1]) + " exceeds " + std::to_string(HIST2_SLOTS_MAX) + " slots");
    if (compx < 0 || compx >= X.ncomp || compy < 0 || compy >= Y.ncomp) throw Error("histogram2: component outside the array");
    if (!hist_counts_here(*X.layout)) return;
    auto& ctx = Context::get();
    int ntiles = 0;
    const int4* tiles = level_tile_list(*X.layout, cell_type(), 0, HIST_TZ, &ntiles);
    if (ntiles == 0) return;
    HistCols hc;
    hc.ncol = 2; hc.nbins = nbins[0]; hc.nby = nbins[1];
    hist_column(hc, 0, compx, lo[0], hi[0], nbins[0]);
    hist_column(hc, 1, compy, lo[1], hi[1], nbins[1]);
    const size_t lds = (size_t)nbins[0] * nbins[1] * sizeof(unsigned);
    const dim3 g((unsigned)hist_grid(ntiles)), blk(256);
    if (cov) hipLaunchKernelGGL((k_hist2<true>), g, blk, lds, ctx.stream, tiles, ntiles, X.layout->d_boxes, X.d_tab, Y.d_tab, cov->d_tab, hc, weight, d_counts);
    else hipLaunchKernelGGL((k_hist2<false>), g, blk, lds, ctx.stream, tiles, ntiles, X.layout->d_boxes, X.d_tab, Y.d_tab, (const FabD*)nullptr, hc, weight, d_counts);
}

void hist_end(const unsigned long long* d_counts, size_t nslots, long long* out)
{
    auto& ctx = Context::get();
    std::vector<unsigned long long> h(nslots);
    IAMRX_HIP_CHECK(hipMemcpyAsync(h.data(), d_counts, nslots * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    const unsigned long long lim = 1ULL << 53;
    if (ctx.comm && ctx.comm->nranks > 1) {
        // the transport carries doubles: integers below 2^53 are summed exactly
        std::vector<double> v(nslots + 1);
        double tot = 0.0;
        for (size_t s = 0; s < nslots; ++s) { if (h[s] >= lim) throw Error("histogram: a slot reached 2^53"); v[s] = (double)h[s]; tot += v[s]; }
        v[nslots] = tot;
        ctx.comm->allreduce(v.data(), (int)(nslots + 1), ReduceOp::Sum);
        if (!(v[nslots] < (double)lim)) throw Error("histogram: the counts of all ranks together reach 2^53");
        for (size_t s = 0; s < nslots; ++s) out[s] = (long long)v[s];
    } else {
        for (size_t s = 0; s < nslots; ++s) { if (h[s] >= lim) throw Error("histogram: a slot reached 2^53"); out[s] = (long long)h[s]; }
    }
}

void hist_bench(const MultiFab& S, int ncol, const int* comps, const MultiFab* cov, const double* lo, const double* hi, int nbins, int nby, int reps, float* ms)
{
    IAMRX_ASSERT(reps >= 1 && ms && ncol >= 1 && (nby == 0 || ncol == 2));
    auto& ctx = Context::get();
    const size_t nslots = nby > 0 ? (size_t)nbins * nby + 1 : (size_t)ncol * (nbins + 3);
    const DevBuf<unsigned long long> d = hist_begin(nslots);
    const int nb2[2] = {nbins, nby};
    PassTimer t(2);
    for (int r = 0; r < reps; ++r) {
        t.mark();
        if (nby > 0) hist_add2(S, comps[0], S, comps[1], cov, lo, hi, nb2, 1ULL, d);
        else hist_add(S, ncol, comps, cov, lo, hi, nbins, 1ULL, d);
        t.mark();
        t.finish(ms + r);
    }
    ctx.sync();
}

}  // namespace iamrx
