// iamr_amd/csrc/k_profile.hip -- plane-averaged profiles of the composite state along one axis (this library's own diagnostic: the
// middle ground between the time-averaged fields of k_stats.hip and the three domain integrals of k_sum_integrated).
//
// For every level one launch forms the sums of the PROFILE_NQ = 14 quantities 1, u, v, w, rho, c, uu, vv, ww, uv, uw, vw, rho rho, c c
// over the uncovered cells of each index plane of THAT level along the axis `dir` (its own index space, over the extent of the level's
// bounding box).  All three axes read with x fastest across the wavefront:
//   dir = 1, 2  k_profile_plane: a workgroup owns (box, plane, a range of rows of the plane); its threads stride over the cells of those
//               rows (x contiguous) with 14 accumulators in registers, then one shuffle + LDS combine per quantity.
//   dir = 0     k_profile_x: the bin index is the contiguous one.  A workgroup owns (box, up to 64 columns i, a range of (j, k) rows); a
//               lane keeps its own i and accumulates over the rows of its wavefront; the wavefronts that hold the same i combine
//               through LDS.  Boxes narrower than a wavefront put 64 / BX rows side by side in one wavefront.
// Every workgroup writes its sums to slots of its own (no atomics); k_profile_bins adds the slots of each plane in a fixed order (a
// per-layout list), k_profile_fold adds the levels 0 .. F into the output bins.  The same call gives the same bits.
#include "kernels.h"
#include "launch.h"
#include <algorithm>
#include <climits>

namespace iamrx {

namespace {

constexpr int NQ = PROFILE_NQ;
constexpr int PROFILE_CELLS = 8192;      // cells per workgroup (32 per thread): enough loads in flight, ~2000 workgroups for a 256^3 box
constexpr int PROFILE_MAXLEV = 16;

// the 14 terms of one cell
__device__ __forceinline__ void profile_add(double (&a)[NQ], double u, double v, double w, double r, double c)
{
    a[0] += 1.0; a[1] += u; a[2] += v; a[3] += w; a[4] += r; a[5] += c;
    a[6] += u * u; a[7] += v * v; a[8] += w * w; a[9] += u * v; a[10] += u * w; a[11] += v * w; a[12] += r * r; a[13] += c * c;
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;       // valid in lane 0
}

// work item = two int4: (fab, plane offset in the box along dir, first row, rows), (slot, 0, 0, 0); rows run along the third axis
// (dir = 2: j, dir = 1: k).  A covered cell (MASK: cov != 0) is skipped, so that what it holds cannot reach a sum.
template <bool MASK>
__global__ void __launch_bounds__(256) k_profile_plane(const int4* __restrict__ items, const BoxD* __restrict__ boxes, const FabD* __restrict__ st,
                                                       const FabD* __restrict__ cov, int dir, int rho_comp, int trac_comp,
                                                       double* __restrict__ partials, long nslots)
{
    const int4 it = items[2 * blockIdx.x];
    const int slot = items[2 * blockIdx.x + 1].x;
    const BoxD b = boxes[it.x];
    const FabD s = st[it.x];
    // (selects, not arrays indexed by dir: a run-time index into a local array would put it into scratch memory)
    const int nx = b.len(0);
    const int bloD = dir == 1 ? b.lo[1] : b.lo[2], bloE = dir == 1 ? b.lo[2] : b.lo[1];
    const long sstrD = dir == 1 ? (long)s.n[0] : (long)s.n[0] * s.n[1], sstrE = dir == 1 ? (long)s.n[0] * s.n[1] : (long)s.n[0];
    const int sloD = dir == 1 ? s.lo[1] : s.lo[2], sloE = dir == 1 ? s.lo[2] : s.lo[1];
    const long s0 = (long)(b.lo[0] - s.lo[0]) + sstrD * (bloD + it.y - sloD) + sstrE * (bloE + it.z - sloE);
    const auto sp = s.gp();
    decltype(s.gp()) cp = nullptr;      // (FabD::gp: a global-address-space pointer in device code)
    long c0 = 0, cstrE = 0;
    if (MASK) {
        const FabD c = cov[it.x];
        const long cstrD = dir == 1 ? (long)c.n[0] : (long)c.n[0] * c.n[1];
        const int cloD = dir == 1 ? c.lo[1] : c.lo[2], cloE = dir == 1 ? c.lo[2] : c.lo[1];
        cstrE = dir == 1 ? (long)c.n[0] * c.n[1] : (long)c.n[0];
        c0 = (long)(b.lo[0] - c.lo[0]) + cstrD * (bloD + it.y - cloD) + cstrE * (bloE + it.z - cloE);
        cp = c.gp();
    }
    double a[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = 0.0;
    // cell p of the item = (i, row) = (p % nx, p / nx), advanced by 256 without a division
    const int di = 256 % nx, de = 256 / nx;
    int i = (int)threadIdx.x % nx, e = (int)threadIdx.x / nx;
    for (; e < it.w; i += di, e += de) {
        if (i >= nx) { i -= nx; if (++e >= it.w) break; }
        if (MASK && cp[c0 + i + cstrE * e] != 0.0) continue;
        const long o = s0 + i + sstrE * e;
        const double u = sp[o], v = sp[o + s.cs], w = sp[o + 2 * s.cs], r = sp[o + rho_comp * s.cs], c = sp[o + trac_comp * s.cs];
        profile_add(a, u, v, w, r, c);
    }
    __shared__ double sm[NQ][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; ++q) { const double v = wave_sum(a[q]); if (lane == 0) sm[q][wv] = v; }
    __syncthreads();
    if (threadIdx.x < NQ) partials[threadIdx.x * nslots + slot] = ((sm[threadIdx.x][0] + sm[threadIdx.x][1]) + sm[threadIdx.x][2]) + sm[threadIdx.x][3];
}

// work item = two int4: (fab, first column offset, first row, rows), (first slot, log2 BX, 0, 0); row r = (j, k) = (r % ny, r / ny).
// The item's columns i0 .. i0 + BX - 1 (those inside the box) each own one slot.
template <bool MASK>
__global__ void __launch_bounds__(256) k_profile_x(const int4* __restrict__ items, const BoxD* __restrict__ boxes, const FabD* __restrict__ st,
                                                   const FabD* __restrict__ cov, int rho_comp, int trac_comp, double* __restrict__ partials, long nslots)
{
    const int4 it = items[2 * blockIdx.x];
    const int4 it2 = items[2 * blockIdx.x + 1];
    const BoxD b = boxes[it.x];
    const FabD s = st[it.x];
    const int bxs = it2.y, bx = 1 << bxs, nsub = 256 >> bxs;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ii = lane & (bx - 1), sub = (wv << (6 - bxs)) + (lane >> bxs);
    const int i = b.lo[0] + it.y + ii, ny = b.len(1);
    double a[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = 0.0;
    if (i <= b.hi[0]) {
        const auto sp = s.gp();
        FabD c;
        if (MASK) c = cov[it.x];
        const int dj = nsub % ny, dk = nsub / ny;
        const int r0 = it.z + sub;
        int j = r0 % ny, k = r0 / ny;
        for (int r = r0; r < it.z + it.w; r += nsub, j += dj, k += dk) {
            if (j >= ny) { j -= ny; ++k; }
            if (MASK && c(i, b.lo[1] + j, b.lo[2] + k) != 0.0) continue;
            const long o = s.off(i, b.lo[1] + j, b.lo[2] + k);
            const double u = sp[o], v = sp[o + s.cs], w = sp[o + 2 * s.cs], r_ = sp[o + rho_comp * s.cs], c_ = sp[o + trac_comp * s.cs];
            profile_add(a, u, v, w, r_, c_);
        }
    }
    // rows side by side in one wavefront (BX < 64), then the wavefronts through LDS: wavefront 0 adds 1, 2, 3 in this order
    __shared__ double sm[NQ][3][64];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double v = a[q];
        for (int off = 32; off >= bx; off >>= 1) v += __shfl_down(v, off, 64);
        a[q] = v;
        if (wv > 0) sm[q][wv - 1][lane] = v;
    }
    __syncthreads();
    if (wv == 0 && lane < bx && i <= b.hi[0]) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) partials[q * nslots + it2.x + ii] = ((a[q] + sm[q][0][lane]) + sm[q][1][lane]) + sm[q][2][lane];
    }
}

// stage 2: one wavefront per (quantity, plane of the level): lev[q * next + b] = sum of the slots slots[ptr[b] .. ptr[b + 1]) in a fixed order
__global__ void __launch_bounds__(256) k_profile_bins(const double* __restrict__ partials, long nslots, const int* __restrict__ ptr,
                                                      const int* __restrict__ slots, int next, double* __restrict__ lev)
{
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wid >= NQ * next) return;
    const int q = wid / next, b = wid - q * next;
    double v = 0.0;
    for (int s = ptr[b] + lane; s < ptr[b + 1]; s += 64) v += partials[q * nslots + slots[s]];
    v = wave_sum(v);
    if (lane == 0) lev[wid] = v;
}

// the levels' plane sums -> the output bins (index space of level B).  A level finer than B adds 2^(l - B) neighbouring planes; a coarser
// one spreads its plane over the 2^(B - l) bins it spans.  w[l] = cell volume of level l (the share of it inside one bin) / slab volume.
struct ProfileFold {
    int nlev, B, nbins;
    int off[PROFILE_MAXLEV], lo[PROFILE_MAXLEV], n[PROFILE_MAXLEV];     // level sums at base + off; planes lo .. lo + n - 1 (from the domain's low end)
    double w[PROFILE_MAXLEV];
};
__global__ void __launch_bounds__(256) k_profile_fold(ProfileFold f, const double* __restrict__ base, double* __restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= NQ * f.nbins) return;
    const int q = t / f.nbins, bin = t - q * f.nbins;
    double acc = 0.0;
    for (int l = 0; l < f.nlev; ++l) {
        const double* lv = base + f.off[l] + (size_t)q * f.n[l];
        if (l <= f.B) {
            const int p = (bin >> (f.B - l)) - f.lo[l];
            if (p >= 0 && p < f.n[l]) acc += f.w[l] * lv[p];
        } else {
            const int sh = l - f.B;
            double s = 0.0;
            bool any = false;
            for (int m = 0; m < (1 << sh); ++m) {
                const int p = (bin << sh) + m - f.lo[l];
                if (p >= 0 && p < f.n[l]) { s += lv[p]; any = true; }
            }
            if (any) acc += f.w[l] * s;
        }
    }
    out[t] = acc;
}

// extent of a level along dir: the bounding box of ALL its boxes (the same on every rank)
void profile_extent(const Layout& l, int dir, int& lo, int& n)
{
    int a = INT_MAX, b = INT_MIN;
    for (const BoxD& bx : l.boxes) { a = std::min(a, bx.lo[dir]); b = std::max(b, bx.hi[dir]); }
    lo = a; n = b - a + 1;
}

// the work items of the local boxes and, per plane of the extent, the slots that hold its partial sums (in item order)
void profile_work(const Layout& l, int dir, std::vector<int4>& items, std::vector<std::vector<int>>& per_bin, long& nslots)
{
    int lo, n;
    profile_extent(l, dir, lo, n);
    per_bin.assign(n, {});
    items.clear();
    int slot = 0;
    for (int f = 0; f < l.nlocal(); ++f) {
        const BoxD& b = l.lbox(f);
        if (dir == 0) {
            int bx = 64, bxs = 6;
            while (bx > 4 && bx / 2 >= b.len(0)) { bx /= 2; --bxs; }
            const int rows = b.len(1) * b.len(2), rc = PROFILE_CELLS / bx;
            for (int i0 = 0; i0 < b.len(0); i0 += bx)
                for (int r0 = 0; r0 < rows; r0 += rc) {
                    const int nb = std::min(bx, b.len(0) - i0);
                    items.push_back(make_int4(f, i0, r0, std::min(rc, rows - r0)));
                    items.push_back(make_int4(slot, bxs, 0, 0));
                    for (int q = 0; q < nb; ++q) per_bin[b.lo[0] + i0 + q - lo].push_back(slot + q);
                    slot += nb;
                }
        } else {
            const int E = 3 - dir, rc = std::max(1, PROFILE_CELLS / b.len(0));
            for (int c = 0; c < b.len(dir); ++c)
                for (int r0 = 0; r0 < b.len(E); r0 += rc) {
                    items.push_back(make_int4(f, c, r0, std::min(rc, b.len(E) - r0)));
                    items.push_back(make_int4(slot, 0, 0, 0));
                    per_bin[b.lo[dir] + c - lo].push_back(slot++);
                }
        }
    }
    nslots = slot;
}

// device copies, built once per (layout, dir): which = 0 the items, 1 the bin pointers followed by the slot list (ints, padded to int4)
const int4* profile_list(const Layout& l, int dir, int which, int* total)
{
    return layout_int4_list(l, {4, dir, which, 0, 0}, [&](std::vector<int4>& h) {
        std::vector<int4> items;
        std::vector<std::vector<int>> per_bin;
        long nslots;
        profile_work(l, dir, items, per_bin, nslots);
        if (which == 0) { h = items; return; }
        std::vector<int> v(per_bin.size() + 1, 0);
        for (size_t b = 0; b < per_bin.size(); ++b) v[b + 1] = v[b] + (int)per_bin[b].size();
        for (const auto& pb : per_bin) v.insert(v.end(), pb.begin(), pb.end());
        v.resize((v.size() + 3) / 4 * 4, 0);
        for (size_t q = 0; q < v.size(); q += 4) h.push_back(make_int4(v[q], v[q + 1], v[q + 2], v[q + 3]));
    }, total);
}

// the number of slots of the local boxes (profile_work's count without the lists)
long profile_nslots(const Layout& l, int dir)
{
    long n = 0;
    for (int f = 0; f < l.nlocal(); ++f) {
        const BoxD& b = l.lbox(f);
        if (dir == 0) {
            int bx = 64;
            while (bx > 4 && bx / 2 >= b.len(0)) bx /= 2;
            const long rows = (long)b.len(1) * b.len(2), rc = PROFILE_CELLS / bx;
            n += (long)b.len(0) * ((rows + rc - 1) / rc);
        } else {
            const int E = 3 - dir, rc = std::max(1, PROFILE_CELLS / b.len(0));
            n += (long)b.len(dir) * ((b.len(E) + rc - 1) / rc);
        }
    }
    return n;
}

}  // namespace

int profile_nbins(const Geometry& g0, int dir, int bin_level) { return g0.domain.len(dir) << bin_level; }

void profile_reduce(int nlev, const ProfileLevel* L, int dir, int bin_level, int rho_comp, int trac_comp, double* out)
{
    IAMRX_ASSERT(nlev >= 1 && nlev <= PROFILE_MAXLEV && dir >= 0 && dir <= 2 && bin_level >= 0 && bin_level < nlev);
    auto& ctx = Context::get();
    const int nranks = ctx.comm ? ctx.comm->nranks : 1, rank = ctx.comm ? ctx.comm->rank : 0;
    ProfileFold f;
    f.nlev = nlev; f.B = bin_level; f.nbins = profile_nbins(*L[0].g, dir, bin_level);
    int total = 0;
    for (int l = 0; l < nlev; ++l) {
        const MultiFab& S = *L[l].S;
        IAMRX_ASSERT(S.type.cell() && (!L[l].cov || (L[l].cov->type.cell() && L[l].cov->layout->id == S.layout->id)));
        int lo;
        profile_extent(*S.layout, dir, lo, f.n[l]);
        f.lo[l] = lo - L[l].g->domain.lo[dir];
        f.off[l] = total;
        total += NQ * f.n[l];
        // cell volume (its share inside one bin) / slab volume = 1 / (cells of the level in a plane, times the planes per bin)
        const BoxD& d = L[l].g->domain;
        const long nperp = (long)d.len((dir + 1) % 3) * d.len((dir + 2) % 3);
        f.w[l] = 1.0 / (double)(nperp << std::max(l - bin_level, 0));
    }
    const size_t nout = (size_t)NQ * f.nbins;
    DevBuf<double> buf(total + nout);
    for (int l = 0; l < nlev; ++l) {
        const MultiFab& S = *L[l].S;
        const Layout& lay = *S.layout;
        double* lev = buf + f.off[l];
        // a level every rank holds in full is counted once
        if (lay.nlocal() == 0 || (lay.replicated && nranks > 1 && rank != 0)) {
            IAMRX_HIP_CHECK(hipMemsetAsync(lev, 0, (size_t)NQ * f.n[l] * sizeof(double), ctx.stream));
            continue;
        }
        int n_items = 0, n_csr = 0;
        const int4* items = profile_list(lay, dir, 0, &n_items);
        const int* csr = (const int*)profile_list(lay, dir, 1, &n_csr);
        n_items /= 2;
        const long nslots = profile_nslots(lay, dir);
        DevBuf<double> part((size_t)NQ * nslots);           // freed behind the launches of this level that use it (DevBuf, mf.h)
        double* partials = part;
        const FabD* cov = L[l].cov ? L[l].cov->d_tab : nullptr;
        const dim3 g((unsigned)n_items), blk(256);
        if (dir == 0) {
            if (cov) hipLaunchKernelGGL((k_profile_x<true>), g, blk, 0, ctx.stream, items, lay.d_boxes, S.d_tab, cov, rho_comp, trac_comp, partials, nslots);
            else hipLaunchKernelGGL((k_profile_x<false>), g, blk, 0, ctx.stream, items, lay.d_boxes, S.d_tab, cov, rho_comp, trac_comp, partials, nslots);
        } else {
            if (cov) hipLaunchKernelGGL((k_profile_plane<true>), g, blk, 0, ctx.stream, items, lay.d_boxes, S.d_tab, cov, dir, rho_comp, trac_comp, partials, nslots);
            else hipLaunchKernelGGL((k_profile_plane<false>), g, blk, 0, ctx.stream, items, lay.d_boxes, S.d_tab, cov, dir, rho_comp, trac_comp, partials, nslots);
        }
        hipLaunchKernelGGL(k_profile_bins, dim3((unsigned)((NQ * f.n[l] + 3) / 4)), blk, 0, ctx.stream, partials, nslots, csr, csr + f.n[l] + 1, f.n[l], lev);
    }
    double* d_out = buf + total;
    hipLaunchKernelGGL(k_profile_fold, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ctx.stream, f, buf, d_out);
    if (nranks > 1) ctx.comm->allreduce_device(d_out, (int)nout, ReduceOp::Sum, ctx.stream);
    const double* h = ctx.read_back(d_out, nout);
    std::copy(h, h + nout, out);
}

}  // namespace iamrx
