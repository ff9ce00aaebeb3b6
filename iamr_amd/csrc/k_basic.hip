// iamr_amd/csrc/k_basic.hip -- streaming kernels: fill, plan copies (ghost exchange), BLAS-1 style
// fused ops and deterministic two-stage reductions (block partials -> single-block finish).
// Role: amrex MultiFab::{setVal,Copy,Saxpy,Xpay,mult,norm0}, FillBoundary pack/unpack.
#include "kernels.h"
#include "launch.h"
#include <algorithm>

namespace iamrx {

__global__ void __launch_bounds__(256) k_fill(double* __restrict__ p, size_t n, double v)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) p[i] = v;
}

void launch_fill(double* p, size_t n, double v, hipStream_t s)
{
    if (n == 0) return;
    size_t nb = (n + 255) / 256;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)nb), dim3(256), 0, s, p, n, v);
}

// one blockIdx.y per copy descriptor; threads stride over region points (x fastest => coalesced rows)
__global__ void __launch_bounds__(256) k_copy_plan(const CopyDesc* __restrict__ descs, const FabD* __restrict__ src,
                                                   const FabD* __restrict__ dst, int scomp, int dcomp, int nc, int add)
{
    const CopyDesc cd = descs[blockIdx.y];
    const int nx = cd.region.len(0), ny = cd.region.len(1);
    const long npts = cd.npts();
    const FabD s = src[cd.src_fab], d = dst[cd.dst_fab];
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < npts; q += (long)gridDim.x * 256) {
        const int i = cd.region.lo[0] + (int)(q % nx);
        const long r = q / nx;
        const int j = cd.region.lo[1] + (int)(r % ny);
        const int k = cd.region.lo[2] + cd.kstep * (int)(r / ny);
        if (add) for (int n = 0; n < nc; ++n) d(i, j, k, dcomp + n) += s(i + cd.shift[0], j + cd.shift[1], k + cd.shift[2], scomp + n);
        else for (int n = 0; n < nc; ++n) d(i, j, k, dcomp + n) = s(i + cd.shift[0], j + cd.shift[1], k + cd.shift[2], scomp + n);
    }
}

void launch_copy_plan(const CopyDesc* d, int nd, long maxpts, const FabD* src, const FabD* dst, int scomp, int dcomp, int nc, hipStream_t s, bool add)
{
    if (nd == 0) return;
    // whole-array copies between layouts (one descriptor of millions of points) want thousands of workgroups in flight; a ghost-shell
    // exchange (many small descriptors: the grid's y dimension) keeps its short x dimension
    long nb = (maxpts + 255) / 256;
    const long cap = nd >= 8 ? 256 : 4096;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_copy_plan, dim3((unsigned)nb, (unsigned)nd), dim3(256), 0, s, d, src, dst, scomp, dcomp, nc, add ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_pack(const CopyDesc* __restrict__ descs, const FabD* __restrict__ src,
                                              double* __restrict__ buf, long pts_total, int scomp, int nc)
{
    const CopyDesc cd = descs[blockIdx.y];
    const int nx = cd.region.len(0), ny = cd.region.len(1);
    const long npts = cd.npts();
    const FabD s = src[cd.src_fab];
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < npts; q += (long)gridDim.x * 256) {
        const int i = cd.region.lo[0] + (int)(q % nx);
        const long r = q / nx;
        const int j = cd.region.lo[1] + (int)(r % ny);
        const int k = cd.region.lo[2] + cd.kstep * (int)(r / ny);
        for (int n = 0; n < nc; ++n) buf[cd.buf_off + q + pts_total * n] = s(i + cd.shift[0], j + cd.shift[1], k + cd.shift[2], scomp + n);
    }
}

__global__ void __launch_bounds__(256) k_unpack(const CopyDesc* __restrict__ descs, const FabD* __restrict__ dst,
                                                const double* __restrict__ buf, long pts_total, int dcomp, int nc, int add)
{
    const CopyDesc cd = descs[blockIdx.y];
    const int nx = cd.region.len(0), ny = cd.region.len(1);
    const long npts = cd.npts();
    const FabD d = dst[cd.dst_fab];
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < npts; q += (long)gridDim.x * 256) {
        const int i = cd.region.lo[0] + (int)(q % nx);
        const long r = q / nx;
        const int j = cd.region.lo[1] + (int)(r % ny);
        const int k = cd.region.lo[2] + cd.kstep * (int)(r / ny);
        if (add) for (int n = 0; n < nc; ++n) d(i, j, k, dcomp + n) += buf[cd.buf_off + q + pts_total * n];
        else for (int n = 0; n < nc; ++n) d(i, j, k, dcomp + n) = buf[cd.buf_off + q + pts_total * n];
    }
}

void launch_pack(const CopyDesc* d, int nd, long maxpts, const FabD* src, double* buf, long pts_total, int scomp, int nc, hipStream_t s)
{
    if (nd == 0) return;
    long nb = (maxpts + 255) / 256; if (nb > 256) nb = 256; if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_pack, dim3((unsigned)nb, (unsigned)nd), dim3(256), 0, s, d, src, buf, pts_total, scomp, nc);
}
void launch_unpack(const CopyDesc* d, int nd, long maxpts, const FabD* dst, const double* buf, long pts_total, int dcomp, int nc, hipStream_t s, bool add)
{
    if (nd == 0) return;
    long nb = (maxpts + 255) / 256; if (nb > 256) nb = 256; if (nb < 1) nb = 1;
    hipLaunchKernelGGL(k_unpack, dim3((unsigned)nb, (unsigned)nd), dim3(256), 0, s, d, dst, buf, pts_total, dcomp, nc, add ? 1 : 0);
}

// ---- the same over a flat work list: workgroup b takes COPY_CHUNK points of descriptor work[b].x starting at work[b].y * COPY_CHUNK
template <int MODE>       // 0 copy, 1 pack, 2 unpack
__global__ void __launch_bounds__(256) k_copy_work(const CopyDesc* __restrict__ descs, const int2* __restrict__ work, const FabD* __restrict__ src,
                                                   const FabD* __restrict__ dst, double* __restrict__ buf, long pts_total, int scomp, int dcomp, int nc, int add)
{
    const int2 e = work[blockIdx.x];
    const CopyDesc cd = descs[e.x];
    const int nx = cd.region.len(0), ny = cd.region.len(1);
    const long npts = cd.npts();
    FabD s, d;
    if (MODE != 2) s = src[cd.src_fab];
    if (MODE != 1) d = dst[cd.dst_fab];
#pragma unroll
    for (int u = 0; u < COPY_CHUNK / 256; ++u) {
        const long q = (long)e.y * COPY_CHUNK + u * 256 + threadIdx.x;
        if (q >= npts) break;
        const int i = cd.region.lo[0] + (int)(q % nx);
        const long r = q / nx;
        const int j = cd.region.lo[1] + (int)(r % ny);
        const int k = cd.region.lo[2] + cd.kstep * (int)(r / ny);
        for (int n = 0; n < nc; ++n) {
            if (MODE == 0) {
                const double v = s(i + cd.shift[0], j + cd.shift[1], k + cd.shift[2], scomp + n);
                if (add) d(i, j, k, dcomp + n) += v; else d(i, j, k, dcomp + n) = v;
            } else if (MODE == 1) buf[cd.buf_off + q + pts_total * n] = s(i + cd.shift[0], j + cd.shift[1], k + cd.shift[2], scomp + n);
            else {
                const double v = buf[cd.buf_off + q + pts_total * n];
                if (add) d(i, j, k, dcomp + n) += v; else d(i, j, k, dcomp + n) = v;
            }
        }
    }
}
void launch_copy_plan_w(const CopyDesc* d, const int2* w, int nw, const FabD* src, const FabD* dst, int scomp, int dcomp, int nc, hipStream_t s, bool add)
{
    if (nw > 0) hipLaunchKernelGGL((k_copy_work<0>), dim3((unsigned)nw), dim3(256), 0, s, d, w, src, dst, (double*)nullptr, 0L, scomp, dcomp, nc, add ? 1 : 0);
}
void launch_pack_w(const CopyDesc* d, const int2* w, int nw, const FabD* src, double* buf, long pts_total, int scomp, int nc, hipStream_t s)
{
    if (nw > 0) hipLaunchKernelGGL((k_copy_work<1>), dim3((unsigned)nw), dim3(256), 0, s, d, w, src, (const FabD*)nullptr, buf, pts_total, scomp, 0, nc, 0);
}
void launch_unpack_w(const CopyDesc* d, const int2* w, int nw, const FabD* dst, const double* buf, long pts_total, int dcomp, int nc, hipStream_t s, bool add)
{
    if (nw > 0) hipLaunchKernelGGL((k_copy_work<2>), dim3((unsigned)nw), dim3(256), 0, s, d, w, (const FabD*)nullptr, dst, const_cast<double*>(buf), pts_total, 0, dcomp, nc, add ? 1 : 0);
}

// ------------------------------------------------------------------ reductions
// wavefront (64 lanes) shuffle reduction, then LDS across the 4 waves of the workgroup
template <int OP> __device__ __forceinline__ double red_op(double a, double b)
{
    if (OP == 0) return a + b;
    return (a > b || a != a) ? a : b;          // maxima: a NaN operand wins on either side (the functor reductions' partials may hold one)
}
template <int OP> __device__ __forceinline__ double block_reduce(double v)
{
    __shared__ double sm[4];
    for (int off = 32; off > 0; off >>= 1) v = red_op<OP>(v, __shfl_down(v, off, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sm[w] = v;
    __syncthreads();
    if (threadIdx.x == 0) v = red_op<OP>(red_op<OP>(sm[0], sm[1]), red_op<OP>(sm[2], sm[3]));
    return v;   // valid in thread 0
}

// stage 2: out[q] = reduce over partials[q*np .. q*np+np)
template <int OP> __global__ void __launch_bounds__(256) k_reduce_finish(const double* __restrict__ partials, int np, double* __restrict__ out)
{
    const int q = blockIdx.x;
    double v = OP == 2 ? -1.7976931348623157e308 : 0.0;       // OP 2: maximum of signed values
    for (int i = threadIdx.x; i < np; i += 256) v = red_op<OP>(v, partials[(size_t)q * np + i]);
    v = block_reduce<OP>(v);
    if (threadIdx.x == 0) out[q] = v;
}

__global__ void __launch_bounds__(256) k_norm0(Tiling t, const BoxD* __restrict__ boxes, int t0, int t1, int t2, int ng,
                                               const FabD* __restrict__ tab, int comp, int nc, double* __restrict__ partials)
{
    const int fab = tile_fab(t);
    const BoxD b = dev_grow_convert(boxes[fab], t0, t1, t2, ng);
    int i, j, k0, k1;
    double m = 0.0;
    if (tile_ijk(t, b, i, j, k0, k1)) {
        const FabD a = tab[fab];
        for (int n = 0; n < nc; ++n)
            for (int k = k0; k <= k1; ++k) { const double v = norm_term(a(i, j, k, comp + n)); m = v > m ? v : m; }
    }
    m = block_reduce<1>(m);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
}

// Stage 2 of every reduction: the block partials -> nout values on the device; global: combined across the ranks IN PLACE on the device
// (Comm::allreduce_device: ncclAllReduce on the launch stream, no host round trip); then ONE read-back.  np == 0: this rank holds no
// data of the level and contributes the identity (0: sums, and maxima of absolute values).
static double finish_to_host(int op, int nout, int np, bool global)
{
    auto& ctx = Context::get();
    ctx.ensure_scratch((size_t)nout * np + 16);
    double* partials = ctx.d_scratch;
    double* out = ctx.d_scratch + (size_t)nout * np;
    if (np == 0 && op != 2) IAMRX_HIP_CHECK(hipMemsetAsync(out, 0, nout * sizeof(double), ctx.stream));
    else if (op == 0) hipLaunchKernelGGL((k_reduce_finish<0>), dim3(nout), dim3(256), 0, ctx.stream, partials, np, out);
    else if (op == 2) hipLaunchKernelGGL((k_reduce_finish<2>), dim3(nout), dim3(256), 0, ctx.stream, partials, np, out);
    else hipLaunchKernelGGL((k_reduce_finish<1>), dim3(nout), dim3(256), 0, ctx.stream, partials, np, out);
    if (global && ctx.comm->nranks > 1) ctx.comm->allreduce_device(out, nout, op == 0 ? ReduceOp::Sum : ReduceOp::Max, ctx.stream);
    IAMRX_HIP_CHECK(hipMemcpyAsync(ctx.h_scratch, out, nout * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    return ctx.h_scratch[0];
}

// the same, results left ON THE DEVICE at d_out[0 .. nout) (no read-back, no host synchronisation): the device-resident Krylov loop
// (krylov.h) consumes them from there.  op 0: sums, 1: maxima of absolute values
void reduce_finish_dev(int op, int nout, int np, bool global, double* d_out)
{
    auto& ctx = Context::get();
    ctx.ensure_scratch((size_t)nout * np + 16);
    double* partials = ctx.d_scratch;
    if (np == 0) IAMRX_HIP_CHECK(hipMemsetAsync(d_out, 0, nout * sizeof(double), ctx.stream));
    else if (op == 0) hipLaunchKernelGGL((k_reduce_finish<0>), dim3(nout), dim3(256), 0, ctx.stream, partials, np, d_out);
    else hipLaunchKernelGGL((k_reduce_finish<1>), dim3(nout), dim3(256), 0, ctx.stream, partials, np, d_out);
    if (global && ctx.comm->nranks > 1) ctx.comm->allreduce_device(d_out, nout, op == 0 ? ReduceOp::Sum : ReduceOp::Max, ctx.stream);
}

void reduce_finish_max(int nout, int np, bool global, double* out)
{
    auto& ctx = Context::get();
    if (np == 0 && !(global && ctx.comm->nranks > 1)) { for (int n = 0; n < nout; ++n) out[n] = 0.0; return; }
    finish_to_host(1, nout, np, global);
    for (int n = 0; n < nout; ++n) out[n] = ctx.h_scratch[n];
}

double reduce_norm0(const MultiFab& mf, int comp, int nc, int ng, bool global)
{
    global = global && !mf.layout->replicated;
    if (mf.nlocal() == 0) return (global && Context::get().comm->nranks > 1) ? finish_to_host(1, 1, 0, true) : 0.0;
    auto& ctx = Context::get();
    Tiling t = level_tiling(*mf.layout, mf.type, ng, 8, true);
    dim3 g = t.grid();
    const int np = (int)(g.x * g.y);
    ctx.ensure_scratch((size_t)np + 16);
    hipLaunchKernelGGL(k_norm0, g, Tiling::block(), 0, ctx.stream, t, mf.layout->d_boxes, mf.type.t[0], mf.type.t[1], mf.type.t[2], ng,
                       mf.d_tab, comp, nc, ctx.d_scratch);
    return finish_to_host(1, 1, np, global);
}

// largest and smallest value of one component in ONE pass and one read-back (partials: block maxima of v, then of -v); a NaN counts as
// +inf in both (mx = +inf, mn = -inf)
__global__ void __launch_bounds__(256) k_minmax(Tiling t, const BoxD* __restrict__ boxes, int t0, int t1, int t2, int ng,
                                                const FabD* __restrict__ tab, int comp, double* __restrict__ partials, int np)
{
    const int fab = tile_fab(t);
    const BoxD b = dev_grow_convert(boxes[fab], t0, t1, t2, ng);
    int i, j, k0, k1;
    const bool in = tile_ijk(t, b, i, j, k0, k1);
    const FabD a = tab[fab];
    double hi = -1.7976931348623157e308, lo = -1.7976931348623157e308;
    if (in)
        for (int k = k0; k <= k1; ++k) {
            const double v = a(i, j, k, comp), vh = v == v ? v : INFINITY, vl = v == v ? -v : INFINITY;
            hi = vh > hi ? vh : hi; lo = vl > lo ? vl : lo;
        }
    hi = block_reduce<1>(hi);
    lo = block_reduce<1>(lo);
    if (threadIdx.x == 0) {
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = hi;
        partials[(size_t)np + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = lo;
    }
}

// (a rank without data of the level contributes the identity -DBL_MAX to both: k_reduce_finish<2> over zero partials)
void reduce_minmax(const MultiFab& mf, int comp, int ng, double& mn, double& mx, bool global)
{
    global = global && !mf.layout->replicated;
    auto& ctx = Context::get();
    int np = 0;
    if (mf.nlocal() > 0) {
        Tiling t = level_tiling(*mf.layout, mf.type, ng, 8, true);
        dim3 g = t.grid();
        np = (int)(g.x * g.y);
        ctx.ensure_scratch((size_t)2 * np + 16);
        hipLaunchKernelGGL(k_minmax, g, Tiling::block(), 0, ctx.stream, t, mf.layout->d_boxes, mf.type.t[0], mf.type.t[1], mf.type.t[2], ng,
                           mf.d_tab, comp, ctx.d_scratch, np);
    }
    finish_to_host(2, 2, np, global);
    mx = ctx.h_scratch[0]; mn = -ctx.h_scratch[1];
}

// per-component maxima: partials[n * np + block]
__global__ void __launch_bounds__(256) k_norm0_comps(Tiling t, const BoxD* __restrict__ boxes, int t0, int t1, int t2, int ng,
                                                     const FabD* __restrict__ tab, int comp, int nc, double* __restrict__ partials, int np)
{
    const int fab = tile_fab(t);
    const BoxD b = dev_grow_convert(boxes[fab], t0, t1, t2, ng);
    int i, j, k0, k1;
    const bool in = tile_ijk(t, b, i, j, k0, k1);
    const FabD a = tab[fab];
    for (int n = 0; n < nc; ++n) {
        double m = 0.0;
        if (in) for (int k = k0; k <= k1; ++k) { const double v = norm_term(a(i, j, k, comp + n)); m = v > m ? v : m; }
        m = block_reduce<1>(m);
        if (threadIdx.x == 0) partials[(size_t)n * np + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
    }
}

void reduce_norm0_comps(const MultiFab& mf, int comp, int nc, int ng, double* out, bool global)
{
    global = global && !mf.layout->replicated;
    auto& ctx = Context::get();
    int np = 0;
    if (mf.nlocal() > 0) {
        Tiling t = level_tiling(*mf.layout, mf.type, ng, 8, true);
        dim3 g = t.grid();
        np = (int)(g.x * g.y);
        ctx.ensure_scratch((size_t)nc * np + 16);
        hipLaunchKernelGGL(k_norm0_comps, g, Tiling::block(), 0, ctx.stream, t, mf.layout->d_boxes, mf.type.t[0], mf.type.t[1], mf.type.t[2], ng,
                           mf.d_tab, comp, nc, ctx.d_scratch, np);
    } else if (!(global && ctx.comm->nranks > 1)) { for (int n = 0; n < nc; ++n) out[n] = 0.0; return; }
    finish_to_host(1, nc, np, global);
    for (int n = 0; n < nc; ++n) out[n] = ctx.h_scratch[n];
}

// owner mask for nodal / face data: a box owns index hi+1 in a nodal direction only on a
// non-periodic domain boundary (elsewhere that point is the low point of a neighbouring box or a
// periodic image)
struct OwnerInfo { int type[3]; int dlo[3]; int dhi[3]; int per[3]; int half_lo[3]; int half_hi[3]; };
// weight of a point in sums / dot products: 0 for non-owner copies, 1/2 per Neumann wall a NODE lies on (the nodal
// system is stored in doubled form at wall nodes: MLNodeLinOp dot mask), 1 otherwise.
// Ownership rule: the hi+1 point of a box in a nodal direction belongs to the neighbouring box (or periodic image) as its low point,
// unless it lies on a non-periodic domain face.  On a level that does not cover the domain the hi+1 points on coarse/fine faces have
// no such neighbour and get weight 0: every caller on such levels (NodalMG with its Dirichlet mask, the composite solver's `own`
// masks, amrns.hip) holds zero / excluded values exactly there, so the sums are unaffected; face-centred sums are only taken on
// levels that cover the domain.
__device__ __forceinline__ double owner_weight(const OwnerInfo& o, const BoxD& cellbox, int i, int j, int k)
{
    const int idx[3] = {i, j, k};
    double w = 1.0;
    for (int d = 0; d < 3; ++d) {
        if (!o.type[d]) continue;
        if (idx[d] == cellbox.hi[d] + 1 && (o.per[d] || idx[d] != o.dhi[d] + 1)) return 0.0;
        if (o.half_lo[d] && idx[d] == o.dlo[d]) w *= 0.5;
        if (o.half_hi[d] && idx[d] == o.dhi[d] + 1) w *= 0.5;
    }
    return w;
}
static OwnerInfo make_owner(const MultiFab& m, const Geometry& g)
{
    OwnerInfo own;
    for (int d = 0; d < 3; ++d) {
        own.type[d] = m.type.t[d]; own.dlo[d] = g.domain.lo[d]; own.dhi[d] = g.domain.hi[d]; own.per[d] = g.periodic[d];
        own.half_lo[d] = g.half_lo[d]; own.half_hi[d] = g.half_hi[d];
    }
    return own;
}

__global__ void __launch_bounds__(256) k_dots(Tiling t, const BoxD* __restrict__ boxes, OwnerInfo own, int nout,
                                              const FabD* x0, const FabD* y0, const FabD* x1, const FabD* y1,
                                              int comp, int nc, double* __restrict__ partials, int np)
{
    const int fab = tile_fab(t);
    const BoxD cb = boxes[fab];
    const BoxD b = dev_grow_convert(cb, own.type[0], own.type[1], own.type[2], 0);
    int i, j, k0, k1;
    double s0 = 0.0, s1 = 0.0;
    if (tile_ijk(t, b, i, j, k0, k1)) {
        const FabD a0 = x0[fab], b0 = y0[fab];
        for (int n = 0; n < nc; ++n)
            for (int k = k0; k <= k1; ++k)
                { const double w = owner_weight(own, cb, i, j, k); if (w != 0.0) s0 += w * (a0(i, j, k, comp + n) * b0(i, j, k, comp + n)); }
        if (nout > 1) {
            const FabD a1 = x1[fab], b1 = y1[fab];
            for (int n = 0; n < nc; ++n)
                for (int k = k0; k <= k1; ++k)
                    { const double w = owner_weight(own, cb, i, j, k); if (w != 0.0) s1 += w * (a1(i, j, k, comp + n) * b1(i, j, k, comp + n)); }
        }
    }
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    s0 = block_reduce<0>(s0);
    if (threadIdx.x == 0) partials[slot] = s0;
    if (nout > 1) {
        s1 = block_reduce<0>(s1);
        if (threadIdx.x == 0) partials[(size_t)np + slot] = s1;
    }
}

void reduce_dots(int nout, const MultiFab* const* x, const MultiFab* const* y, int comp, int nc, const Geometry& g, double* out, bool local)
{
    IAMRX_ASSERT(nout == 1 || nout == 2);
    auto& ctx = Context::get();
    const MultiFab& m = *x[0];
    for (int q = 0; q < nout; ++q) out[q] = 0.0;
    const bool global = !local && !m.layout->replicated && ctx.comm->nranks > 1;
    if (m.nlocal() == 0 && global) { finish_to_host(0, nout, 0, true); for (int q = 0; q < nout; ++q) out[q] = ctx.h_scratch[q]; }
    if (m.nlocal() > 0) {
        Tiling t = level_tiling(*m.layout, m.type, 0, 8, true);
        dim3 gr = t.grid();
        const int np = (int)(gr.x * gr.y);
        ctx.ensure_scratch((size_t)np * nout + 16);
        const OwnerInfo own = make_owner(m, g);
        hipLaunchKernelGGL(k_dots, gr, Tiling::block(), 0, ctx.stream, t, m.layout->d_boxes, own, nout,
                           x[0]->d_tab, y[0]->d_tab, nout > 1 ? x[1]->d_tab : nullptr, nout > 1 ? y[1]->d_tab : nullptr,
                           comp, nc, ctx.d_scratch, np);
        finish_to_host(0, nout, np, global);
        for (int q = 0; q < nout; ++q) out[q] = ctx.h_scratch[q];
    }
}

// dot products left on the device (see reduce_finish_dev)
void reduce_dots_dev(int nout, const MultiFab* const* x, const MultiFab* const* y, int comp, int nc, const Geometry& g, double* d_out, bool local)
{
    IAMRX_ASSERT(nout == 1 || nout == 2);
    auto& ctx = Context::get();
    const MultiFab& m = *x[0];
    const bool global = !local && !m.layout->replicated && ctx.comm->nranks > 1;
    int np = 0;
    if (m.nlocal() > 0) {
        Tiling t = level_tiling(*m.layout, m.type, 0, 8, true);
        dim3 gr = t.grid();
        np = (int)(gr.x * gr.y);
        ctx.ensure_scratch((size_t)np * nout + 16);
        const OwnerInfo own = make_owner(m, g);
        hipLaunchKernelGGL(k_dots, gr, Tiling::block(), 0, ctx.stream, t, m.layout->d_boxes, own, nout,
                           x[0]->d_tab, y[0]->d_tab, nout > 1 ? x[1]->d_tab : nullptr, nout > 1 ? y[1]->d_tab : nullptr,
                           comp, nc, ctx.d_scratch, np);
    }
    reduce_finish_dev(0, nout, np, global, d_out);
}

__global__ void __launch_bounds__(256) k_sum_unique(Tiling t, const BoxD* __restrict__ boxes, OwnerInfo own,
                                                    const FabD* __restrict__ tab, int comp, double* __restrict__ partials)
{
    const int fab = tile_fab(t);
    const BoxD cb = boxes[fab];
    const BoxD b = dev_grow_convert(cb, own.type[0], own.type[1], own.type[2], 0);
    int i, j, k0, k1;
    double s = 0.0;
    if (tile_ijk(t, b, i, j, k0, k1)) {
        const FabD a = tab[fab];
        for (int k = k0; k <= k1; ++k)
            { const double w = owner_weight(own, cb, i, j, k); if (w != 0.0) s += w * a(i, j, k, comp); }
    }
    s = block_reduce<0>(s);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

double reduce_sum_unique(const MultiFab& mf, int comp, const Geometry& g, bool global)
{
    global = global && !mf.layout->replicated;
    if (mf.nlocal() == 0) return (global && Context::get().comm->nranks > 1) ? finish_to_host(0, 1, 0, true) : 0.0;
    auto& ctx = Context::get();
    Tiling t = level_tiling(*mf.layout, mf.type, 0, 8, true);
    dim3 gr = t.grid();
    const int np = (int)(gr.x * gr.y);
    ctx.ensure_scratch((size_t)np + 16);
    const OwnerInfo own = make_owner(mf, g);
    hipLaunchKernelGGL(k_sum_unique, gr, Tiling::block(), 0, ctx.stream, t, mf.layout->d_boxes, own, mf.d_tab, comp, ctx.d_scratch);
    return finish_to_host(0, 1, np, global);
}

// NavierStokes::sum_integrated_quantities (NavierStokes.cpp:1046-1079): the three sums of one level in ONE pass over its state -- mass
// (volWgtSum "density"), tracer (volWgtSum "tracer") and kinetic energy (volWgtSum "energy" = derkeng, NS_derive.cpp:266-295) -- over the
// cells the finer level does not cover (MASK: cov != 0 there; such a cell is skipped, not multiplied by zero, so what it holds cannot
// reach the sums).  A NaN in a counted cell makes its sum NaN.  partials[q * np + block]; the caller applies the cell volume.
template <bool MASK>
__global__ void __launch_bounds__(256) k_sum_integrated(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ st, const FabD* __restrict__ cov,
                                                        int rho_comp, int trac_comp, double* __restrict__ partials, int np)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (tile_ijk(t, b, i, j, k0, k1)) {
        const FabD s = st[fab];
        for (int k = k0; k <= k1; ++k) {
            if (MASK && cov[fab](i, j, k) != 0.0) continue;
            const double u = s(i, j, k, 0), v = s(i, j, k, 1), w = s(i, j, k, 2), r = s(i, j, k, rho_comp), q = s(i, j, k, trac_comp);
            s0 += r; s1 += q; s2 += 0.5 * r * (u * u + v * v + w * w);
        }
    }
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    s0 = block_reduce<0>(s0);
    if (threadIdx.x == 0) partials[slot] = s0;
    s1 = block_reduce<0>(s1);
    if (threadIdx.x == 0) partials[(size_t)np + slot] = s1;
    s2 = block_reduce<0>(s2);
    if (threadIdx.x == 0) partials[2 * (size_t)np + slot] = s2;
}

// out[0..3) = sum rho, sum tracer, sum rho |u|^2 / 2 over the valid cells of THIS RANK's boxes (cov: cells with cov != 0 left out; null:
// none).  Two stages like every sum here (block partials in a fixed order, then one block over them): the same call gives the same bits.
void reduce_sum_integrated(const MultiFab& S, int rho_comp, int trac_comp, const MultiFab* cov, double out[3])
{
    IAMRX_ASSERT(S.type.cell() && (!cov || (cov->type.cell() && cov->layout->id == S.layout->id)));
    out[0] = out[1] = out[2] = 0.0;
    if (S.nlocal() == 0) return;
    auto& ctx = Context::get();
    Tiling t = level_tiling(*S.layout, S.type, 0, 8, true);
    dim3 g = t.grid();
    const int np = (int)(g.x * g.y);
    ctx.ensure_scratch((size_t)3 * np + 16);
    if (cov) hipLaunchKernelGGL((k_sum_integrated<true>), g, Tiling::block(), 0, ctx.stream, t, S.layout->d_boxes, S.d_tab, cov->d_tab, rho_comp, trac_comp, ctx.d_scratch, np);
    else hipLaunchKernelGGL((k_sum_integrated<false>), g, Tiling::block(), 0, ctx.stream, t, S.layout->d_boxes, S.d_tab, (const FabD*)nullptr, rho_comp, trac_comp, ctx.d_scratch, np);
    finish_to_host(0, 3, np, false);
    for (int q = 0; q < 3; ++q) out[q] = ctx.h_scratch[q];
}

// the same for named fields (NavierStokes::integrate): the sums of up to SUM_COMPS_MAX components of one array over the cells where cov
// is zero (skipped, not multiplied by zero), in the tiling and the order of k_sum_integrated.  partials[q * np + block]
struct SumComps { int n; int comp[SUM_COMPS_MAX]; };
template <bool MASK>
__global__ void __launch_bounds__(256) k_sum_comps(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ at, const FabD* __restrict__ cov, SumComps c,
                                                   double* __restrict__ partials, int np)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    double s[SUM_COMPS_MAX];
#pragma unroll
    for (int q = 0; q < SUM_COMPS_MAX; ++q) s[q] = 0.0;
    if (tile_ijk(t, b, i, j, k0, k1)) {
        const FabD a = at[fab];
        for (int k = k0; k <= k1; ++k) {
            if (MASK && cov[fab](i, j, k) != 0.0) continue;
#pragma unroll
            for (int q = 0; q < SUM_COMPS_MAX; ++q) if (q < c.n) s[q] += a(i, j, k, c.comp[q]);
        }
    }
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
#pragma unroll
    for (int q = 0; q < SUM_COMPS_MAX; ++q)
        if (q < c.n) {          // (uniform: every thread of the workgroup takes part in the reduction)
            const double v = block_reduce<0>(s[q]);
            if (threadIdx.x == 0) partials[(size_t)q * np + slot] = v;
        }
}

void reduce_sum_comps(const MultiFab& mf, int n, const int* comps, const MultiFab* cov, double* out)
{
    IAMRX_ASSERT(mf.type.cell() && (!cov || (cov->type.cell() && cov->layout->id == mf.layout->id)));
    for (int q = 0; q < n; ++q) { IAMRX_ASSERT(comps[q] >= 0 && comps[q] < mf.ncomp); out[q] = 0.0; }
    if (mf.nlocal() == 0) return;
    auto& ctx = Context::get();
    Tiling t = level_tiling(*mf.layout, mf.type, 0, 8, true);
    dim3 g = t.grid();
    const int np = (int)(g.x * g.y);
    for (int q0 = 0; q0 < n; q0 += SUM_COMPS_MAX) {
        SumComps c;
        c.n = std::min(SUM_COMPS_MAX, n - q0);
        for (int q = 0; q < SUM_COMPS_MAX; ++q) c.comp[q] = q < c.n ? comps[q0 + q] : 0;
        ctx.ensure_scratch((size_t)c.n * np + 16);
        if (cov) hipLaunchKernelGGL((k_sum_comps<true>), g, Tiling::block(), 0, ctx.stream, t, mf.layout->d_boxes, mf.d_tab, cov->d_tab, c, ctx.d_scratch, np);
        else hipLaunchKernelGGL((k_sum_comps<false>), g, Tiling::block(), 0, ctx.stream, t, mf.layout->d_boxes, mf.d_tab, (const FabD*)nullptr, c, ctx.d_scratch, np);
        finish_to_host(0, c.n, np, false);
        for (int q = 0; q < c.n; ++q) out[q0 + q] = ctx.h_scratch[q];
    }
}

// ------------------------------------------------------------------ BLAS-1 style
void mf_lincomb(MultiFab& dst, double a, const MultiFab& x, double b, const MultiFab& y, int comp, int nc, int ng)
{
    trace_blas_site("lincomb", dst.layout ? dst.layout->local_cells() * nc : 0);
    if (!dst.base) return;
    const FabD *dt = dst.d_tab, *xt = x.d_tab, *yt = y.d_tab;
    for_each_2ph(*dst.layout, dst.type, ng, nc, Context::get().stream,
        [=] __device__(int i, int j, int k, int f, int n) { return a * xt[f](i, j, k, comp + n) + b * yt[f](i, j, k, comp + n); },
        [=] __device__(int i, int j, int k, int f, int n, double v) { dt[f](i, j, k, comp + n) = v; });
}

void mf_saxpy(MultiFab& y, double a, const MultiFab& x, int xcomp, int ycomp, int nc, int ng)
{
    trace_blas_site("saxpy", y.layout ? y.layout->local_cells() * nc : 0);
    if (!y.base) return;
    const FabD *yt = y.d_tab, *xt = x.d_tab;
    for_each_2ph(*y.layout, y.type, ng, nc, Context::get().stream,
        [=] __device__(int i, int j, int k, int f, int n) { return yt[f](i, j, k, ycomp + n) + a * xt[f](i, j, k, xcomp + n); },
        [=] __device__(int i, int j, int k, int f, int n, double v) { yt[f](i, j, k, ycomp + n) = v; });
}

void mf_add_scalar(MultiFab& y, double a, int comp, int nc, int ng)
{
    if (!y.base) return;
    const FabD* yt = y.d_tab;
    for_each(*y.layout, y.type, ng, Context::get().stream, [=] __device__(int i, int j, int k, int f) {
        const FabD yy = yt[f];
        for (int n = 0; n < nc; ++n) yy(i, j, k, comp + n) += a;
    });
}

// y += a (mf_add_scalar's expression) and the max norm of the result (norm0's terms) in one pass
double mf_add_scalar_norm0(MultiFab& y, double a, int comp, int ng)
{
    const FabD* yt = y.d_tab;
    double out = 0.0;
    reduce_max_f<1>(*y.layout, y.type, ng, [=] __device__(int i, int j, int k, int f, double (&m)[1]) {
        double v = yt[f](i, j, k, comp);
        v += a;
        yt[f](i, j, k, comp) = v;
        const double t = norm_term(v);
        m[0] = t > m[0] ? t : m[0];
    }, &out);
    return out;
}

// rhs = S - div(umac) on the cells.  sum: also the sum of rhs over the level, formed as rhs.sum_unique(g, 0) forms it -- k_sum_unique's
// tiling, each thread's planes added in the same order (a cell's owner weight is 1), the same two reduction stages: the same bits --
// without the second read of the array
template <bool SUM>
__global__ void __launch_bounds__(256) k_mac_rhs(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ rt, const FabD* __restrict__ ut,
                                                 const FabD* __restrict__ vt, const FabD* __restrict__ wt, const FabD* __restrict__ st,
                                                 double dx, double dy, double dz, double* __restrict__ partials)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    double s = 0.0;
    if (tile_ijk(t, b, i, j, k0, k1)) {
        const FabD u = ut[fab], v = vt[fab], w = wt[fab], rr = rt[fab];
        for (int k = k0; k <= k1; ++k) {
            const double div = (u(i + 1, j, k) - u(i, j, k)) / dx + (v(i, j + 1, k) - v(i, j, k)) / dy + (w(i, j, k + 1) - w(i, j, k)) / dz;
            double r = -div;
            if (st) r += st[fab](i, j, k, 0);
            rr(i, j, k, 0) = r;
            if (SUM) s += r;
        }
    }
    if (SUM) {
        s = block_reduce<0>(s);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

void mac_rhs(const Geometry& g, MultiFab& rhs, const MultiFab* const umac[3], const MultiFab* S, double* sum)
{
    auto& ctx = Context::get();
    const bool global = !rhs.layout->replicated;
    if (rhs.nlocal() == 0) {
        if (sum) *sum = (global && ctx.comm->nranks > 1) ? finish_to_host(0, 1, 0, true) : 0.0;
        return;
    }
    Tiling t = level_tiling(*rhs.layout, cell_type(), 0, 8, true);
    dim3 gr = t.grid();
    const int np = (int)(gr.x * gr.y);
    const FabD* st = S ? S->d_tab : nullptr;
    if (!sum) {
        hipLaunchKernelGGL((k_mac_rhs<false>), gr, Tiling::block(), 0, ctx.stream, t, rhs.layout->d_boxes, rhs.d_tab, umac[0]->d_tab, umac[1]->d_tab,
                           umac[2]->d_tab, st, g.dx[0], g.dx[1], g.dx[2], (double*)nullptr);
        return;
    }
    ctx.ensure_scratch((size_t)np + 16);
    hipLaunchKernelGGL((k_mac_rhs<true>), gr, Tiling::block(), 0, ctx.stream, t, rhs.layout->d_boxes, rhs.d_tab, umac[0]->d_tab, umac[1]->d_tab,
                       umac[2]->d_tab, st, g.dx[0], g.dx[1], g.dx[2], ctx.d_scratch);
    *sum = finish_to_host(0, 1, np, global);
}

void mf_mult(MultiFab& y, double a, int comp, int nc, int ng)
{
    trace_blas_site("mult", y.layout ? y.layout->local_cells() * nc : 0);
    if (!y.base) return;
    const FabD* yt = y.d_tab;
    for_each_2ph(*y.layout, y.type, ng, nc, Context::get().stream,
        [=] __device__(int i, int j, int k, int f, int n) { return yt[f](i, j, k, comp + n) * a; },
        [=] __device__(int i, int j, int k, int f, int n, double v) { yt[f](i, j, k, comp + n) = v; });
}

// point idx of the ghost shell of box b (ng layers): per box two z-slabs (whole grown planes), two y-slabs (grown rows of the valid planes)
// and two x-slabs
__device__ __forceinline__ void shell_ijk(const BoxD& b, int ng, long idx, int& i, int& j, int& k)
{
    const long nx = b.len(0), ny = b.len(1), nz = b.len(2), gx = nx + 2 * ng, gy = ny + 2 * ng;
    const long nA = gx * gy * ng, nB = gx * ng * nz, nC = ng * ny * nz;
    long r = idx;
    if (r < 2 * nA) {
        const int side = (int)(r / nA); r -= side * nA;
        i = b.lo[0] - ng + (int)(r % gx); j = b.lo[1] - ng + (int)((r / gx) % gy);
        k = (side ? b.hi[2] + 1 : b.lo[2] - ng) + (int)(r / (gx * gy));
    } else if ((r -= 2 * nA) < 2 * nB) {
        const int side = (int)(r / nB); r -= side * nB;
        i = b.lo[0] - ng + (int)(r % gx); k = b.lo[2] + (int)(r / (gx * ng));
        j = (side ? b.hi[1] + 1 : b.lo[1] - ng) + (int)((r / gx) % ng);
    } else {
        r -= 2 * nB;
        const int side = (int)(r / nC); r -= side * nC;
        j = b.lo[1] + (int)((r / ng) % ny); k = b.lo[2] + (int)(r / (ng * ny));
        i = (side ? b.hi[0] + 1 : b.lo[0] - ng) + (int)(r % ng);
    }
}
__device__ __forceinline__ long shell_npts(const BoxD& b, int ng)
{
    const long nx = b.len(0), ny = b.len(1), nz = b.len(2), gx = nx + 2 * ng, gy = ny + 2 * ng;
    return 2 * (gx * gy * ng + gx * ng * nz + ng * ny * nz);
}

// y *= a on the ghost shell
__global__ void __launch_bounds__(256) k_mult_shell(const BoxD* __restrict__ boxes, const FabD* __restrict__ yt, int t0, int t1, int t2, int ng, int comp, int nc, double a)
{
    const int fab = blockIdx.y;
    BoxD b = boxes[fab];
    b.hi[0] += t0; b.hi[1] += t1; b.hi[2] += t2;
    const FabD y = yt[fab];
    const long total = shell_npts(b, ng);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int i, j, k;
        shell_ijk(b, ng, idx, i, j, k);
        for (int n = 0; n < nc; ++n) y(i, j, k, comp + n) = y(i, j, k, comp + n) * a;
    }
}

// h = 0.5 * (a + b) on the ghost shell (cell-centred, component 0)
__global__ void __launch_bounds__(256) k_half_sum_shell(const BoxD* __restrict__ boxes, const FabD* __restrict__ ht, const FabD* __restrict__ at,
                                                        const FabD* __restrict__ bt, int ng)
{
    const int fab = blockIdx.y;
    const BoxD b = boxes[fab];
    const FabD h = ht[fab], pa = at[fab], pb = bt[fab];
    const long total = shell_npts(b, ng);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        int i, j, k;
        shell_ijk(b, ng, idx, i, j, k);
        h(i, j, k, 0) = 0.5 * (pa(i, j, k, 0) + pb(i, j, k, 0));
    }
}

static unsigned shell_blocks(const Layout& l, const IndexType& type, int ng)
{
    const long nx = l.max_len[0] + type.t[0], ny = l.max_len[1] + type.t[1], nz = l.max_len[2] + type.t[2];
    const long total = 2 * ((nx + 2 * ng) * (ny + 2 * ng) * ng + (nx + 2 * ng) * ng * nz + ng * ny * nz);
    return (unsigned)std::min<long>((total + 255) / 256, 4096);
}

void mf_half_sum_ghosts(MultiFab& h, const MultiFab& a, const MultiFab& b, int ng)
{
    if (ng <= 0 || h.nlocal() == 0) return;
    IAMRX_ASSERT(ng <= h.ngrow && ng <= a.ngrow && ng <= b.ngrow && a.layout.get() == h.layout.get() && b.layout.get() == h.layout.get());
    const Layout& l = *h.layout;
    hipLaunchKernelGGL(k_half_sum_shell, dim3(shell_blocks(l, h.type, ng), (unsigned)l.nlocal()), dim3(256), 0, Context::get().stream, l.d_boxes, h.d_tab,
                       a.d_tab, b.d_tab, ng);
}

void mf_mult_ghosts(MultiFab& y, double a, int comp, int nc, int ng)
{
    if (!y.base || ng <= 0 || y.nlocal() == 0) return;
    IAMRX_ASSERT(ng <= y.ngrow);
    const Layout& l = *y.layout;
    hipLaunchKernelGGL(k_mult_shell, dim3(shell_blocks(l, y.type, ng), (unsigned)l.nlocal()), dim3(256), 0, Context::get().stream, l.d_boxes, y.d_tab, y.type.t[0], y.type.t[1],
                       y.type.t[2], ng, comp, nc, a);
}

// ---------------------------------------------------------------------------------------------------------------- dense image
constexpr int DENSE_THREADS = 256;

// grid (chunks, local boxes): cell p of the box -> dst[dense index] = f (MODE 0), dst[2 * dense index] = (f, 0) (MODE 1), or the
// imaginary part dst[2 * dense index + 1] = f alone (MODE 2: the second field of a packed pair, k_spectrum.hip)
template <int MODE>
__global__ void __launch_bounds__(DENSE_THREADS) k_dense_pack(const BoxD* __restrict__ boxes, const FabD* __restrict__ st, int comp, BoxD dom,
                                                              double* __restrict__ dst)
{
    const BoxD b = boxes[blockIdx.y];
    const FabD s = st[blockIdx.y];
    const auto sp = s.gp() + (long)comp * s.cs;
    const int bx = b.len(0), by = b.len(1);
    const long np = b.npts(), nx = dom.len(0), ny = dom.len(1);
    for (long p = (long)blockIdx.x * DENSE_THREADS + threadIdx.x; p < np; p += (long)gridDim.x * DENSE_THREADS) {
        const int i = (int)(p % bx);
        const long r = p / bx;
        const int j = (int)(r % by), k = (int)(r / by);
        const double v = sp[s.off(b.lo[0] + i, b.lo[1] + j, b.lo[2] + k)];
        const long o = (long)(b.lo[0] - dom.lo[0] + i) + nx * ((long)(b.lo[1] - dom.lo[1] + j) + ny * (long)(b.lo[2] - dom.lo[2] + k));
        if (MODE == 1) { dst[2 * o] = v; dst[2 * o + 1] = 0.0; }
        else if (MODE == 2) dst[2 * o + 1] = v;
        else dst[o] = v;
    }
}

void dense_check_cover(const char* who, const Geometry& g, const Layout& lay)
{
    long cells = 0;
    for (const BoxD& b : lay.boxes) {
        for (int d = 0; d < 3; ++d)
            if (b.lo[d] < g.domain.lo[d] || b.hi[d] > g.domain.hi[d]) throw Error(std::string(who) + ": a box of the level reaches outside the domain");
        cells += b.npts();
    }
    if (cells != g.domain.npts())
        throw Error(std::string(who) + ": the boxes of the level do not cover the domain (" + std::to_string(cells) + " of " + std::to_string(g.domain.npts()) + " cells)");
}

static void dense_pack_mode(const Geometry& g, const MultiFab& S, int comp, double* dst, int mode)
{
    const Layout& lay = *S.layout;
    if (lay.nlocal() == 0) return;
    long big = 1;
    for (int f = 0; f < lay.nlocal(); ++f) big = std::max(big, lay.lbox(f).npts());
    const dim3 grid((unsigned)std::min<long>((big + 4 * DENSE_THREADS - 1) / (4 * DENSE_THREADS), 65535), (unsigned)lay.nlocal());
    hipStream_t s = Context::get().stream;
    if (mode == 1) hipLaunchKernelGGL((k_dense_pack<1>), grid, dim3(DENSE_THREADS), 0, s, lay.d_boxes, S.d_tab, comp, g.domain, dst);
    else if (mode == 2) hipLaunchKernelGGL((k_dense_pack<2>), grid, dim3(DENSE_THREADS), 0, s, lay.d_boxes, S.d_tab, comp, g.domain, dst);
    else hipLaunchKernelGGL((k_dense_pack<0>), grid, dim3(DENSE_THREADS), 0, s, lay.d_boxes, S.d_tab, comp, g.domain, dst);
}

void dense_pack(const Geometry& g, const MultiFab& S, int comp, double* dst, bool cplx) { dense_pack_mode(g, S, comp, dst, cplx ? 1 : 0); }
void dense_pack_imag(const Geometry& g, const MultiFab& S, int comp, double* dst) { dense_pack_mode(g, S, comp, dst, 2); }

// grid (chunks, local boxes): the inverse of k_dense_pack<1>, cell p of the box <- scale * src[2 * dense index] (the real part)
__global__ void __launch_bounds__(DENSE_THREADS) k_dense_unpack(const BoxD* __restrict__ boxes, const FabD* __restrict__ dt, int comp, BoxD dom,
                                                                const double* __restrict__ src, double scale)
{
    const BoxD b = boxes[blockIdx.y];
    const FabD d = dt[blockIdx.y];
    const auto dp = d.gp() + (long)comp * d.cs;
    const int bx = b.len(0), by = b.len(1);
    const long np = b.npts(), nx = dom.len(0), ny = dom.len(1);
    for (long p = (long)blockIdx.x * DENSE_THREADS + threadIdx.x; p < np; p += (long)gridDim.x * DENSE_THREADS) {
        const int i = (int)(p % bx);
        const long r = p / bx;
        const int j = (int)(r % by), k = (int)(r / by);
        const long o = (long)(b.lo[0] - dom.lo[0] + i) + nx * ((long)(b.lo[1] - dom.lo[1] + j) + ny * (long)(b.lo[2] - dom.lo[2] + k));
        dp[d.off(b.lo[0] + i, b.lo[1] + j, b.lo[2] + k)] = src[2 * o] * scale;
    }
}

void dense_unpack(const Geometry& g, MultiFab& S, int comp, const double* src, double scale)
{
    const Layout& lay = *S.layout;
    if (lay.nlocal() == 0) return;
    long big = 1;
    for (int f = 0; f < lay.nlocal(); ++f) big = std::max(big, lay.lbox(f).npts());
    const dim3 grid((unsigned)std::min<long>((big + 4 * DENSE_THREADS - 1) / (4 * DENSE_THREADS), 65535), (unsigned)lay.nlocal());
    hipLaunchKernelGGL(k_dense_unpack, grid, dim3(DENSE_THREADS), 0, Context::get().stream, lay.d_boxes, S.d_tab, comp, g.domain, src, scale);
}

bool dense_needs_gather(const MultiFab& S)
{
    auto& ctx = Context::get();
    return (ctx.comm ? ctx.comm->nranks : 1) > 1 && !S.layout->replicated;
}

void dense_gather(const Geometry& g, const MultiFab& S, int comp, double* R)
{
    auto& ctx = Context::get();
    if (!dense_needs_gather(S)) { dense_pack(g, S, comp, R, false); return; }
    const long N = g.domain.npts();
    IAMRX_HIP_CHECK(hipMemsetAsync(R, 0, (size_t)N * sizeof(double), ctx.stream));
    dense_pack(g, S, comp, R, false);
    ctx.comm->allreduce_device(R, (int)N, ReduceOp::Sum, ctx.stream);
}

// slab levels (mf.h): every y-plane of dst takes the single y-plane of src
void slab_duplicate(MultiFab& dst, const MultiFab& src)
{
    IAMRX_ASSERT(dst.ncomp == src.ncomp && dst.layout->boxes.size() == src.layout->boxes.size());
    if (dst.nlocal() == 0) return;
    const FabD *dt = dst.d_tab, *st = src.d_tab;
    const int nc = dst.ncomp;
    for_each(*dst.layout, dst.type, 0, Context::get().stream, [=] __device__(int i, int j, int k, int f) {
        const FabD s = st[f];
        for (int n = 0; n < nc; ++n) dt[f](i, j, k, n) = s(i, 0, k, n);        // (slab boxes start at y = 0: Layout::slab_coarsenable)
    });
}

}  // namespace iamrx
