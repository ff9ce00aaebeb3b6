// iamr_amd/csrc/k_sgs.hip -- a-priori LES analysis on a triply periodic level: the subgrid stress of a filtered field, the inter-scale
// flux and what the Smagorinsky operators make of the same filtered field (this library's own diagnostic; definitions and summation
// orders: include/iamrx.h, iamrx_mf_sgs).  The driver sgs_compute sits beside specop_filter (k_spectrum.hip) and runs the filter's own
// passes on nine dense complex images -- u_i (the plain pack) and u_i u_j, i <= j -- which stay on the device; this file holds
//   k_sgs_pack      the valid cells of u_i * u_j of every local box -> their place in the dense image, (value, 0) or the value alone (the
//                   real array several ranks sum): k_dense_pack with one more read and one product, formed in double, rounded once
//   k_sgs_point     one launch over the dense index space, x fastest.  A cell reads the real parts of the six filtered products at its own
//                   index and of the three filtered velocities at its six face neighbours (the wrap is a mask: every extent is a power of
//                   two), forms tau, A, S, Pi, D_0, D_1, stores the requested fields and accumulates the 16 sums and the count of Pi < 0.
//                   Plain reads through the caches: the x neighbours lie in the wavefront's own lines and the y / z neighbours in lines
//                   that the neighbouring rows of the same or the next workgroup have just fetched (DESIGN.md has the measurement against
//                   the three-plane LDS ring of k_velgrad.hip on the same stencil).
//                   Fields go into the product images, which nobody else reads: tau_ij over the real part of image ij, fields 6 .. 9 into
//                   the imaginary parts of images 0 .. 3 (dense_unpack takes either through the pointer it is given).
//   k_sgs_finish    one wavefront per statistic adds the slots in slot order and divides once by N
// Sums: per thread in index order (a grid-stride loop over a grid that depends on N alone), across the wavefront by a butterfly in which
// both partners add the same two numbers in the same order, the four wavefronts of a workgroup in order into the workgroup's own 16
// slots.  No floating-point atomics: the same call gives the same bits for every box layout and number of ranks.  The count of Pi < 0
// is an integer and takes an integer atomic per wavefront.
#include "kernels.h"
#include "launch.h"
#include "les_model.h"
#include <algorithm>

namespace iamrx {

namespace {

constexpr int SGS_THREADS = 256;

// grid (chunks, local boxes), as k_dense_pack
template <bool CPLX>
__global__ void __launch_bounds__(SGS_THREADS) k_sgs_pack(const BoxD* __restrict__ boxes, const FabD* __restrict__ st, int ci, int cj, BoxD dom,
                                                          double* __restrict__ dst)
{
    const BoxD b = boxes[blockIdx.y];
    const FabD s = st[blockIdx.y];
    const auto si = s.gp() + (long)ci * s.cs;
    const auto sj = s.gp() + (long)cj * s.cs;
    const int bx = b.len(0), by = b.len(1);
    const long np = b.npts(), nx = dom.len(0), ny = dom.len(1);
    for (long p = (long)blockIdx.x * SGS_THREADS + threadIdx.x; p < np; p += (long)gridDim.x * SGS_THREADS) {
        const int i = (int)(p % bx);
        const long r = p / bx;
        const int j = (int)(r % by), k = (int)(r / by);
        const long c = s.off(b.lo[0] + i, b.lo[1] + j, b.lo[2] + k);
        const double v = si[c] * sj[c];
        const long o = (long)(b.lo[0] - dom.lo[0] + i) + nx * ((long)(b.lo[1] - dom.lo[1] + j) + ny * (long)(b.lo[2] - dom.lo[2] + k));
        if (CPLX) { dst[2 * o] = v; dst[2 * o + 1] = 0.0; }
        else dst[o] = v;
    }
}

// the sum over the wavefront, the same bits in every lane
__device__ __forceinline__ double sgs_wave_sum(double v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = (threadIdx.x & off) ? o + v : v + o;              // both partners add the same two numbers in the same order
    }
    return v;
}

template <bool FIELDS>
__global__ void __launch_bounds__(SGS_THREADS) k_sgs_point(SgsPoint a, double* __restrict__ slots, unsigned long long* __restrict__ neg)
{
    __shared__ double part[SGS_THREADS / 64][SGS_NSTAT];
    const int nx = 1 << a.ln[0], ny = 1 << a.ln[1], nz = 1 << a.ln[2];
    const int lxy = a.ln[0] + a.ln[1];
    const long N = (long)1 << (lxy + a.ln[2]);
    double acc[SGS_NSTAT];
#pragma unroll
    for (int q = 0; q < SGS_NSTAT; ++q) acc[q] = 0.0;
    unsigned cnt = 0;
    // XCD-aware order (see make_tiling): consecutive workgroups go to the eight XCDs in turn, so each XCD takes a run of gridDim.x / 8
    // consecutive 256-cell pieces and finds the y neighbours of its rows in its own L2
    const int wg = (gridDim.x & 7) == 0 ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
    for (long p = (long)wg * SGS_THREADS + threadIdx.x; p < N; p += (long)gridDim.x * SGS_THREADS) {
        const int i = (int)(p & (nx - 1)), j = (int)((p >> a.ln[0]) & (ny - 1)), k = (int)(p >> lxy);
        const long row = p - i, col = p - ((long)j << a.ln[0]), pln = p - ((long)k << lxy);
        const long xm = row + ((i - 1) & (nx - 1)), xp = row + ((i + 1) & (nx - 1));
        const long ym = col + ((long)((j - 1) & (ny - 1)) << a.ln[0]), yp = col + ((long)((j + 1) & (ny - 1)) << a.ln[0]);
        const long zm = pln + ((long)((k - 1) & (nz - 1)) << lxy), zp = pln + ((long)((k + 1) & (nz - 1)) << lxy);
        double A[9], u[3];
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            const double2* __restrict__ U = a.U[n];
            u[n] = U[p].x;
            A[3 * n + 0] = 0.5 * (U[xp].x - U[xm].x) * a.dxi[0];
            A[3 * n + 1] = 0.5 * (U[yp].x - U[ym].x) * a.dxi[1];
            A[3 * n + 2] = 0.5 * (U[zp].x - U[zm].x) * a.dxi[2];
        }
        // tau_ij = (u_i u_j)~ - u~_i u~_j in the order xx xy xz yy yz zz
        const double txx = a.P[0][p].x - u[0] * u[0], txy = a.P[1][p].x - u[0] * u[1], txz = a.P[2][p].x - u[0] * u[2];
        const double tyy = a.P[3][p].x - u[1] * u[1], tyz = a.P[4][p].x - u[1] * u[2], tzz = a.P[5][p].x - u[2] * u[2];
        const double ksgs = 0.5 * ((txx + tyy) + tzz);
        // s_ij = A_ij + A_ji = 2 S_ij; SS as k_velgrad.hip forms it
        const double s01 = A[1] + A[3], s02 = A[2] + A[6], s12 = A[5] + A[7];
        const double ss = A[0] * A[0] + A[4] * A[4] + A[8] * A[8] + 0.5 * (s01 * s01 + s02 * s02 + s12 * s12);
        const double ss2 = 2 * ss;
        const double smag = sqrt(ss2);
        const double offd = (txy * s01 + txz * s02) + tyz * s12;
        const double pi = -(((txx * A[0] + tyy * A[4]) + tzz * A[8]) + offd);
        const double iso = (2.0 / 3.0) * ksgs;
        const double dxx = txx - iso, dyy = tyy - iso, dzz = tzz - iso;
        const double tdtd = ((dxx * dxx + dyy * dyy) + dzz * dzz) + 2 * ((txy * txy + txz * txz) + tyz * tyz);
        const double tds = ((dxx * A[0] + dyy * A[4]) + dzz * A[8]) + offd;
        const double D0 = a.delta2 * smag;
        const double D1 = les_model<0>(A, a.delta2);
        const double P0 = D0 * ss2, P1 = D1 * ss2;
        if (FIELDS) {
            const int m = a.mask;
            if (m & 1) ((double*)a.P[0])[2 * p] = txx;
            if (m & 2) ((double*)a.P[1])[2 * p] = txy;
            if (m & 4) ((double*)a.P[2])[2 * p] = txz;
            if (m & 8) ((double*)a.P[3])[2 * p] = tyy;
            if (m & 16) ((double*)a.P[4])[2 * p] = tyz;
            if (m & 32) ((double*)a.P[5])[2 * p] = tzz;
            if (m & 64) ((double*)a.P[0])[2 * p + 1] = ksgs;
            if (m & 128) ((double*)a.P[1])[2 * p + 1] = pi;
            if (m & 256) ((double*)a.P[2])[2 * p + 1] = smag;
            if (m & 512) ((double*)a.P[3])[2 * p + 1] = P0;
        }
        acc[0] += pi;
        acc[1] += pi * pi;
        acc[2] += fmin(pi, 0.0);
        acc[3] += ksgs;
        acc[4] += ss2;
        acc[5] += tdtd;
        acc[6] += P0;
        acc[7] += P0 * P0;
        acc[8] += pi * P0;
        acc[9] += (D0 * D0) * ss2;
        acc[10] += D0 * tds;
        acc[11] += P1;
        acc[12] += P1 * P1;
        acc[13] += pi * P1;
        acc[14] += (D1 * D1) * ss2;
        acc[15] += D1 * tds;
        cnt += pi < 0.0 ? 1u : 0u;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < SGS_NSTAT; ++q) {
        const double v = sgs_wave_sum(acc[q]);
        if (lane == 0) part[wave][q] = v;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0 && cnt != 0) atomicAdd(neg, (unsigned long long)cnt);
    __syncthreads();
    if (threadIdx.x < SGS_NSTAT) {
        const int q = threadIdx.x;
        slots[(long)wg * SGS_NSTAT + q] =((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
    }
}

// one wavefront per statistic: lane l adds the slots l, l + 64, ... in order, the lanes combine in a fixed tree, one division by N;
// stats[SGS_NSTAT] takes the bits of the count
__global__ void __launch_bounds__(SGS_THREADS) k_sgs_finish(const double* __restrict__ slots, int nwg, double N, const unsigned long long* __restrict__ neg,
                                                            double* __restrict__ stats)
{
    const int q = blockIdx.x * (SGS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= SGS_NSTAT) return;
    double v = 0.0;
    for (int g = lane; g < nwg; g += 64) v += slots[(long)g * SGS_NSTAT + q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) {
        stats[q] = v / N;
        if (q == 0) stats[SGS_NSTAT] = __longlong_as_double((long long)*neg);
    }
}

}  // namespace

void sgs_pack_product(const Geometry& g, const MultiFab& S, int ci, int cj, double* dst, bool cplx)
{
    const Layout& lay = *S.layout;
    if (lay.nlocal() == 0) return;
    long big = 1;
    for (int f = 0; f < lay.nlocal(); ++f) big = std::max(big, lay.lbox(f).npts());
    const dim3 grid((unsigned)std::min<long>((big + 4 * SGS_THREADS - 1) / (4 * SGS_THREADS), 65535), (unsigned)lay.nlocal());
    hipStream_t s = Context::get().stream;
    if (cplx) hipLaunchKernelGGL((k_sgs_pack<true>), grid, dim3(SGS_THREADS), 0, s, lay.d_boxes, S.d_tab, ci, cj, g.domain, dst);
    else hipLaunchKernelGGL((k_sgs_pack<false>), grid, dim3(SGS_THREADS), 0, s, lay.d_boxes, S.d_tab, ci, cj, g.domain, dst);
}

int sgs_nwg(long N) { return (int)std::min<long>((N + SGS_THREADS - 1) / SGS_THREADS, SGS_MAXWG); }

void sgs_point(const SgsPoint& a, double* slots, unsigned long long* neg, double* stats)
{
    auto& ctx = Context::get();
    const long N = (long)1 << (a.ln[0] + a.ln[1] + a.ln[2]);
    const int nwg = sgs_nwg(N);
    IAMRX_HIP_CHECK(hipMemsetAsync(neg, 0, sizeof(unsigned long long), ctx.stream));
    if (a.mask) hipLaunchKernelGGL((k_sgs_point<true>), dim3((unsigned)nwg), dim3(SGS_THREADS), 0, ctx.stream, a, slots, neg);
    else hipLaunchKernelGGL((k_sgs_point<false>), dim3((unsigned)nwg), dim3(SGS_THREADS), 0, ctx.stream, a, slots, neg);
    hipLaunchKernelGGL(k_sgs_finish, dim3((unsigned)((SGS_NSTAT + 3) / 4)), dim3(SGS_THREADS), 0, ctx.stream, slots, nwg, (double)N, neg, stats);
}

}  // namespace iamrx
