// iamr_amd/csrc/k_strfn.hip -- structure functions and two-point correlations of cell-centred fields along the axes (this library's
// own diagnostic, beside the spectra of k_spectrum.hip; a turbulence user otherwise post-processes plotfiles for them).
//
// Definition (include/iamrx.h): for an axis d and a separation of r cells, delta = f(x + r e_d) - f(x) over the pairs of the axis
// (periodic: all N cells with wrap-around; otherwise the pairs inside the domain), every column divided by the number of pairs:
//   column 0 = <f(x) f(x + r e_d)>, columns 1 .. pmax = <delta^p>, then <|delta|^p> for the odd p <= pmax.
//
// One component at a time through one dense real array R (8 B per cell, x fastest) from the arena:
//   dense_gather       (k_basic.hip, shared with the spectra) valid cells of every local box -> R; the only step that sees boxes or ranks
//   k_strfn_pairs<PM, PER>  one launch per axis.  A workgroup takes tiles of TW pencils: along x TW whole contiguous pencils, along y
//                      and z TW adjacent x columns times the whole pencil, so that every global load runs along x.  LDS image:
//                      element of the pencil major, pencil minor (stride TW; TW + 1 along x, where the store into the image runs
//                      along the pencil); on a periodic axis the first rmax elements follow once more behind the last, so that the
//                      partner of x is x + r with no wrap in the loop.  Thread (t, g) = (tid % TW, tid / TW) walks pencil t for the
//                      separations r = g, g + G, ... (G = 256 / TW), four of them at a time (then two, then one): f(x) is read once for
//                      the four, the partners come from LDS at lane-contiguous addresses, powers by successive multiplication, all
//                      sums in registers.  The TW pencils of a group combine by a fixed butterfly of wave shuffles; lane t = 0 adds
//                      the result to the workgroup's own slots in global memory (first tile: stores), tile after tile in order.
//   k_strfn_sum        per-workgroup sums of R for the mean
//   k_strfn_finish     one wavefront per output: adds the slots in slot order, then the one division by the exact count
// No floating-point atomics: every sum has a fixed order -- along a pencil, across the pencils of a group, across the tiles of a
// workgroup, across workgroups -- so the same call gives the same bits, whatever the boxes and ranks.  PM is pmax rounded up to 2, 4
// or 8 (the registers of a thread are sized at compile time); a column's bits do not depend on PM.
#include "kernels.h"
#include "launch.h"
#include <algorithm>
#include <string>
#include <vector>

namespace iamrx {

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_MAXWG = 1024;          // workgroups (= slots per output) of a pair launch
constexpr int SF_SUMWG = 256;           // workgroups of k_strfn_sum
constexpr int SF_TILE_ELEMS = 6144;     // elements of the LDS image without the x padding: 48 KiB, three workgroups per CU

struct StrfnPass {
    int n;              // cells along the axis
    int rmax;           // separations 0 .. rmax
    int len;            // elements of the LDS image of a pencil: n, on a periodic axis n + rmax
    int ltw;            // log2 of TW
    int ts;             // LDS stride between two elements of a pencil
    int x;              // the axis is x
    int ncolumns;       // pencils across a row of tiles: n_y n_z (x) or n_x (y, z)
    int ntile_row;      // tiles across them
    int ntiles;         // all tiles
    long estride, ostride;      // y, z: distance of two elements of a pencil, of two rows of tiles
};

// the columns a thread carries for one separation
template <int PM>
struct SfAcc {
    static constexpr int NA = (PM + 1) / 2, NC = 1 + PM + NA;
    double R, S[PM], A[NA];
    __device__ __forceinline__ void zero()
    {
        R = 0.0;
#pragma unroll
        for (int p = 0; p < PM; ++p) S[p] = 0.0;
#pragma unroll
        for (int p = 0; p < NA; ++p) A[p] = 0.0;
    }
    __device__ __forceinline__ void add(double fa, double fb)
    {
        const double d = fb - fa;
        R += fa * fb;
        double w = d;
#pragma unroll
        for (int p = 0; p < PM; ++p) {
            if (p > 0) w *= d;
            S[p] += w;
            if ((p & 1) == 0) A[p >> 1] += fabs(w);        // |delta|^p = |delta^p| to the bit: rounding is symmetric in the sign
        }
    }
    __device__ __forceinline__ double& col(int c) { return c == 0 ? R : (c <= PM ? S[c - 1] : A[c - 1 - PM]); }
};

// RS separations r0, r0 + G, ... of pencil t over the whole pencil.  A separation beyond rmax repeats r0 and is not written.
template <int PM, bool PER, int RS>
__device__ __forceinline__ void sf_batch(const double* __restrict__ s, const StrfnPass& ps, int t, int r0, int G, bool first, double* __restrict__ slot)
{
    SfAcc<PM> acc[RS];
    int rj[RS];
#pragma unroll
    for (int j = 0; j < RS; ++j) { acc[j].zero(); rj[j] = r0 + j * G <= ps.rmax ? r0 + j * G : r0; }
    if (r0 <= ps.rmax) {
        const double* pa = s + t;
        // every partner inside the image: all x on a periodic axis (the image carries the wrap), x < n - (largest separation) otherwise
        int rl = r0;
#pragma unroll
        for (int j = 0; j < RS; ++j) rl = max(rl, rj[j]);
        const int xfull = PER ? ps.n : ps.n - rl;
        int x = 0;
#pragma unroll 2
        for (; x < xfull; ++x) {
            const double fa = pa[x * ps.ts];
#pragma unroll
            for (int j = 0; j < RS; ++j) acc[j].add(fa, pa[(x + rj[j]) * ps.ts]);
        }
        if (!PER) {
            // the last pairs of the shorter separations
            for (; x < ps.n - r0; ++x) {
                const double fa = pa[x * ps.ts];
#pragma unroll
                for (int j = 0; j < RS; ++j)
                    if (x + rj[j] < ps.n) acc[j].add(fa, pa[(x + rj[j]) * ps.ts]);
            }
        }
    }
    // across the TW pencils of the group: a butterfly, the same tree in every lane (the loop is uniform over the workgroup)
    const int tw_ = 1 << ps.ltw;
#pragma unroll
    for (int j = 0; j < RS; ++j) {
#pragma unroll
        for (int c = 0; c < SfAcc<PM>::NC; ++c) {
            double v = acc[j].col(c);
            for (int off = 1; off < tw_; off <<= 1) {
                const double o = __shfl_xor(v, off, 64);
                v = (t & off) ? o + v : v + o;              // both partners add the same two numbers in the same order
            }
            acc[j].col(c) = v;
        }
    }
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < RS; ++j) {
            const int r = r0 + j * G;
            if (r <= ps.rmax) {
                double* q = slot + (long)r * SfAcc<PM>::NC;
#pragma unroll
                for (int c = 0; c < SfAcc<PM>::NC; ++c) q[c] = first ? acc[j].col(c) : q[c] + acc[j].col(c);
            }
        }
    }
}

// slots[(wg * (rmax + 1) + r) * NC + c]: the sums of workgroup wg over its tiles wg, wg + gridDim.x, ...
template <int PM, bool PER>
__global__ void __launch_bounds__(SF_THREADS) k_strfn_pairs(const double* __restrict__ R, StrfnPass ps, double* __restrict__ slots)
{
    extern __shared__ double sf_lds[];
    double* s = sf_lds;
    const int tid = threadIdx.x, tw_ = 1 << ps.ltw, G = SF_THREADS >> ps.ltw;
    const int t = tid & (tw_ - 1), g = tid >> ps.ltw;
    const int gwave = (tid & ~63) >> ps.ltw;                 // the smallest group of this wavefront
    double* slot = slots + (long)blockIdx.x * (ps.rmax + 1) * SfAcc<PM>::NC;
    bool first = true;
    for (int tile = blockIdx.x; tile < ps.ntiles; tile += gridDim.x, first = false) {
        if (!first) __syncthreads();                         // the image of the previous tile has been read
        const int tr = tile % ps.ntile_row, to = tile / ps.ntile_row;
        const int c0 = tr * tw_;                             // first pencil of the tile
        if (ps.x) {
            const int total = ps.n << ps.ltw;
            for (int q = tid; q < total; q += SF_THREADS) {
                const int e = q % ps.n, p = q / ps.n;
                s[e * ps.ts + p] = c0 + p < ps.ncolumns ? R[(long)(c0 + p) * ps.n + e] : 0.0;
            }
        } else {
            const int total = ps.n << ps.ltw;
            const long base = (long)to * ps.ostride + c0;
            for (int q = tid; q < total; q += SF_THREADS) {
                const int p = q & (tw_ - 1), e = q >> ps.ltw;
                s[e * ps.ts + p] = c0 + p < ps.ncolumns ? R[base + p + (long)e * ps.estride] : 0.0;
            }
        }
        __syncthreads();
        if (PER) {
            // the wrap: elements n .. n + rmax - 1 of the image repeat 0 .. rmax - 1 (rmax <= n / 2: they are disjoint)
            const int total = ps.rmax << ps.ltw;
            for (int q = tid; q < total; q += SF_THREADS) {
                const int p = q & (tw_ - 1), e = q >> ps.ltw;
                s[(ps.n + e) * ps.ts + p] = s[e * ps.ts + p];
            }
            __syncthreads();
        }
        // the separations in rounds of 4 G, 2 G or G, the same rounds for every thread of the workgroup
        for (int rb = 0; rb <= ps.rmax;) {
            const int rem = ps.rmax - rb + 1;
            const bool mine = rb + gwave <= ps.rmax;         // uniform over the wavefront: one without a separation in the round skips it
            if (rem >= 4 * G) { if (mine) sf_batch<PM, PER, 4>(s, ps, t, rb + g, G, first, slot); rb += 4 * G; }
            else if (rem >= 2 * G) { if (mine) sf_batch<PM, PER, 2>(s, ps, t, rb + g, G, first, slot); rb += 2 * G; }
            else { if (mine) sf_batch<PM, PER, 1>(s, ps, t, rb + g, G, first, slot); rb += G; }
        }
    }
}

// slots[wg] = the sum of this workgroup's share of R: thread by thread in index order, a fixed tree over the lanes, the wavefronts in order
__global__ void __launch_bounds__(SF_THREADS) k_strfn_sum(const double* __restrict__ R, long N, double* __restrict__ slots)
{
    __shared__ double part[4];
    double v = 0.0;
    for (long p = (long)blockIdx.x * SF_THREADS + threadIdx.x; p < N; p += (long)gridDim.x * SF_THREADS) v += R[p];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) slots[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

struct StrfnFinish {
    int nwg, nr, nck;           // workgroups, separations and columns per separation of the slots
    int pm, pmax, ncol;         // the launch's PM; the columns asked for
    int rcap;
    long long cnt0, cntr;       // count(r) = cnt0 - r * cntr
};

// one wavefront per output (r, col): lane l adds the slots l, l + 64, ... in order, then the lanes combine in a fixed tree;
// out[col * rcap + r] = sum / count(r)
__global__ void __launch_bounds__(SF_THREADS) k_strfn_finish(const double* __restrict__ slots, StrfnFinish f, double* __restrict__ out)
{
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (item >= f.nr * f.ncol) return;
    const int r = item / f.ncol, col = item % f.ncol;
    const int kc = col <= f.pmax ? col : 1 + f.pm + (col - 1 - f.pmax);
    double v = 0.0;
    for (int g = lane; g < f.nwg; g += 64) v += slots[((long)g * f.nr + r) * f.nck + kc];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) out[(long)col * f.rcap + r] = v / (double)(f.cnt0 - (long long)r * f.cntr);
}

int pow2_floor(int v) { int p = 1; while (2 * p <= v) p *= 2; return p; }
int pow2_ceil(int v) { int p = 1; while (p < v) p *= 2; return p; }
int ilog2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }
int strfn_pm(int pmax) { return pmax <= 2 ? 2 : (pmax <= 4 ? 4 : 8); }

StrfnPass strfn_pass(const Geometry& g, int d, int rmax)
{
    const int nx = g.domain.len(0), ny = g.domain.len(1), nz = g.domain.len(2);
    StrfnPass ps;
    ps.n = g.domain.len(d);
    ps.rmax = rmax;
    ps.len = g.periodic[d] ? ps.n + rmax : ps.n;
    ps.x = d == 0;
    ps.ncolumns = d == 0 ? ny * nz : nx;
    const int tw_ = std::min({64, pow2_floor(SF_TILE_ELEMS / ps.len), pow2_ceil(ps.ncolumns)});
    ps.ltw = ilog2(tw_);
    ps.ts = d == 0 ? tw_ + 1 : tw_;
    ps.ntile_row = (ps.ncolumns + tw_ - 1) / tw_;
    ps.ntiles = ps.ntile_row * (d == 0 ? 1 : (d == 1 ? nz : ny));
    ps.estride = d == 1 ? nx : (long)nx * ny;
    ps.ostride = d == 1 ? (long)nx * ny : nx;
    return ps;
}

int strfn_nwg(const StrfnPass& ps) { return std::min(ps.ntiles, SF_MAXWG); }

template <int PM>
void strfn_launch_pm(const StrfnPass& ps, bool per, const double* R, double* slots)
{
    auto& ctx = Context::get();
    const size_t lds = (size_t)ps.len * ps.ts * sizeof(double);
    IAMRX_ASSERT(lds <= 65536);
    const dim3 grid((unsigned)strfn_nwg(ps));
    if (per) hipLaunchKernelGGL((k_strfn_pairs<PM, true>), grid, dim3(SF_THREADS), lds, ctx.stream, R, ps, slots);
    else hipLaunchKernelGGL((k_strfn_pairs<PM, false>), grid, dim3(SF_THREADS), lds, ctx.stream, R, ps, slots);
}

// axis d of the dense array R: the pair launch and its finish; out: the ncol * rcap doubles of (d, component)
void strfn_axis(const Geometry& g, int d, int rmax, int pmax, int rcap, const double* R, double* slots, double* out)
{
    auto& ctx = Context::get();
    const StrfnPass ps = strfn_pass(g, d, rmax);
    const int pm = strfn_pm(pmax);
    if (pm == 2) strfn_launch_pm<2>(ps, g.periodic[d] != 0, R, slots);
    else if (pm == 4) strfn_launch_pm<4>(ps, g.periodic[d] != 0, R, slots);
    else strfn_launch_pm<8>(ps, g.periodic[d] != 0, R, slots);
    StrfnFinish f;
    f.nwg = strfn_nwg(ps); f.nr = rmax + 1; f.nck = 1 + pm + (pm + 1) / 2;
    f.pm = pm; f.pmax = pmax; f.ncol = strfn_ncol(pmax); f.rcap = rcap;
    f.cnt0 = strfn_count(g, d, 0); f.cntr = f.cnt0 - strfn_count(g, d, 1);
    const int items = f.nr * f.ncol;
    hipLaunchKernelGGL(k_strfn_finish, dim3((unsigned)((items + 3) / 4)), dim3(SF_THREADS), 0, ctx.stream, slots, f, out);
}

void strfn_mean(const Geometry& g, const double* R, double* slots, double* out)
{
    auto& ctx = Context::get();
    const long N = g.domain.npts();
    const int nwg = (int)std::min<long>((N + SF_THREADS - 1) / SF_THREADS, SF_SUMWG);
    hipLaunchKernelGGL(k_strfn_sum, dim3((unsigned)nwg), dim3(SF_THREADS), 0, ctx.stream, R, N, slots);
    StrfnFinish f;
    f.nwg = nwg; f.nr = 1; f.nck = 1; f.pm = 0; f.pmax = 0; f.ncol = 1; f.rcap = 1; f.cnt0 = N; f.cntr = 0;
    hipLaunchKernelGGL(k_strfn_finish, dim3(1), dim3(SF_THREADS), 0, ctx.stream, slots, f, out);
}

// doubles of the slots a call needs: the largest pair launch of its axes (the mean's share is smaller)
size_t strfn_slots(const Geometry& g, const int rmax[3], int pmax)
{
    const int pm = strfn_pm(pmax);
    size_t n = SF_SUMWG;
    for (int d = 0; d < 3; ++d)
        if (rmax[d] > 0) n = std::max(n, (size_t)strfn_nwg(strfn_pass(g, d, rmax[d])) * (rmax[d] + 1) * (1 + pm + (pm + 1) / 2));
    return n;
}

}  // namespace

int strfn_ncol(int pmax)
{
    if (pmax < 1 || pmax > STRFN_PMAX) throw Error("strfn: pmax = " + std::to_string(pmax) + " outside 1 .. " + std::to_string(STRFN_PMAX));
    return 1 + pmax + (pmax + 1) / 2;
}

void strfn_resolve_rmax(const Geometry& g, const int rmax[3], int out[3])
{
    static const char* axis = "xyz";
    for (int d = 0; d < 3; ++d) {
        const int n = g.domain.len(d);
        const int lim = g.periodic[d] ? n / 2 : n - 1;
        if (rmax[d] < -1 || rmax[d] > lim)
            throw Error(std::string("strfn: rmax_") + axis[d] + " = " + std::to_string(rmax[d]) + " outside -1 .. " + std::to_string(lim) + " (n_" + axis[d] + " = " +
                        std::to_string(n) + (g.periodic[d] ? ", periodic: n / 2)" : ", not periodic: n - 1)"));
        out[d] = rmax[d] < 0 ? lim : rmax[d];
        if (out[d] > 0 && n > STRFN_MAX_EXTENT)
            throw Error(std::string("strfn: extent n_") + axis[d] + " = " + std::to_string(n) + " above " + std::to_string(STRFN_MAX_EXTENT));
    }
}

long long strfn_count(const Geometry& g, int d, int r)
{
    const long long N = g.domain.npts(), n = g.domain.len(d);
    return g.periodic[d] ? N : (n - r) * (N / n);
}

void strfn_compute(const Geometry& g, const MultiFab& S, int nq, const int* comps, int pmax, const int rmax[3], int rcap, double* out, double* mean)
{
    const int ncol = strfn_ncol(pmax);
    if (!S.type.cell()) throw Error("strfn: the array is not cell-centred");
    for (int q = 0; q < nq; ++q)
        if (comps[q] < 0 || comps[q] >= S.ncomp) throw Error("strfn: component " + std::to_string(comps[q]) + " outside 0 .. " + std::to_string(S.ncomp - 1));
    for (int d = 0; d < 3; ++d) IAMRX_ASSERT(rmax[d] >= 0 && rmax[d] < rcap && (rmax[d] == 0 || g.domain.len(d) <= STRFN_MAX_EXTENT));
    dense_check_cover("strfn", g, *S.layout);
    auto& ctx = Context::get();
    const size_t nsf = (size_t)3 * nq * ncol * rcap, nout = nsf + nq;
    DevBuf<double> R((size_t)g.domain.npts()), slots(strfn_slots(g, rmax, pmax)), d_out(nout);
    IAMRX_HIP_CHECK(hipMemsetAsync(d_out, 0, nout * sizeof(double), ctx.stream));         // the separations beyond an axis's rmax
    for (int q = 0; q < nq; ++q) {
        dense_gather(g, S, comps[q], R);
        for (int d = 0; d < 3; ++d)
            if (rmax[d] > 0) strfn_axis(g, d, rmax[d], pmax, rcap, R, slots, d_out + ((size_t)d * nq + q) * ncol * rcap);
        strfn_mean(g, R, slots, d_out + nsf + q);
    }
    const double* h = ctx.read_back(d_out, nout);
    std::copy(h, h + nsf, out);
    if (mean) std::copy(h + nsf, h + nout, mean);
}

void strfn_bench(const Geometry& g, const MultiFab& S, int comp, int pmax, const int rmax[3], int reps, float* ms)
{
    const int ncol = strfn_ncol(pmax);
    dense_check_cover("strfn", g, *S.layout);
    IAMRX_ASSERT(S.type.cell() && comp >= 0 && comp < S.ncomp && reps >= 1);
    int rcap = 1;
    for (int d = 0; d < 3; ++d) { IAMRX_ASSERT(rmax[d] >= 0); rcap = std::max(rcap, rmax[d] + 1); }
    DevBuf<double> R((size_t)g.domain.npts()), slots(strfn_slots(g, rmax, pmax)), d_out((size_t)3 * ncol * rcap);
    PassTimer t(5);
    for (int r = 0; r < reps; ++r) {
        t.mark();
        dense_gather(g, S, comp, R);
        t.mark();
        for (int d = 0; d < 3; ++d) {
            if (rmax[d] > 0) strfn_axis(g, d, rmax[d], pmax, rcap, R, slots, d_out + (size_t)d * ncol * rcap);
            t.mark();
        }
        t.finish(ms + 4 * r);
    }
}


}  // namespace iamrx
