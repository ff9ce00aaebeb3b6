// iamr_amd/csrc/k_velgrad.hip -- derived fields of the velocity-gradient tensor: diveru, the vorticity components, enstrophy, strain rate,
// viscous dissipation, the invariants Q and R, helicity.  This library's own derived quantities (upstream's derive list has mag_vort,
// NS_derive.cpp:86-264, and nothing else of the gradient); DESIGN.md section 4.
//
// A[3 n + d] = d u_n / d x_d at the cell centre, the centred difference over the FillPatched velocity with one ghost layer, written as
// derive_mag_vort (regrid.hip) writes it: 0.5 * (u_n(+e_d) - u_n(-e_d)) * (1 / dx_d), left to right; the file is built without FMA
// contraction.  ONE pass forms the nine entries once per cell and writes any subset of the ten quantities (a run-time list of at most
// VELGRAD_NQ ids; output q goes to component ocomp + q).  With
//   SS = A00^2 + A11^2 + A22^2 + 0.5 * ((A01 + A10)^2 + (A02 + A20)^2 + (A12 + A21)^2)      (= S_ij S_ij, each sum in that order)
//   0 diveru       (A00 + A11) + A22
//   1 2 3 vort_x / vort_y / vort_z   A21 - A12, A02 - A20, A10 - A01 (the three terms under the root of mag_vort)
//   4 enstrophy    0.5 * (vort_x^2 + vort_y^2 + vort_z^2)
//   5 strain_rate  sqrt(2 SS)
//   6 dissipation  mu * (2 SS): the molecular part only, also in an LES run; a rate per unit volume, the partner of "energy"
//   7 q_criterion  0.5 * (enstrophy - SS)      (= -A_ij A_ji / 2)
//   8 r_invariant  -det(A), cofactor expansion along the first row
//   9 helicity     u vort_x + v vort_y + w vort_z with the cell's own velocity
// Only the face neighbours of a cell are read.
//
// Two kernels, one cell function (velgrad_cell), so the two cannot diverge -- the arrangement of k_les.hip:
//   k_velgrad_zm     a 32 x 8 workgroup marches a z-chunk with the three-plane ring of the velocity tile (LdsVel) in LDS; tile order and
//                    chunk sizing of k_les_mut.  The tile's edge cells are staged but never read.
//   k_velgrad_plain  level_tiling over the cells of every fab, reads from L1 / L2; levels of short boxes, and with four or more boxes of
//                    unequal size the flat list of the tiles that exist.
// Which one a call takes is decided once per call from the layout (velgrad_path): see derive_velgrad.
#include "kernels.h"
#include "launch.h"
#include "tensor_lds.h"
#include <algorithm>

namespace iamrx {

struct VelgradArgs {
    double dxi, dyi, dzi, mu;
    int vcomp, ocomp;
    int nq;
    int id[VELGRAD_NQ];
};

struct VgVelAt {
    FabD v; int c0;
    __device__ __forceinline__ double operator()(int i, int j, int k, int n) const { return v(i, j, k, c0 + n); }
};

// quantity `id` of one cell from its gradient A and its velocity; everything but the root is shared arithmetic of a few dozen flops
// (the kernels are bound by memory), so it is formed once and `id` -- uniform over the launch -- picks
struct VelgradCell {
    double div, wx, wy, wz, ens, ss2, q, r, hel;
    __device__ __forceinline__ VelgradCell(const double A[9], double u, double v, double w)
    {
        div = (A[0] + A[4]) + A[8];
        wx = A[7] - A[5]; wy = A[2] - A[6]; wz = A[3] - A[1];
        ens = 0.5 * (wx * wx + wy * wy + wz * wz);
        const double s01 = A[1] + A[3], s02 = A[2] + A[6], s12 = A[5] + A[7];
        const double ss = A[0] * A[0] + A[4] * A[4] + A[8] * A[8] + 0.5 * (s01 * s01 + s02 * s02 + s12 * s12);
        ss2 = 2 * ss;
        q = 0.5 * (ens - ss);
        r = -(A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]));
        hel = u * wx + v * wy + w * wz;
    }
    __device__ __forceinline__ double pick(int id, double mu) const
    {
        switch (id) {
        case 0: return div;
        case 1: return wx;
        case 2: return wy;
        case 3: return wz;
        case 4: return ens;
        case 5: return sqrt(ss2);
        case 6: return mu * ss2;
        case 7: return q;
        case 8: return r;
        default: return hel;
        }
    }
};

template <class VA>
__device__ __forceinline__ void velgrad_cell(const VA& v, int i, int j, int k, const VelgradArgs& p, const FabD& out)
{
    double A[9];
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        A[3 * n + 0] = 0.5 * (v(i + 1, j, k, n) - v(i - 1, j, k, n)) * p.dxi;
        A[3 * n + 1] = 0.5 * (v(i, j + 1, k, n) - v(i, j - 1, k, n)) * p.dyi;
        A[3 * n + 2] = 0.5 * (v(i, j, k + 1, n) - v(i, j, k - 1, n)) * p.dzi;
    }
    const VelgradCell c(A, v(i, j, k, 0), v(i, j, k, 1), v(i, j, k, 2));
    // the slots are a run-time list: unrolled with a uniform branch, so that no array is indexed at run time (p.id[s] is a kernel argument)
#pragma unroll
    for (int s = 0; s < VELGRAD_NQ; ++s)
        if (s < p.nq) out(i, j, k, p.ocomp + s) = c.pick(p.id[s], p.mu);
}

__global__ void __launch_bounds__(256) k_velgrad_plain(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ vt, const FabD* __restrict__ ot, VelgradArgs p)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    if (!tile_ijk(t, b, i, j, k0, k1)) return;
    const VgVelAt v{vt[fab], p.vcomp};
    const FabD out = ot[fab];
    for (int k = k0; k <= k1; ++k) velgrad_cell(v, i, j, k, p, out);
}

template <int TX, int TY>
__global__ void __launch_bounds__(TX * TY) k_velgrad_zm(const BoxD* __restrict__ boxes, const FabD* __restrict__ vt, const FabD* __restrict__ ot, VelgradArgs p,
                                                        int ntx, int nty, int nkc, int kcs, int xcd_cnt)
{
    constexpr int NT = TX * TY, W = TX + 2, H = TY + 2, PS = W * H;
    __shared__ double V[3][3 * PS];
    const int fab = blockIdx.y;
    const BoxD b = boxes[fab];
    int bid = blockIdx.x;
    if (xcd_cnt > 0) {
        bid = (bid & 7) * xcd_cnt + (bid >> 3);          // XCD-aware order, see make_tiling
        if (bid >= ntx * nty * nkc) return;
    }
    const int tix = bid % ntx, r1 = bid / ntx, tiy = r1 % nty, kci = r1 / nty;
    const int tx0 = b.lo[0] + tix * TX, ty0 = b.lo[1] + tiy * TY, k0 = b.lo[2] + kci * kcs;
    if (tx0 > b.hi[0] || ty0 > b.hi[1] || k0 > b.hi[2]) return;          // (the whole workgroup leaves: no barrier is skipped by a part of it)
    const int k1 = min(k0 + kcs - 1, b.hi[2]);
    const int tid = threadIdx.x;
    const int i = tx0 + tid % TX, j = ty0 + tid / TX;
    const bool on = i <= b.hi[0] && j <= b.hi[1];
    const FabD v = vt[fab], out = ot[fab];
    const int vhx = min(tx0 + TX, b.hi[0] + 1), vhy = min(ty0 + TY, b.hi[1] + 1);      // last staged column / row (ghost included)
    const long vc0 = v.cs * p.vcomp;
    auto stage = [&](int k) {
        double* dst = V[((k % 3) + 3) % 3];
        for (int e = tid; e < PS; e += NT) {
            const int ii = tx0 - 1 + e % W, jj = ty0 - 1 + e / W;
            if (ii <= vhx && jj <= vhy) {
                const long o = v.off(ii, jj, k) + vc0;
#pragma unroll
                for (int n = 0; n < 3; ++n) dst[e + PS * n] = v.gp()[o + v.cs * n];
            }
        }
    };
    // the plane after the next one travels through registers, as in k_les_mut: fetched before the arithmetic of a plane, written to LDS at
    // the top of the next iteration
    constexpr int NE = (PS + NT - 1) / NT;
    double pf[NE][3];
    long pfo[NE];
#pragma unroll
    for (int s_ = 0; s_ < NE; ++s_) {
        const int e = tid + s_ * NT;
        const int ii = tx0 - 1 + e % W, jj = ty0 - 1 + e / W;
        pfo[s_] = (e < PS && ii <= vhx && jj <= vhy) ? v.off(ii, jj, k0) + vc0 : -1;      // (>= 0: the cell lies in the array)
    }
    const long vks = (long)v.n[0] * v.n[1];
    auto fetch = [&](int k) {
#pragma unroll
        for (int s_ = 0; s_ < NE; ++s_)
            if (pfo[s_] >= 0) {
                const long o = pfo[s_] + vks * (k - k0);
#pragma unroll
                for (int n = 0; n < 3; ++n) pf[s_][n] = v.gp()[o + v.cs * n];
            }
    };
    auto commit = [&](int k) {
        double* dst = V[((k % 3) + 3) % 3];
#pragma unroll
        for (int s_ = 0; s_ < NE; ++s_)
            if (pfo[s_] >= 0) {
                const int e = tid + s_ * NT;
#pragma unroll
                for (int n = 0; n < 3; ++n) dst[e + PS * n] = pf[s_][n];
            }
    };
    stage(k0 - 1);
    stage(k0);
    fetch(k0 + 1);
    LdsVel<TX, TY> a;
    a.i0 = tx0 - 1; a.j0 = ty0 - 1;
    for (int k = k0; k <= k1; ++k) {
        commit(k + 1);
        if (k < k1) fetch(k + 2);
        __syncthreads();
        a.kc = k; a.pm = V[((k - 1) % 3 + 3) % 3]; a.p0 = V[(k % 3 + 3) % 3]; a.pp = V[((k + 1) % 3 + 3) % 3];
        if (on) velgrad_cell(a, i, j, k, p, out);
        __syncthreads();
    }
}

static VelgradArgs velgrad_args(const Geometry& g, const MultiFab& out, int ocomp, int nq, const int* which, const MultiFab& vel, int vcomp, double mu)
{
    if (nq < 1 || nq > VELGRAD_NQ || !which) throw Error("iamrx derive_velgrad: the number of quantities must be 1 .. " + std::to_string(VELGRAD_NQ) + ", not " + std::to_string(nq));
    if (!vel.type.cell() || !out.type.cell()) throw Error("iamrx derive_velgrad: the arrays must be cell-centred");
    if (vel.ngrow < 1) throw Error("iamrx derive_velgrad: the velocity needs at least one ghost layer");
    if (vcomp < 0 || vcomp + 3 > vel.ncomp) throw Error("iamrx derive_velgrad: velocity components " + std::to_string(vcomp) + " .. " + std::to_string(vcomp + 2) + " outside the array's " + std::to_string(vel.ncomp));
    if (ocomp < 0 || ocomp + nq > out.ncomp) throw Error("iamrx derive_velgrad: output components " + std::to_string(ocomp) + " .. " + std::to_string(ocomp + nq - 1) + " outside the array's " + std::to_string(out.ncomp));
    if (out.layout->id != vel.layout->id) throw Error("iamrx derive_velgrad: the two arrays live on different layouts");
    VelgradArgs p;
    p.dxi = 1.0 / g.dx[0]; p.dyi = 1.0 / g.dx[1]; p.dzi = 1.0 / g.dx[2];
    p.mu = mu; p.vcomp = vcomp; p.ocomp = ocomp; p.nq = nq;
    for (int q = 0; q < VELGRAD_NQ; ++q) p.id[q] = 0;
    for (int q = 0; q < nq; ++q) {
        if (which[q] < 0 || which[q] >= VELGRAD_NQ) throw Error("iamrx derive_velgrad: unknown quantity id " + std::to_string(which[q]) + " (0 .. " + std::to_string(VELGRAD_NQ - 1) + ")");
        p.id[q] = which[q];
    }
    return p;
}

// the form a call takes: 1 marching, 2 plain.  path 0: the marching form when the level's largest box holds a full 32 x 8 tile (the rule
// of k_les_mut, here over the boxes of ALL ranks, so every rank decides alike; a rank whose own boxes are shorter runs the same kernel
// with partly idle tiles); 1 / 2 force a form
int velgrad_path(const Layout& l, int path)
{
    if (path < 0 || path > 2) throw Error("iamrx derive_velgrad: path must be 0 (by the layout), 1 (marching) or 2 (plain), not " + std::to_string(path));
    int mx = 0, my = 0;
    for (const BoxD& b : l.boxes) { mx = std::max(mx, b.hi[0] - b.lo[0] + 1); my = std::max(my, b.hi[1] - b.lo[1] + 1); }
    const bool full = mx >= 32 && my >= 8;
    if (path == 1 && !full) throw Error("iamrx derive_velgrad: path 1 (marching form) needs a box of at least 32 x 8 cells in x and y, the largest has " +
                                        std::to_string(mx) + " x " + std::to_string(my));
    return path == 0 ? (full ? 1 : 2) : path;
}

static void velgrad_launch(const Layout& l, const MultiFab& out, const MultiFab& vel, const VelgradArgs& p, int form)
{
    hipStream_t s = Context::get().stream;
    if (form == 1) {
        constexpr int TX = 32, TY = 8;
        const int ntx = (l.max_len[0] + TX - 1) / TX, nty = (l.max_len[1] + TY - 1) / TY;
        const int kcs = std::min(32, std::max(4, l.max_len[2] / 8));
        const int nkc = (l.max_len[2] + kcs - 1) / kcs;
        const int total = ntx * nty * nkc;
        const int xcd_cnt = total >= 64 ? (total + 7) / 8 : 0;
        dim3 grid((unsigned)(xcd_cnt > 0 ? 8 * xcd_cnt : total), (unsigned)l.nlocal());
        hipLaunchKernelGGL((k_velgrad_zm<TX, TY>), grid, dim3(TX * TY), 0, s, l.d_boxes, vel.d_tab, out.d_tab, p, ntx, nty, nkc, kcs, xcd_cnt);
        return;
    }
    Tiling t = level_tiling(l, cell_type(), 0, 4, true);
    hipLaunchKernelGGL(k_velgrad_plain, t.grid(), Tiling::block(), 0, s, t, l.d_boxes, vel.d_tab, out.d_tab, p);
}

void derive_velgrad(const Geometry& g, MultiFab& out, int ocomp, int nq, const int* which, const MultiFab& vel, int vcomp, double mu, int path)
{
    const VelgradArgs p = velgrad_args(g, out, ocomp, nq, which, vel, vcomp, mu);
    const int form = velgrad_path(*vel.layout, path);
    if (vel.nlocal() == 0) return;
    velgrad_launch(*vel.layout, out, vel, p, form);
}

// ms[r] = time of `ncalls` launches between two events (ncalls = 1: one call of nq outputs; ncalls = nq: one single-output call per
// quantity, the cost structure without the fused pass).  Nothing is read back.
void velgrad_bench(const Geometry& g, MultiFab& out, int nq, const int* which, const MultiFab& vel, int vcomp, double mu, int path, bool split, int reps, float* ms)
{
    IAMRX_ASSERT(reps >= 1 && ms);
    auto& ctx = Context::get();
    const VelgradArgs p = velgrad_args(g, out, 0, nq, which, vel, vcomp, mu);
    const int form = velgrad_path(*vel.layout, path);
    if (vel.nlocal() == 0) { for (int r = 0; r < reps; ++r) ms[r] = 0.f; return; }
    PassTimer t(2);
    for (int r = 0; r < reps; ++r) {
        t.mark();
        if (!split) velgrad_launch(*vel.layout, out, vel, p, form);
        else for (int q = 0; q < nq; ++q) {
            VelgradArgs one = p;
            one.nq = 1; one.id[0] = p.id[q]; one.ocomp = q;
            velgrad_launch(*vel.layout, out, vel, one, form);
        }
        t.mark();
        t.finish(ms + r);
    }
    ctx.sync();
}

}  // namespace iamrx
