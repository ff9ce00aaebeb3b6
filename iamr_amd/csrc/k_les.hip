// iamr_amd/csrc/k_les.hip -- large-eddy simulation: the eddy viscosity of the Smagorinsky and the Sigma model on the faces of a level.
// Role: NavierStokesBase::calc_mut_LES (reference Source/NS_LES.cpp:22-225) behind its FillPatch and boundary step, i.e. MLTensorOp::compVelGrad
// (:97) and the model loops (:105-222), and the setVal + Add of NavierStokes::getViscosity (Source/NavierStokes.cpp:2119-2153).
//
// The reference writes the nine velocity-gradient components on each of the three face arrays (27 doubles per cell), reads them back in the
// model loop, then adds the molecular viscosity in two more passes.  Here ONE launch per level reads the cell velocity (one ghost layer)
// and writes the three 1-component face arrays out_d = base + mu_t: the gradients live in registers only.
//
// Gradients on a d-face: the normal derivative is the two-point difference across the face, the transverse derivatives are the four-point
// means of the tensor operator's cross fluxes (cross_flux<D>, k_tensor.hip).  Upstream's compVelGrad is not in the reference tree; this is
// the project's own restatement.  g[3 n + d] = d u_n / d x_d; both models are invariant under transposing g, so the
// component order upstream uses cannot change the result.
//
// Two kernels, one model function (les_model, les_model.h), so the two cannot diverge:
//   k_les_mut        a 32 x 8 workgroup marches a z-chunk with the three-plane ring of the velocity tile (LdsVel) in LDS, XCD-aware tile
//                    order and chunk sizing of k_tensor_cross_zm.  Taken when the level's largest box has at least one full tile
//                    (max_len[0] >= 32 && max_len[1] >= 8, the rule of tensor_cross_terms_sub).  Its grid is sized for the largest box; on a
//                    level of unequal boxes the workgroups beyond a smaller box return at once.
//   k_les_mut_plain  level_tiling over the nodal box of every fab, reads from L1 / L2.  Levels of short boxes; with four or more boxes of
//                    unequal size level_tiling hands it the flat list of the tiles that exist.
// Every thread owns the x-, y- and z-face (i, j, k) of its cell; the threads on a box's high sides also write the face at hi + 1 (a face
// array has n + 1 faces per box and every one is written; faces shared by two boxes are written by both, with the same value when the
// ghost cells of the two agree).
#include "kernels.h"
#include "launch.h"
#include "les_model.h"
#include "tensor_lds.h"

namespace iamrx {

struct LesArgs {
    double dxi, dyi, dzi;
    double fac[3];       // (Cs dx[d])^2: the filter width is the cell size in the face's own direction (NS_LES.cpp:134, 209)
    double base;         // added to mu_t: the molecular viscosity in the level step
    int vcomp;           // first velocity component of the array
};

struct VelAt {
    FabD v; int c0;
    __device__ __forceinline__ double operator()(int i, int j, int k, int n) const { return v(i, j, k, c0 + n); }
};

// the nine gradient components on the d-face (i, j, k)
template <int D, class VA>
__device__ __forceinline__ void les_face_grad(const VA& v, int i, int j, int k, const LesArgs& p, double g[9])
{
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        if (D == 0) {
            g[3 * n + 0] = (v(i, j, k, n) - v(i - 1, j, k, n)) * p.dxi;
            g[3 * n + 1] = (v(i, j + 1, k, n) + v(i - 1, j + 1, k, n) - v(i, j - 1, k, n) - v(i - 1, j - 1, k, n)) * (0.25 * p.dyi);
            g[3 * n + 2] = (v(i, j, k + 1, n) + v(i - 1, j, k + 1, n) - v(i, j, k - 1, n) - v(i - 1, j, k - 1, n)) * (0.25 * p.dzi);
        } else if (D == 1) {
            g[3 * n + 0] = (v(i + 1, j, k, n) + v(i + 1, j - 1, k, n) - v(i - 1, j, k, n) - v(i - 1, j - 1, k, n)) * (0.25 * p.dxi);
            g[3 * n + 1] = (v(i, j, k, n) - v(i, j - 1, k, n)) * p.dyi;
            g[3 * n + 2] = (v(i, j, k + 1, n) + v(i, j - 1, k + 1, n) - v(i, j, k - 1, n) - v(i, j - 1, k - 1, n)) * (0.25 * p.dzi);
        } else {
            g[3 * n + 0] = (v(i + 1, j, k, n) + v(i + 1, j, k - 1, n) - v(i - 1, j, k, n) - v(i - 1, j, k - 1, n)) * (0.25 * p.dxi);
            g[3 * n + 1] = (v(i, j + 1, k, n) + v(i, j + 1, k - 1, n) - v(i, j - 1, k, n) - v(i, j - 1, k - 1, n)) * (0.25 * p.dyi);
            g[3 * n + 2] = (v(i, j, k, n) - v(i, j, k - 1, n)) * p.dzi;
        }
    }
}

// mu_t of one face from its gradient: les_model<MODEL> (les_model.h, shared with the a-priori analysis of k_sgs.hip)
template <int D, int MODEL, class VA>
__device__ __forceinline__ double les_face(const VA& v, int i, int j, int k, const LesArgs& p)
{
    double g[9];
    les_face_grad<D>(v, i, j, k, p, g);
    return p.base + les_model<MODEL>(g, p.fac[D]);
}

template <int MODEL>
__global__ void __launch_bounds__(256) k_les_mut_plain(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ vt, const FabD* __restrict__ mxt,
                                                       const FabD* __restrict__ myt, const FabD* __restrict__ mzt, LesArgs p)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    if (!tile_ijk(t, dev_grow_convert(b, 1, 1, 1, 0), i, j, k0, k1)) return;
    const VelAt v{vt[fab], p.vcomp};
    const FabD mx = mxt[fab], my = myt[fab], mz = mzt[fab];
    const bool inx = i <= b.hi[0], iny = j <= b.hi[1];
    for (int k = k0; k <= k1; ++k) {
        const bool inz = k <= b.hi[2];
        if (iny && inz) mx(i, j, k, 0) = les_face<0, MODEL>(v, i, j, k, p);
        if (inx && inz) my(i, j, k, 0) = les_face<1, MODEL>(v, i, j, k, p);
        if (inx && iny) mz(i, j, k, 0) = les_face<2, MODEL>(v, i, j, k, p);
    }
}

template <int MODEL, int TX, int TY>
__global__ void __launch_bounds__(TX * TY) k_les_mut(const BoxD* __restrict__ boxes, const FabD* __restrict__ vt, const FabD* __restrict__ mxt,
    const FabD* __restrict__ myt, const FabD* __restrict__ mzt, LesArgs p, int ntx, int nty, int nkc, int kcs, int xcd_cnt)
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
    const FabD v = vt[fab], mx = mxt[fab], my = myt[fab], mz = mzt[fab];
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
    // the plane after the next one travels through registers, as in k_tensor_cross_zm: fetched before the arithmetic of a plane, written to
    // LDS at the top of the next iteration
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
        if (on) {
            mx(i, j, k, 0) = les_face<0, MODEL>(a, i, j, k, p);
            my(i, j, k, 0) = les_face<1, MODEL>(a, i, j, k, p);
            mz(i, j, k, 0) = les_face<2, MODEL>(a, i, j, k, p);
            // the extra faces on the box's high sides
            if (i == b.hi[0]) mx(i + 1, j, k, 0) = les_face<0, MODEL>(a, i + 1, j, k, p);
            if (j == b.hi[1]) my(i, j + 1, k, 0) = les_face<1, MODEL>(a, i, j + 1, k, p);
            if (k == b.hi[2]) mz(i, j, k + 1, 0) = les_face<2, MODEL>(a, i, j, k + 1, p);
        }
        __syncthreads();
    }
}

void les_mut(const Geometry& g, const MultiFab& vel, int vcomp, int model, double Cs, double base, MultiFab* const mu[3])
{
    if (model != 0 && model != 1) throw Error("iamrx les_mut: unknown LES model (0 Smagorinsky, 1 Sigma)");
    IAMRX_ASSERT(vel.type.cell() && vel.ngrow >= 1 && vcomp >= 0 && vcomp + 3 <= vel.ncomp);
    for (int d = 0; d < 3; ++d) {
        const IndexType ft = face_type(d);
        IAMRX_ASSERT(mu[d]->layout->id == vel.layout->id && mu[d]->ncomp >= 1);
        for (int q = 0; q < 3; ++q) IAMRX_ASSERT(mu[d]->type.t[q] == ft.t[q]);
    }
    if (vel.nlocal() == 0) return;
    const Layout& l = *vel.layout;
    LesArgs p;
    p.dxi = 1.0 / g.dx[0]; p.dyi = 1.0 / g.dx[1]; p.dzi = 1.0 / g.dx[2];
    for (int d = 0; d < 3; ++d) p.fac[d] = (Cs * g.dx[d]) * (Cs * g.dx[d]);
    p.base = base;
    p.vcomp = vcomp;
    hipStream_t s = Context::get().stream;
    if (tune("LES_ZM", 1) != 0 && l.max_len[0] >= 32 && l.max_len[1] >= 8) {
        constexpr int TX = 32, TY = 8;
        const int ntx = (l.max_len[0] + TX - 1) / TX, nty = (l.max_len[1] + TY - 1) / TY;
        const int kcs = std::min(32, std::max(4, l.max_len[2] / 8));
        const int nkc = (l.max_len[2] + kcs - 1) / kcs;
        const int total = ntx * nty * nkc;
        const int xcd_cnt = total >= 64 ? (total + 7) / 8 : 0;
        dim3 grid((unsigned)(xcd_cnt > 0 ? 8 * xcd_cnt : total), (unsigned)l.nlocal());
#define IAMRX_LES(M) hipLaunchKernelGGL((k_les_mut<M, TX, TY>), grid, dim3(TX * TY), 0, s, l.d_boxes, vel.d_tab, mu[0]->d_tab, mu[1]->d_tab, mu[2]->d_tab, \
                                        p, ntx, nty, nkc, kcs, xcd_cnt)
        if (model == 0) IAMRX_LES(0); else IAMRX_LES(1);
#undef IAMRX_LES
        return;
    }
    Tiling t = level_tiling(l, node_type(), 0, 4, true);
    if (model == 0)
        hipLaunchKernelGGL(k_les_mut_plain<0>, t.grid(), Tiling::block(), 0, s, t, l.d_boxes, vel.d_tab, mu[0]->d_tab, mu[1]->d_tab, mu[2]->d_tab, p);
    else
        hipLaunchKernelGGL(k_les_mut_plain<1>, t.grid(), Tiling::block(), 0, s, t, l.d_boxes, vel.d_tab, mu[0]->d_tab, mu[1]->d_tab, mu[2]->d_tab, p);
}

}  // namespace iamrx
