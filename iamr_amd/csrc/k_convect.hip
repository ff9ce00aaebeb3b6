// iamr_amd/csrc/k_convect.hip -- the nonlinear term of the momentum equation in its skew-symmetric centred form, the field whose
// co-spectrum with the velocity is the spectral energy transfer T(k) (this library's own diagnostic: k_spectrum.hip).
//
// With h_d = 0.5 / dx_d and delta_d f(x) = (f(x + e_d) - f(x - e_d)) * h_d, for i = 0, 1, 2:
//   N_i(x) = 0.5 * sum_d [ u_d(x) * delta_d u_i(x) + delta_d(u_d u_i)(x) ]
// evaluated as
//   a_d = u_d(x) * ((u_i(+e_d) - u_i(-e_d)) * h_d),   b_d = (u_d(+e_d) * u_i(+e_d) - u_d(-e_d) * u_i(-e_d)) * h_d,
//   N_i = 0.5 * (((a_0 + b_0) + (a_1 + b_1)) + (a_2 + b_2));
// the file is built without FMA contraction.  On a periodic grid sum_x u_i N_i = 0 identically (summation by parts: the advective half and
// the divergence half cancel term by term), whatever the divergence of u: the transfer sums to zero over the shells up to rounding.
// Only the six face neighbours of a cell are read, so one filled ghost layer suffices and a wall's ghost cell is differenced like any other.
//
// One kernel, the plain form of k_velgrad.hip (level_tiling over the cells of every fab, neighbours from L1 / L2); a plane-ring form is
// not built: DESIGN.md section 4.
#include "kernels.h"
#include "launch.h"

namespace iamrx {

struct ConvectArgs {
    double h[3];
    int vcomp, ocomp;
};

template <class VA>
__device__ __forceinline__ void convect_cell(const VA& v, int i, int j, int k, const ConvectArgs& p, const FabD& out)
{
    double c[3], lo[3][3], hi[3][3];          // the cell's velocity; [d][n]: component n at x - e_d / x + e_d
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        c[n] = v(i, j, k, n);
        lo[0][n] = v(i - 1, j, k, n); hi[0][n] = v(i + 1, j, k, n);
        lo[1][n] = v(i, j - 1, k, n); hi[1][n] = v(i, j + 1, k, n);
        lo[2][n] = v(i, j, k - 1, n); hi[2][n] = v(i, j, k + 1, n);
    }
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        double t[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double a = c[d] * ((hi[d][n] - lo[d][n]) * p.h[d]);
            const double b = (hi[d][d] * hi[d][n] - lo[d][d] * lo[d][n]) * p.h[d];
            t[d] = a + b;
        }
        out(i, j, k, p.ocomp + n) = 0.5 * ((t[0] + t[1]) + t[2]);
    }
}

struct CvVelAt {
    FabD v; int c0;
    __device__ __forceinline__ double operator()(int i, int j, int k, int n) const { return v(i, j, k, c0 + n); }
};

__global__ void __launch_bounds__(256) k_convect_plain(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ vt, const FabD* __restrict__ ot, ConvectArgs p)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    if (!tile_ijk(t, b, i, j, k0, k1)) return;
    const CvVelAt v{vt[fab], p.vcomp};
    const FabD out = ot[fab];
    for (int k = k0; k <= k1; ++k) convect_cell(v, i, j, k, p, out);
}

static ConvectArgs convect_args(const Geometry& g, const MultiFab& out, int ocomp, const MultiFab& vel, int vcomp)
{
    if (!vel.type.cell() || !out.type.cell()) throw Error("iamrx convective_term: the arrays must be cell-centred");
    if (vel.ngrow < 1) throw Error("iamrx convective_term: the velocity needs at least one ghost layer");
    if (vcomp < 0 || vcomp + 3 > vel.ncomp) throw Error("iamrx convective_term: velocity components " + std::to_string(vcomp) + " .. " + std::to_string(vcomp + 2) + " outside the array's " + std::to_string(vel.ncomp));
    if (ocomp < 0 || ocomp + 3 > out.ncomp) throw Error("iamrx convective_term: output components " + std::to_string(ocomp) + " .. " + std::to_string(ocomp + 2) + " outside the array's " + std::to_string(out.ncomp));
    if (out.layout->id != vel.layout->id) throw Error("iamrx convective_term: the two arrays live on different layouts");
    ConvectArgs p;
    for (int d = 0; d < 3; ++d) p.h[d] = 0.5 / g.dx[d];
    p.vcomp = vcomp; p.ocomp = ocomp;
    return p;
}

static void convect_launch(const Layout& l, const MultiFab& out, const MultiFab& vel, const ConvectArgs& p)
{
    Tiling t = level_tiling(l, cell_type(), 0, 4, true);
    hipLaunchKernelGGL(k_convect_plain, t.grid(), Tiling::block(), 0, Context::get().stream, t, l.d_boxes, vel.d_tab, out.d_tab, p);
}

void convective_term(const Geometry& g, MultiFab& out, int ocomp, const MultiFab& vel, int vcomp)
{
    const ConvectArgs p = convect_args(g, out, ocomp, vel, vcomp);
    if (vel.nlocal() == 0) return;
    convect_launch(*vel.layout, out, vel, p);
}

// ms[r] = one launch between two events.  Nothing is read back.
void convective_bench(const Geometry& g, MultiFab& out, const MultiFab& vel, int vcomp, int reps, float* ms)
{
    IAMRX_ASSERT(reps >= 1 && ms);
    auto& ctx = Context::get();
    const ConvectArgs p = convect_args(g, out, 0, vel, vcomp);
    if (vel.nlocal() == 0) { for (int r = 0; r < reps; ++r) ms[r] = 0.f; return; }
    PassTimer t(2);
    for (int r = 0; r < reps; ++r) {
        t.mark();
        convect_launch(*vel.layout, out, vel, p);
        t.mark();
        t.finish(ms + r);
    }
    ctx.sync();
}

}  // namespace iamrx
