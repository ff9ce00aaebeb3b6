// iamr_amd/csrc/k_stats.hip -- on-the-fly velocity statistics: the accumulation of NavierStokesBase::time_average
// (reference Source/NS_average.cpp:19-69) and the derived quantity "velocity_average" (der_vel_avg, Source/NS_derive.cpp:11-45).
//
// Both are streaming kernels over the cells of a level: one launch for all its boxes (launch.h Tiling), x fastest across the wavefront,
// each thread the three velocity components of its cells.  Built with -ffp-contract=off and written in the reference's expression order,
// so numpy reproduces the accumulators to the bit (tests/test_gpu_stats.py).
#include "kernels.h"
#include "launch.h"

namespace iamrx {

// A = A + dt_avg * u;  FLUCT: vp = u - A / t_sum (the UPDATED A, t_sum = time_avg + dt_avg), R = R + dt_avg * vp * vp.
// The mean-only form neither reads nor writes components 3..5.  The state carries ghost cells, the accumulator none: each is indexed
// through its own table entry.  All loads of a cell are issued before its first store (the two arrays are different allocations, which
// the compiler cannot know).
template <bool FLUCT>
__global__ void __launch_bounds__(256) k_time_average(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ avg,
                                                      const FabD* __restrict__ st, int vcomp, double dt_avg, double t_sum)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    if (!tile_ijk(t, b, i, j, k0, k1)) return;
    const FabD a = avg[fab], s = st[fab];
    for (int k = k0; k <= k1; ++k) {
        double u[3], A[3], R[3];
#pragma unroll
        for (int n = 0; n < 3; ++n) { u[n] = s(i, j, k, vcomp + n); A[n] = a(i, j, k, n); if (FLUCT) R[n] = a(i, j, k, n + 3); }
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            A[n] = A[n] + dt_avg * u[n];
            if (FLUCT) { const double vp = u[n] - A[n] / t_sum; R[n] = R[n] + dt_avg * vp * vp; }
        }
#pragma unroll
        for (int n = 0; n < 3; ++n) { a(i, j, k, n) = A[n]; if (FLUCT) a(i, j, k, n + 3) = R[n]; }
    }
}

void stats_accumulate(MultiFab& avg, const MultiFab& S, int vcomp, double dt_avg, double t_sum, bool fluct)
{
    IAMRX_ASSERT(avg.type.cell() && S.type.cell() && avg.ncomp == 6 && avg.layout->id == S.layout->id && vcomp >= 0 && vcomp + 3 <= S.ncomp);
    const Layout& l = *avg.layout;
    if (l.nlocal() == 0) return;
    const Tiling t = level_tiling(l, cell_type(), 0, 4, true);
    hipStream_t s = Context::get().stream;
    if (fluct) hipLaunchKernelGGL((k_time_average<true>), t.grid(), Tiling::block(), 0, s, t, l.d_boxes, avg.d_tab, S.d_tab, vcomp, dt_avg, t_sum);
    else hipLaunchKernelGGL((k_time_average<false>), t.grid(), Tiling::block(), 0, s, t, l.d_boxes, avg.d_tab, S.d_tab, vcomp, dt_avg, t_sum);
}

// der_vel_avg: mean = A / time_avg, rms = sqrt(R / time_avg_fluct); the host hands over 1 for a divisor that is zero
__global__ void __launch_bounds__(256) k_vel_avg(Tiling t, const BoxD* __restrict__ boxes, const FabD* __restrict__ out, int ocomp,
                                                 const FabD* __restrict__ avg, double t_mean, double t_fluct)
{
    const int fab = tile_fab(t);
    const BoxD b = boxes[fab];
    int i, j, k0, k1;
    if (!tile_ijk(t, b, i, j, k0, k1)) return;
    const FabD o = out[fab], a = avg[fab];
    for (int k = k0; k <= k1; ++k) {
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            o(i, j, k, ocomp + n) = a(i, j, k, n) / t_mean;
            o(i, j, k, ocomp + 3 + n) = __dsqrt_rn(a(i, j, k, n + 3) / t_fluct);
        }
    }
}

void stats_derive_vel_avg(MultiFab& out, int ocomp, const MultiFab& avg, double t_mean, double t_fluct)
{
    IAMRX_ASSERT(out.type.cell() && avg.ncomp == 6 && out.layout->id == avg.layout->id && ocomp >= 0 && ocomp + 6 <= out.ncomp);
    const Layout& l = *avg.layout;
    if (l.nlocal() == 0) return;
    const Tiling t = level_tiling(l, cell_type(), 0, 4, true);
    hipLaunchKernelGGL(k_vel_avg, t.grid(), Tiling::block(), 0, Context::get().stream, t, l.d_boxes, out.d_tab, ocomp, avg.d_tab,
                       t_mean == 0.0 ? 1.0 : t_mean, t_fluct == 0.0 ? 1.0 : t_fluct);
}

}  // namespace iamrx
