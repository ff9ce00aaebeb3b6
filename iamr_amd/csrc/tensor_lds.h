// iamr_amd/csrc/tensor_lds.h -- the velocity tile of the kernels that march a TX x TY column of cells through z with the 3-component
// velocity (one ghost cell in x and y) staged in LDS: k_tensor_cross_zm (k_tensor.hip) and k_les_mut (k_les.hip).
#pragma once

namespace iamrx {

template <int TX, int TY>
struct LdsVel {
    static constexpr int W = TX + 2, H = TY + 2, PS = W * H;
    const double *pm, *p0, *pp;      // planes kc-1, kc, kc+1 (3 components each, component stride PS)
    int kc, i0, j0;
    __device__ __forceinline__ double operator()(int i, int j, int k, int n) const
    {
        const int d = k - kc;
        const double* p = d < 0 ? pm : (d > 0 ? pp : p0);
        return p[(i - i0) + W * (j - j0) + PS * n];
    }
};

}  // namespace iamrx
