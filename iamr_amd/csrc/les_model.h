// iamr_amd/csrc/les_model.h -- the eddy-viscosity operators of the LES closure as ONE device function: k_les.hip runs it on the face
// gradients of a step, k_sgs.hip on the centred gradient of a filtered field (the a-priori analysis), so the two cannot diverge.
#pragma once
#include <hip/hip_runtime.h>

namespace iamrx {

// mu_t of one gradient g[3 n + d] = d u_n / d x_d, statement by statement as NS_LES.cpp:114-211.  MODEL 0: Smagorinsky, 1: Sigma
template <int MODEL>
__device__ __forceinline__ double les_model(const double g[9], double fac)
{
    if (MODEL == 0) {
        // :125-134.  "symij" doubles each component -- it is NOT the symmetric part g_ij + g_ji; the reference's expression, kept
        double smag = 0.0;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const double symij = g[q] + g[q];
            smag += symij * symij;
        }
        smag = 0.5 * smag;
        return fac * sqrt(smag);
    }
    // Sigma (Nicoud, Baya Toda, Cabrit, Bose, Lee, Phys. Fluids 23 (2011) 085106), :153-209
    const double G_11 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    const double G_12 = g[0] * g[3] + g[1] * g[4] + g[2] * g[5];
    const double G_13 = g[0] * g[6] + g[1] * g[7] + g[2] * g[8];
    const double G_22 = g[3] * g[3] + g[4] * g[4] + g[5] * g[5];
    const double G_23 = g[3] * g[6] + g[4] * g[7] + g[5] * g[8];
    const double G_33 = g[6] * g[6] + g[7] * g[7] + g[8] * g[8];
    const double I1 = G_11 + G_22 + G_33;
    const double I2 = G_11 * G_22 - G_12 * G_12 + G_22 * G_33 - G_23 * G_23 + G_11 * G_33 - G_13 * G_13;
    const double I3 = G_11 * (G_22 * G_33 - G_23 * G_23) - G_12 * (G_33 * G_12 - G_13 * G_23) + G_13 * (G_12 * G_23 - G_13 * G_22);
    const double t = I1 / 3;
    const double alpha1 = fmax(0., t * t - I2 / 3);
    if (alpha1 == 0.) return 0.;
    const double alpha2 = t * t * t - I1 * I2 / 6 + I3 / 2;
    double alphaArg = (alpha2 * sqrt(1 / alpha1)) / alpha1;
    if (alphaArg > 1.) alphaArg = 1.;
    else if (alphaArg < -1.) alphaArg = -1.;
    const double alpha3 = acos(alphaArg) / 3;
    constexpr double Pi = 3.14159265358979323846264338327950288;
    double sigma1 = sqrt(fmax(0., t + 2 * sqrt(alpha1) * cos(alpha3)));
    double sigma2 = sqrt(fmax(0., t - 2 * sqrt(alpha1) * cos(Pi / 3 + alpha3)));
    const double sigma3 = sqrt(fmax(0., t - 2 * sqrt(alpha1) * cos(Pi / 3 - alpha3)));
    const double verysmall = 1.e-24;
    sigma2 = fmax(sigma3, sigma2);
    sigma1 = fmax(sigma2, sigma1);
    sigma1 = fmax(verysmall, sigma1);
    return fac * ((sigma3 * (sigma1 - sigma2) * (sigma2 - sigma3)) / (sigma1 * sigma1));
}

}  // namespace iamrx
