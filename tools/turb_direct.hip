// tools/turb_direct.hip -- measurement aid, not part of the library: the turbulent forcing evaluated the DIRECT way, every mode's nine
// sin / cos pairs and cos(FTX t + TAT) at every cell (the form of the reference, Tutorials/HIT/NS_getForce.cpp:541-705, divergence-free
// branch), to put a number beside the separable kernel k_turb_force (iamr_amd/csrc/k_turb.hip).  Times it by HIP events on an n^3 box
// with one ghost layer and prints one JSON line.
//   hipcc -O3 --offload-arch=gfx950 tools/turb_direct.hip -Iinclude -Liamr_amd -liamrx -Wl,-rpath,'$ORIGIN/../iamr_amd' -o tools/_turb_direct
//   tools/_turb_direct [n = 256] [nmodes = 4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "iamrx.h"

#define CHECK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(_e), __LINE__); return 1; } } while (0)

__global__ void __launch_bounds__(256) k_direct(int M, const int* __restrict__ kxyz, const double* __restrict__ data, int n, double dx, double lo, double L,
                                                double time, double* __restrict__ out)
{
    const double TwoPi = 2.0 * 3.141592653589793238462643383279502884197;
    const int m1 = n + 2;
    const long total = (long)m1 * m1 * m1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int i = (int)(idx % m1) - 1, j = (int)((idx / m1) % m1) - 1, k = (int)(idx / ((long)m1 * m1)) - 1;
    const double x = lo + (i + 0.5) * dx, y = lo + (j + 0.5) * dx, z = lo + (k + 0.5) * dx;
    double f1 = 0, f2 = 0, f3 = 0;
    for (int m = 0; m < M; ++m) {
        const double* v = data + 17 * m;
        const int kx = kxyz[3 * m], ky = kxyz[3 * m + 1], kz = kxyz[3 * m + 2];
        const double xT = cos(v[0] * time + v[1]);
        const double FAX = v[5], FAY = v[6], FAZ = v[7];
        f1 += xT * (FAZ * TwoPi * (ky / L) * sin(TwoPi * kx * x / L + v[14]) * cos(TwoPi * ky * y / L + v[15]) * sin(TwoPi * kz * z / L + v[16])
                    - FAY * TwoPi * (kz / L) * sin(TwoPi * kx * x / L + v[11]) * sin(TwoPi * ky * y / L + v[12]) * cos(TwoPi * kz * z / L + v[13]));
        f2 += xT * (FAX * TwoPi * (kz / L) * sin(TwoPi * kx * x / L + v[8]) * sin(TwoPi * ky * y / L + v[9]) * cos(TwoPi * kz * z / L + v[10])
                    - FAZ * TwoPi * (kx / L) * cos(TwoPi * kx * x / L + v[14]) * sin(TwoPi * ky * y / L + v[15]) * sin(TwoPi * kz * z / L + v[16]));
        f3 += xT * (FAY * TwoPi * (kx / L) * cos(TwoPi * kx * x / L + v[11]) * sin(TwoPi * ky * y / L + v[12]) * sin(TwoPi * kz * z / L + v[13])
                    - FAX * TwoPi * (ky / L) * sin(TwoPi * kx * x / L + v[8]) * cos(TwoPi * ky * y / L + v[9]) * sin(TwoPi * kz * z / L + v[10]));
    }
    out[idx] = f1; out[idx + total] = f2; out[idx + 2 * total] = f3;
}

int main(int argc, char** argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 256, nmodes = argc > 2 ? atoi(argv[2]) : 4;
    if (n < 8 || n > 512) { fprintf(stderr, "n must be 8 .. 512\n"); return 2; }
    const double plo[3] = {-0.5, -0.5, -0.5}, phi[3] = {0.5, 0.5, 0.5};
    int M = 0;
    if (iamrx_host_turb_modes(plo, phi, nmodes, 0, 1, 0, &M, nullptr, nullptr)) { fprintf(stderr, "%s\n", iamrx_last_error()); return 1; }
    std::vector<int> k(3 * M);
    std::vector<double> d(17 * M);
    if (iamrx_host_turb_modes(plo, phi, nmodes, 0, 1, M, &M, k.data(), d.data())) { fprintf(stderr, "%s\n", iamrx_last_error()); return 1; }
    const long total = (long)(n + 2) * (n + 2) * (n + 2);
    int* dk; double *dd, *out;
    CHECK(hipMalloc(&dk, k.size() * sizeof(int))); CHECK(hipMalloc(&dd, d.size() * sizeof(double))); CHECK(hipMalloc(&out, 3 * total * sizeof(double)));
    CHECK(hipMemcpy(dk, k.data(), k.size() * sizeof(int), hipMemcpyHostToDevice)); CHECK(hipMemcpy(dd, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const dim3 grid((unsigned)((total + 255) / 256));
    std::vector<float> ms;
    for (int r = 0; r < 4; ++r) {              // the first launch loads the code object: not counted
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_direct, grid, dim3(256), 0, 0, M, dk, dd, n, 1.0 / n, -0.5, 1.0, 0.37, out);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float t = 0;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (r > 0) ms.push_back(t);
    }
    CHECK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    printf("{\"tool\": \"turb_direct\", \"n\": %d, \"modes\": %d, \"direct_ms_median\": %.4f, \"direct_ms_min\": %.4f}\n", n, M, ms[ms.size() / 2], ms[0]);
    (void)hipFree(dk); (void)hipFree(dd); (void)hipFree(out);
    return 0;
}
