// iamr_amd/csrc/k_turb.hip -- turbulent forcing of forced homogeneous isotropic turbulence: the table of low-wavenumber Fourier modes and
// the acceleration f(x, t) it defines on the cells and ghost cells of a level.
// Role: TurbulentForcing::init_turbulent_forcing (reference Tutorials/HIT/TurbulentForcing_def.H:21-366, generator Tutorials/HIT/depRand.cpp)
// and the forcing block of NavierStokesBase::getForce (Tutorials/HIT/NS_getForce.cpp:205-707, the form without USE_FAST_FORCE, :531-706).
//
// The reference keeps 17 arrays of 33^3 doubles indexed by the wavevector (most entries never written) and evaluates, per cell, every mode
// inside the sphere kappa <= kappaMax: 9 sin / cos pairs plus cos(FTX t + TAT) per mode in the divergence-free form.  Here the table is
// the compact list of the modes the reference's loops write, in their order, and the sum is evaluated through its separability: every
// factor sin / cos(2 pi k_d x_d / L_d + phase) depends on one coordinate and the mode only.
//   k_turb_factors  one small launch per evaluation: the sin and cos of every (mode, phase family, position) along the three coordinate
//                   lines of the level, each with the argument expression of the direct form; the z-line factors are folded with
//                   cos(FTX t + TAT), the amplitude and 2 pi k / L into the NT = 6 (3) per-mode z-factors of the terms below.
//   k_turb_force    level_tiling over the cells + ghost cells of every box (flat tile lists on levels of unequal boxes); a thread owns
//                   a fixed (i, j), loops the modes outermost and its TZ z-planes innermost with 3 x TZ accumulators in registers: per
//                   mode the NT x.y products once, then NT fused multiply-adds per plane whose z-factors are workgroup-uniform.
// Divergence-free form (:570-601), a in {X, Y, Z} the phase family FPa{X,Y,Z} of amplitude FAa, s / c = sin / cos along the named axis:
//   f1 += [sx^Z cy^Z] Z0 - [sx^Y sy^Y] Z1     Z0 = xT FAZ 2pi(ky/Ly) sz^Z    Z1 = xT FAY 2pi(kz/Lz) cz^Y
//   f2 += [sx^X sy^X] Z2 - [cx^Z sy^Z] Z3     Z2 = xT FAX 2pi(kz/Lz) cz^X    Z3 = xT FAZ 2pi(kx/Lx) sz^Z
//   f3 += [cx^Y sy^Y] Z4 - [sx^X cy^X] Z5     Z4 = xT FAY 2pi(kx/Lx) sz^Y    Z5 = xT FAX 2pi(ky/Ly) sz^X
// the other form (:603-615), one family FP{X,Y,Z}:  f1 += [cx sy] xT FAX sz,  f2 += [sx cy] xT FAY sz,  f3 += [sx sy] xT FAZ cz.
// Position: x_d = prob_lo_d + (i_d - domain_lo_d + 0.5) dx_d from the domain's index origin (the reference: from the box's low corner,
// equal up to rounding) -- the field does not depend on how the level is cut into boxes, and integer modes make it
// periodic, so ghost cells are evaluated at their own positions and no boundary fill follows.
#include "kernels.h"
#include "launch.h"
#include <cmath>
#include <random>

namespace iamrx {

namespace {
constexpr double TwoPi = 2.0 * 3.141592653589793238462643383279502884197;     // iamr_constants.H:9-10
constexpr double Pi = 3.141592653589793238462643383279502884197;
enum { FTX = 0, TAT, FPX, FPY, FPZ, FAX, FAY, FAZ, FPXX, FPXY, FPXZ, FPYX, FPYY, FPYZ, FPZX, FPZY, FPZZ, NDATA };
}  // namespace

// TurbulentForcing::init_turbulent_forcing with the constants it hard-codes (TurbulentForcing_def.H:55-56): spectrum_type 2,
// moderate_zero_modes 1, forcing_time_scale_min / max 0.5 / 1, force_scale 1, hack_lz 0
void turb_host_modes(const double problo[3], const double probhi[3], int nmodes, int mode_start, int div_free, std::vector<int>& kxyz,
                     std::vector<double>& data)
{
    const double Lx = probhi[0] - problo[0], Ly = probhi[1] - problo[1], Lz = probhi[2] - problo[2];     // :31-33
    if (nmodes < 1 || mode_start < 0) throw Error("iamrx turbulent forcing: turb.nmodes >= 1 and turb.mode_start >= 0 are required");
    if (!(Lx == Ly)) throw Error("iamrx turbulent forcing: the domain must have Lx == Ly (TurbulentForcing_def.H:34)");
    if (!(Lz >= Lx)) throw Error("iamrx turbulent forcing: the domain must have Lz >= Lx (only z may be the long direction, TurbulentForcing_def.H:30, 241)");
    const double Lmin = std::min(Lx, std::min(Ly, Lz));                        // :102-106
    const double kappaMax = ((double)nmodes) / Lmin + 1.0e-8;
    const int xstep = (int)(Lx / Lmin + 0.5), ystep = (int)(Ly / Lmin + 0.5), zstep = (int)(Lz / Lmin + 0.5);   // :135-137
    const int nxmodes = nmodes * (int)(0.5 + Lx / Lmin), nymodes = nmodes * (int)(0.5 + Ly / Lmin), nzmodes = nmodes * (int)(0.5 + Lz / Lmin);
    if ((long)nmodes * zstep > 32)
        throw Error("iamrx turbulent forcing: nmodes * zstep must be <= 32 (the reference's tables hold wavenumbers 0 .. 32, TurbulentForcing_params.H:19)");
    const double forcing_time_scale_min = 0.5, forcing_time_scale_max = 1.0;
    const double freqMin = 1.0 / forcing_time_scale_max, freqMax = 1.0 / forcing_time_scale_min, freqDiff = freqMax - freqMin;   // :117-119
    // DepRand::InitRandom(111397) (:131): MT19937 seeded by init_genrand (depRand.cpp:46-59) -- std::mt19937 is that generator and that
    // seeding; Random() = d_value(): the 32-bit draw times 1 / (2^32 - 1) (depRand.cpp:187-191)
    std::mt19937 gen(111397u);
    auto Random = [&gen]() { return (double)gen() * (1.0 / 4294967295.0); };
    kxyz.clear(); data.clear();
    auto mode = [&](int kx, int ky, int kz) {                                  // the body of both loops, :147-237 = :249-339
        const double kxd = (double)kx, kyd = (double)ky, kzd = (double)kz;
        const double kappa = std::sqrt((kxd * kxd) / (Lx * Lx) + (kyd * kyd) / (Ly * Ly) + (kzd * kzd) / (Lz * Lz));
        if (!(kappa <= kappaMax)) return;
        double v[NDATA];
        for (double& q : v) q = 0.0;
        v[FTX] = (freqMin + freqDiff * Random()) * TwoPi;
        v[TAT] = Random() * TwoPi;
        v[FPX] = Random() * TwoPi; v[FPY] = Random() * TwoPi; v[FPZ] = Random() * TwoPi;
        if (div_free) {                                                        // :159-169: XX YX ZX, XY YY ZY, XZ YZ ZZ (without: never written upstream, zero here)
            v[FPXX] = Random() * TwoPi; v[FPYX] = Random() * TwoPi; v[FPZX] = Random() * TwoPi;
            v[FPXY] = Random() * TwoPi; v[FPYY] = Random() * TwoPi; v[FPZY] = Random() * TwoPi;
            v[FPXZ] = Random() * TwoPi; v[FPYZ] = Random() * TwoPi; v[FPZZ] = Random() * TwoPi;
        }
        const double thetaTmp = Random() * TwoPi;                              // :171-183
        const double cosThetaTmp = std::cos(thetaTmp), sinThetaTmp = std::sin(thetaTmp);
        const double phiTmp = Random() * Pi;
        const double cosPhiTmp = std::cos(phiTmp), sinPhiTmp = std::sin(phiTmp);
        const double px = cosThetaTmp * sinPhiTmp, py = sinThetaTmp * sinPhiTmp, pz = cosPhiTmp;
        const double mp2 = px * px + py * py + pz * pz;
        if (!(kappa < 0.000001)) {                                             // the zero mode keeps its draws and a zero amplitude (:184-188)
            double Ekh = 1. / (kappa * kappa);                                 // spectrum_type 2
            if (div_free) Ekh /= kappa;
            if (kx == 0) Ekh /= 2.;                                            // moderate_zero_modes
            if (ky == 0) Ekh /= 2.;
            if (kz == 0) Ekh /= 2.;
            const double force_scale = 1.0;
            v[FAX] = force_scale * px * Ekh / mp2; v[FAY] = force_scale * py * Ekh / mp2; v[FAZ] = force_scale * pz * Ekh / mp2;
        }
        kxyz.push_back(kx); kxyz.push_back(ky); kxyz.push_back(kz);
        data.insert(data.end(), v, v + NDATA);
    };
    for (int kz = mode_start * zstep; kz <= nzmodes; kz += zstep)              // :142-146
        for (int ky = mode_start * ystep; ky <= nymodes; ky += ystep)
            for (int kx = mode_start * xstep; kx <= nxmodes; kx += xstep) mode(kx, ky, kz);
    for (int kz = 1; kz < zstep; kz++)                                         // the symmetry-breaking set of a domain long in z, :244-248
        for (int ky = mode_start; ky <= nymodes; ky += ystep)
            for (int kx = mode_start; kx <= nxmodes; kx += xstep) mode(kx, ky, kz);
}

TurbTable::~TurbTable()
{
    if (d_kxyz) Context::get().free(d_kxyz);
    if (d_data) Context::get().free(d_data);
}

TurbTableP turb_make_table(int M, const int* kxyz, const double* data, int div_free)
{
    if (M < 0 || (M > 0 && (!kxyz || !data))) throw Error("iamrx turbulent forcing: a mode table needs M >= 0, the wavevectors and the 17 values per mode");
    auto t = std::make_shared<TurbTable>();
    t->M = M; t->div_free = div_free != 0;
    t->kxyz.assign(kxyz, kxyz + 3 * (size_t)M);
    t->data.assign(data, data + NDATA * (size_t)M);
    return t;
}

TurbTableP turb_make_table(const Geometry& g, int nmodes, int mode_start, int div_free)
{
    std::vector<int> k;
    std::vector<double> d;
    turb_host_modes(g.problo, g.probhi, nmodes, mode_start, div_free, k, d);
    return turb_make_table((int)(k.size() / 3), k.data(), d.data(), div_free);
}

struct TurbLines {
    int lo[3], n[3];            // first index and number of positions of the x-, y- and z-line of the level
    int domlo[3];
    double problo[3], dx[3], L[3];
};

// thread (m, p): mode m, position p of the concatenated x-, y- and z-line
template <bool DIVFREE>
__global__ void __launch_bounds__(256) k_turb_factors(int M, const int* __restrict__ kxyz, const double* __restrict__ data, TurbLines ln, double time, int zpad,
                                                      double* __restrict__ FX, double* __restrict__ FY, double* __restrict__ FZ)
{
    constexpr int NF = DIVFREE ? 3 : 1, NQ = 2 * NF, NT = DIVFREE ? 6 : 3;
    const int ntot = ln.n[0] + ln.n[1] + ln.n[2];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * ntot) return;
    const int m = (int)(idx / ntot);
    int p = (int)(idx % ntot);
    const int d = p < ln.n[0] ? 0 : (p < ln.n[0] + ln.n[1] ? 1 : 2);
    if (d >= 1) p -= ln.n[0];
    if (d == 2) p -= ln.n[1];
    const double* v = data + (size_t)NDATA * m;
    const int kd = kxyz[3 * m + d];
    const double x = ln.problo[d] + ((double)(ln.lo[d] + p - ln.domlo[d]) + 0.5) * ln.dx[d];
    double s[NF], c[NF];
#pragma unroll
    for (int a = 0; a < NF; ++a) {
        const double ph = DIVFREE ? v[FPXX + 3 * a + d] : v[FPX + d];
        const double arg = TwoPi * (double)kd * x / ln.L[d] + ph;             // the argument expression of NS_getForce.cpp:574-615
        s[a] = sin(arg); c[a] = cos(arg);
    }
    if (d < 2) {
        double* F = (d == 0 ? FX : FY) + (size_t)m * NQ * ln.n[d] + p;
#pragma unroll
        for (int a = 0; a < NF; ++a) { F[(size_t)(2 * a) * ln.n[d]] = s[a]; F[(size_t)(2 * a + 1) * ln.n[d]] = c[a]; }
        return;
    }
    const double xT = cos(v[FTX] * time + v[TAT]);                             // :561
    double z[NT];
    if constexpr (DIVFREE) {
        const double wx = TwoPi * ((double)kxyz[3 * m] / ln.L[0]), wy = TwoPi * ((double)kxyz[3 * m + 1] / ln.L[1]), wz = TwoPi * ((double)kxyz[3 * m + 2] / ln.L[2]);
        enum { X = 0, Y = 1, Z = 2 };
        z[0] = xT * (v[FAZ] * wy) * s[Z];
        z[1] = xT * (v[FAY] * wz) * c[Y];
        z[2] = xT * (v[FAX] * wz) * c[X];
        z[3] = xT * (v[FAZ] * wx) * s[Z];
        z[4] = xT * (v[FAY] * wx) * s[Y];
        z[5] = xT * (v[FAX] * wy) * s[X];
    } else {
        z[0] = xT * v[FAX] * s[0];
        z[1] = xT * v[FAY] * s[0];
        z[2] = xT * v[FAZ] * c[0];
    }
    // a z-row holds n[2] + zpad positions: k_turb_force reads TZ consecutive ones from any plane of the line; the pad is zero
    const int nzp = ln.n[2] + zpad;
    double* F = FZ + (size_t)m * NT * nzp + p;
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        F[(size_t)q * nzp] = z[q];
        if (p == ln.n[2] - 1) for (int e = 1; e <= zpad; ++e) F[(size_t)q * nzp + e] = 0.0;
    }
}

template <bool DIVFREE, int TZ>
__global__ void __launch_bounds__(256) k_turb_force(Tiling t, const BoxD* __restrict__ boxes, int ng, const FabD* __restrict__ out, int ocomp, int M,
                                                    const double* __restrict__ FX, const double* __restrict__ FY, const double* __restrict__ FZ,
                                                    int ilo, int jlo, int klo, int nx, int ny, int nz)
{
    constexpr int NQ = DIVFREE ? 6 : 2, NT = DIVFREE ? 6 : 3;
    const int fab = tile_fab(t);
    const BoxD b = dev_grow_convert(boxes[fab], 0, 0, 0, ng);
    int i, j, k0, k1;
    if (!tile_ijk(t, b, i, j, k0, k1)) return;
    double a0[TZ], a1[TZ], a2[TZ];
#pragma unroll
    for (int p = 0; p < TZ; ++p) { a0[p] = 0.0; a1[p] = 0.0; a2[p] = 0.0; }
    const double* fx = FX + (i - ilo);
    const double* fy = FY + (j - jlo);
    // the z-planes of a workgroup are the same for all its threads: the z-factors are read through a wave-uniform index (scalar loads of
    // TZ consecutive doubles).  nz: the padded row length, so planes past the tile's last one read zeros (in bounds) and are not stored
    const double* fz = FZ + __builtin_amdgcn_readfirstlane(k0 - klo);
    for (int m = 0; m < M; ++m) {
        const double* gx = fx + (size_t)m * NQ * nx;
        const double* gy = fy + (size_t)m * NQ * ny;
        const double* gz = fz + (size_t)m * NT * nz;
        if constexpr (DIVFREE) {
            // rows: 0 s^X, 1 c^X, 2 s^Y, 3 c^Y, 4 s^Z, 5 c^Z
            const double sxX = gx[0], sxY = gx[2 * (size_t)nx], cxY = gx[3 * (size_t)nx], sxZ = gx[4 * (size_t)nx], cxZ = gx[5 * (size_t)nx];
            const double syX = gy[0], cyX = gy[(size_t)ny], syY = gy[2 * (size_t)ny], syZ = gy[4 * (size_t)ny], cyZ = gy[5 * (size_t)ny];
            const double P0 = sxZ * cyZ, P1 = sxY * syY, P2 = sxX * syX, P3 = cxZ * syZ, P4 = cxY * syY, P5 = sxX * cyX;
#pragma unroll
            for (int p = 0; p < TZ; ++p) {
                a0[p] = fma(P0, gz[p], a0[p]);
                a0[p] = fma(-P1, gz[(size_t)nz + p], a0[p]);
                a1[p] = fma(P2, gz[2 * (size_t)nz + p], a1[p]);
                a1[p] = fma(-P3, gz[3 * (size_t)nz + p], a1[p]);
                a2[p] = fma(P4, gz[4 * (size_t)nz + p], a2[p]);
                a2[p] = fma(-P5, gz[5 * (size_t)nz + p], a2[p]);
            }
        } else {
            const double sx = gx[0], cx = gx[(size_t)nx], sy = gy[0], cy = gy[(size_t)ny];
            const double P0 = cx * sy, P1 = sx * cy, P2 = sx * sy;
#pragma unroll
            for (int p = 0; p < TZ; ++p) {
                a0[p] = fma(P0, gz[p], a0[p]);
                a1[p] = fma(P1, gz[(size_t)nz + p], a1[p]);
                a2[p] = fma(P2, gz[2 * (size_t)nz + p], a2[p]);
            }
        }
    }
    const FabD o = out[fab];
#pragma unroll
    for (int p = 0; p < TZ; ++p)
        if (k0 + p <= k1) { o(i, j, k0 + p, ocomp) = a0[p]; o(i, j, k0 + p, ocomp + 1) = a1[p]; o(i, j, k0 + p, ocomp + 2) = a2[p]; }
}

void turb_force(const Geometry& g, const TurbTable& tt, double time, MultiFab& out, int ocomp)
{
    IAMRX_ASSERT(out.type.cell() && ocomp >= 0 && ocomp + 3 <= out.ncomp);
    if (out.nlocal() == 0) return;
    auto& ctx = Context::get();
    const Layout& l = *out.layout;
    const int ng = out.ngrow, M = tt.M;
    if (M == 0) { out.setVal(0.0, ocomp, 3, ng); return; }
    if (!tt.d_kxyz) {                                   // the device copy of the table, made at the first evaluation
        tt.d_kxyz = (int*)ctx.alloc(tt.kxyz.size() * sizeof(int));
        tt.d_data = (double*)ctx.alloc(tt.data.size() * sizeof(double));
        ctx.upload_async(tt.d_kxyz, tt.kxyz.data(), tt.kxyz.size() * sizeof(int));
        ctx.upload_async(tt.d_data, tt.data.data(), tt.data.size() * sizeof(double));
    }
    TurbLines ln;
    for (int d = 0; d < 3; ++d) {
        int lo = l.lbox(0).lo[d], hi = l.lbox(0).hi[d];
        for (int q = 1; q < l.nlocal(); ++q) { lo = std::min(lo, l.lbox(q).lo[d]); hi = std::max(hi, l.lbox(q).hi[d]); }
        ln.lo[d] = lo - ng; ln.n[d] = hi - lo + 1 + 2 * ng;
        ln.domlo[d] = g.domain.lo[d]; ln.problo[d] = g.problo[d]; ln.dx[d] = g.dx[d]; ln.L[d] = g.probhi[d] - g.problo[d];
    }
    const bool df = tt.div_free != 0;
    const int NQ = df ? 6 : 2, NT = df ? 6 : 3;
    constexpr int TZ = 8;
    const int nzp = ln.n[2] + TZ - 1;                  // padded z-rows (k_turb_factors)
    const size_t nfx = (size_t)M * NQ * ln.n[0], nfy = (size_t)M * NQ * ln.n[1], nfz = (size_t)M * NT * nzp;
    double* ws = (double*)ctx.alloc((nfx + nfy + nfz) * sizeof(double));
    double *FX = ws, *FY = ws + nfx, *FZ = FY + nfy;
    const long nthr = (long)M * (ln.n[0] + ln.n[1] + ln.n[2]);
    const dim3 fgrid((unsigned)((nthr + 255) / 256));
    if (df) hipLaunchKernelGGL(k_turb_factors<true>, fgrid, dim3(256), 0, ctx.stream, M, tt.d_kxyz, tt.d_data, ln, time, TZ - 1, FX, FY, FZ);
    else hipLaunchKernelGGL(k_turb_factors<false>, fgrid, dim3(256), 0, ctx.stream, M, tt.d_kxyz, tt.d_data, ln, time, TZ - 1, FX, FY, FZ);
    const Tiling t = level_tiling(l, cell_type(), ng, TZ, true);
    IAMRX_ASSERT(t.tz <= TZ);
    if (df)
        hipLaunchKernelGGL((k_turb_force<true, TZ>), t.grid(), Tiling::block(), 0, ctx.stream, t, l.d_boxes, ng, out.d_tab, ocomp, M, FX, FY, FZ, ln.lo[0],
                           ln.lo[1], ln.lo[2], ln.n[0], ln.n[1], nzp);
    else
        hipLaunchKernelGGL((k_turb_force<false, TZ>), t.grid(), Tiling::block(), 0, ctx.stream, t, l.d_boxes, ng, out.d_tab, ocomp, M, FX, FY, FZ, ln.lo[0],
                           ln.lo[1], ln.lo[2], ln.n[0], ln.n[1], nzp);
    ctx.free(ws);                                       // the allocator's cache is ordered by the stream: the block is reused by later launches only
}

}  // namespace iamrx
