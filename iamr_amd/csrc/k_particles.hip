// iamr_amd/csrc/k_particles.hip -- tracer particles: the container of particles.h and its kernels (advect with the MAC velocity,
// redistribute over levels and boxes, the two particle counts, cell-centred state sampled at the particles and the timestamp files written
// from it).  UNPINNED against AMReX, whose source is not in the reference tree; the scheme as implemented is
// restated in numpy by tests/particles_numpy.py and tests/timestamp_numpy.py.
#include "particles.h"
#include "launch.h"
#include "operators.h"
#include <algorithm>
#include <numeric>
#include <cmath>
#include <cstring>
#include <cstdio>

namespace iamrx {

namespace {

constexpr int PB = 256;   // threads per workgroup: one particle each

// ---- placement ------------------------------------------------------------------------------------------------------------------------
// periodic wrap of one coordinate into [lo, hi): x - L floor((x - lo) / L), then the two roundings that can leave it on or outside an end
__device__ __forceinline__ double wrap_coord(double x, double lo, double hi)
{
    const double L = hi - lo;
    x = x - L * floor((x - lo) / L);
    if (x >= hi) x = lo;
    if (x < lo) x = lo;
    return x;
}

// cell of the level that holds x (inside the domain), relative to the domain's low corner
__device__ __forceinline__ void cell_of(const PHierD& H, int L, const double x[3], int c[3])
{
    const PLevelD& lv = H.L[L];
    for (int e = 0; e < 3; ++e) {
        const double l = floor((x[e] - H.plo[e]) / lv.dx[e]);
        int i = (int)fmin(fmax(l, 0.0), (double)(lv.n[e] - 1));
        c[e] = i;
    }
}

__device__ __forceinline__ int box_at(const PLevelD& lv, int c0, int c1, int c2)
{
    const int g = lv.gran;
    return lv.tab[(c0 / g) + lv.tn[0] * ((c1 / g) + lv.tn[1] * (c2 / g))];
}

// ctr[k] += 1 for every active lane of the wavefront, one atomic per distinct k in the wavefront: the lanes that share a k elect a leader,
// which adds their number; returns the lane's slot (the counter before the add + the lane's rank among its peers).  Particles arrive
// grouped by box, so a wavefront holds one or two distinct keys -- a plain atomicAdd per lane sends 64 adds to ONE address, and a level
// of few boxes then runs at the rate of serialised atomics (measured: 6 ms per redistribution of 262 144 particles in one box).
// To be called where the wavefront's remaining lanes are convergent.
__device__ __forceinline__ int wave_add_one(int* ctr, int k)
{
    const int lane = __lane_id();
    unsigned long long todo = __ballot(1);
    int slot = 0;
    while (todo) {                                             // wave-uniform: every ballot below is
        const int leader = __ffsll((long long)todo) - 1;
        const int lk = __shfl(k, leader);
        const bool mine = k == lk && ((todo >> lane) & 1ull);
        const unsigned long long same = __ballot(mine);
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctr[lk], (int)__popcll(same));
        base = __shfl(base, leader);
        if (mine) slot = base + (int)__popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return slot;
}

// the new group of particle p (written to key[p]; -1: leaves) -> the counter it adds to.  MR (several ranks): the box found is one of the
// level's global list; a particle whose box rank q owns gets key -2 - q, its level and global box go to dlev / dbox (the record that
// travels), and it counts under nkeys + 3 + q
template <bool MR>
__device__ int place_one(const PHierD& H, const PArrays& a, long p, int lev_min, int lev_max, int ngrow, int nkeys, int* __restrict__ key, int me,
                         int* __restrict__ dlev, int* __restrict__ dbox)
{
    double x[3] = {a.x[0][p], a.x[1][p], a.x[2][p]};
    bool out = false;
    for (int e = 0; e < 3; ++e) {
        if (H.per[e]) x[e] = wrap_coord(x[e], H.plo[e], H.phi[e]);
        if (!(x[e] >= H.plo[e] && x[e] < H.phi[e])) out = true;          // also a NaN
    }
    if (out) { key[p] = -1; return nkeys; }
    int found = -1, flev = lev_min;                         // found: index in the global box list of level flev
    for (int L = lev_max; L >= lev_min && found < 0; --L) {
        int c[3];
        cell_of(H, L, x, c);
        const int b = box_at(H.L[L], c[0], c[1], c[2]);
        if (b >= 0) { found = b; flev = L; }
    }
    if (found < 0 && ngrow > 0) {
        // a box of lev_min whose ngrow-grown region holds the cell, or a periodic image of it: the lowest box index.  Every such box
        // contains one of the 26 cells c + ngrow * s, s in {-1, 0, 1}^3 (boxes are at least ngrow cells long: checked by the host)
        const PLevelD& lv = H.L[lev_min];
        int c[3];
        cell_of(H, lev_min, x, c);
        int best = -1, best_ns = 0, bs[3] = {0, 0, 0};      // lowest box index; of its images the one with the fewest shifts (the cell itself first)
        for (int s2 = -1; s2 <= 1; ++s2)
            for (int s1 = -1; s1 <= 1; ++s1)
                for (int s0 = -1; s0 <= 1; ++s0) {
                    const int s[3] = {s0, s1, s2};
                    int q[3], sh[3];
                    bool ok = true;
                    for (int e = 0; e < 3; ++e) {
                        q[e] = c[e] + ngrow * s[e];
                        sh[e] = 0;
                        if (q[e] < 0) { if (H.per[e]) { q[e] += lv.n[e]; sh[e] = 1; } else ok = false; }
                        else if (q[e] >= lv.n[e]) { if (H.per[e]) { q[e] -= lv.n[e]; sh[e] = -1; } else ok = false; }
                        if (q[e] < 0 || q[e] >= lv.n[e]) ok = false;
                    }
                    if (!ok) continue;
                    const int b = box_at(lv, q[0], q[1], q[2]);
                    const int ns = (sh[0] != 0) + (sh[1] != 0) + (sh[2] != 0);
                    if (b < 0 || (best >= 0 && (b > best || (b == best && ns >= best_ns)))) continue;
                    const BoxD bx = lv.gboxes[b];
                    bool in = true;
                    for (int e = 0; e < 3; ++e) {
                        const int ci = c[e] + sh[e] * lv.n[e] + lv.dlo[e];
                        in = in && ci >= bx.lo[e] - ngrow && ci <= bx.hi[e] + ngrow;
                    }
                    if (in) { best = b; best_ns = ns; bs[0] = sh[0]; bs[1] = sh[1]; bs[2] = sh[2]; }
                }
        if (best >= 0) {
            found = best;
            for (int e = 0; e < 3; ++e) if (bs[e] != 0) x[e] = x[e] + (double)bs[e] * (H.phi[e] - H.plo[e]);    // the image next to the box
        }
    }
    for (int e = 0; e < 3; ++e) a.x[e][p] = x[e];
    if (found < 0) { key[p] = -1; return nkeys + 1; }
    if (MR) {
        const int q = H.L[flev].owner[found];
        if (q != me) { key[p] = -2 - q; dlev[p] = flev; dbox[p] = found; return nkeys + 3 + q; }
        found = H.L[flev].lidx[found];
    }
    found += H.L[flev].key0;
    key[p] = found;
    return found;
}


// key: group of the particle after the redistribution (level's key0 + box), -1 removed.  counts: [nkeys] group sizes, then
// [nkeys] removed beyond a non-periodic face, [nkeys + 1] could not be placed, [nkeys + 2] invalid (id <= 0, dropped); MR: then
// [nkeys + 3 + q] leaves for rank q
template <bool MR>
__global__ void __launch_bounds__(PB) k_part_place(PHierD H, PArrays a, long n, int lev_min, int lev_max, int ngrow, int nkeys, int* __restrict__ key,
                                                   int* __restrict__ counts, int me, int* __restrict__ dlev, int* __restrict__ dbox)
{
    const long p = (long)blockIdx.x * PB + threadIdx.x;
    if (p >= n) return;
    // cidx: the counter the particle adds to -- its group, or one of the three after the groups; one aggregated add at the end
    int cidx;
    const int l0 = a.lev[p];
    if (a.id[p] <= 0) { key[p] = -1; cidx = nkeys + 2; }
    else if (l0 < lev_min) { cidx = H.L[l0].key0 + a.box[p]; key[p] = cidx; }      // not this call's business
    else cidx = place_one<MR>(H, a, p, lev_min, lev_max, ngrow, nkeys, key, me, dlev, dbox);
    wave_add_one(counts, cidx);
}

// exclusive prefix sum of counts[0 .. n) into offs[0 .. n), one workgroup; cursor[0 .. n) = 0
__global__ void __launch_bounds__(PB) k_part_prefix(int n, const int* __restrict__ counts, int* __restrict__ offs, int* __restrict__ cursor)
{
    __shared__ int part[PB];
    const int t = threadIdx.x, chunk = (n + PB - 1) / PB;
    const int q0 = t * chunk, q1 = min(n, q0 + chunk);
    int s = 0;
    for (int q = q0; q < q1; ++q) s += counts[q];
    part[t] = s;
    __syncthreads();
    int base = 0;
    for (int u = 0; u < t; ++u) base += part[u];
    for (int q = q0; q < q1; ++q) { offs[q] = base; base += counts[q]; cursor[q] = 0; }
}

__global__ void __launch_bounds__(PB) k_part_scatter(PHierD H, PArrays a, PArrays o, long n, const int* __restrict__ key, const int* __restrict__ offs,
                                                     int* __restrict__ cursor)
{
    const long p = (long)blockIdx.x * PB + threadIdx.x;
    if (p >= n) return;
    const int k = key[p];
    if (k < 0) return;
    const long q = (long)offs[k] + wave_add_one(cursor, k);
    int L = 0;
    while (L + 1 < H.nlev && k >= H.L[L + 1].key0) ++L;
    for (int e = 0; e < 3; ++e) { o.x[e][q] = a.x[e][p]; o.r[e][q] = a.r[e][p]; }
    o.id[q] = a.id[p]; o.cpu[q] = a.cpu[p];
    o.lev[q] = L; o.box[q] = k - H.L[L].key0;
}

// ---- migration (several ranks) ----------------------------------------------------------------------------------------------------------
// A record is NREC doubles: x, y, z, r0, r1, r2, id, cpu, level, global box (32-bit integers are exact as doubles).  The buffer for / from
// one peer holds its cnt records field by field (field f of record i at f * cnt + i), the peers' parts one after another in rank order.
constexpr int NREC = 10;

// the leavers (key <= -2) into the send buffer; sendcnt[q]: how many leave for rank q (the place kernel's counters), scursor[q] = 0
__global__ void __launch_bounds__(PB) k_part_pack(PArrays a, long n, const int* __restrict__ key, const int* __restrict__ dlev, const int* __restrict__ dbox,
                                                  const int* __restrict__ sendcnt, int* __restrict__ scursor, double* __restrict__ buf)
{
    const long p = (long)blockIdx.x * PB + threadIdx.x;
    if (p >= n) return;
    const int k = key[p];
    if (k > -2) return;
    const int q = -2 - k;
    const int slot = wave_add_one(scursor, q);
    long start = 0;
    for (int u = 0; u < q; ++u) start += sendcnt[u];
    const long cnt = sendcnt[q];
    double* b = buf + start * NREC + slot;
    for (int e = 0; e < 3; ++e) { b[e * cnt] = a.x[e][p]; b[(3 + e) * cnt] = a.r[e][p]; }
    b[6 * cnt] = (double)a.id[p]; b[7 * cnt] = (double)a.cpu[p];
    b[8 * cnt] = (double)dlev[p]; b[9 * cnt] = (double)dbox[p];
}

// arrival j of nrecv -> the part of the receive buffer it lies in (rstart[q]: first arrival from rank q, rstart[nranks] = nrecv) and its
// index there
__device__ __forceinline__ const double* arrival(const double* __restrict__ rbuf, const int* __restrict__ rstart, int nranks, long j, long& cnt)
{
    int q = 0;
    while (q + 1 < nranks && j >= rstart[q + 1]) ++q;
    cnt = rstart[q + 1] - rstart[q];
    return rbuf + (long)rstart[q] * NREC + (j - rstart[q]);
}

// files the arrivals: akey[j] = the group of arrival j, from the level and the global box its sender found (nothing is placed a second
// time: the sender may have moved the particle to the periodic image next to its box); counts[group] += 1.  A record that names no box of
// this rank counts under nkeys + 1 and gets key -1
__global__ void __launch_bounds__(PB) k_part_file(PHierD H, const double* __restrict__ rbuf, const int* __restrict__ rstart, int nranks, long nrecv, int me,
                                                  int nkeys, int* __restrict__ akey, int* __restrict__ counts)
{
    const long j = (long)blockIdx.x * PB + threadIdx.x;
    if (j >= nrecv) return;
    long cnt;
    const double* b = arrival(rbuf, rstart, nranks, j, cnt);
    const int L = (int)b[8 * cnt], gb = (int)b[9 * cnt];
    int k = -1;
    if (L >= 0 && L < H.nlev && gb >= 0 && gb < H.L[L].ngbox && H.L[L].owner[gb] == me) k = H.L[L].key0 + H.L[L].lidx[gb];
    akey[j] = k;
    wave_add_one(counts, k < 0 ? nkeys + 1 : k);
}

// the one scatter of a redistribution over ranks: threads 0 .. n - 1 the particles held (leavers and removed ones have a negative key),
// n .. n + nrecv - 1 the arrivals
__global__ void __launch_bounds__(PB) k_part_scatter_ranks(PHierD H, PArrays a, PArrays o, long n, const int* __restrict__ key, const double* __restrict__ rbuf,
                                                           const int* __restrict__ rstart, int nranks, long nrecv, const int* __restrict__ akey,
                                                           const int* __restrict__ offs, int* __restrict__ cursor)
{
    const long t = (long)blockIdx.x * PB + threadIdx.x;
    if (t >= n + nrecv) return;
    const int k = t < n ? key[t] : akey[t - n];
    if (k < 0) return;
    const long q = (long)offs[k] + wave_add_one(cursor, k);
    int L = 0;
    while (L + 1 < H.nlev && k >= H.L[L + 1].key0) ++L;
    if (t < n) {
        for (int e = 0; e < 3; ++e) { o.x[e][q] = a.x[e][t]; o.r[e][q] = a.r[e][t]; }
        o.id[q] = a.id[t]; o.cpu[q] = a.cpu[t];
    } else {
        long cnt;
        const double* b = arrival(rbuf, rstart, nranks, t - n, cnt);
        for (int e = 0; e < 3; ++e) { o.x[e][q] = b[e * cnt]; o.r[e][q] = b[(3 + e) * cnt]; }
        o.id[q] = (int)b[6 * cnt]; o.cpu[q] = (int)b[7 * cnt];
    }
    o.lev[q] = L; o.box[q] = k - H.L[L].key0;
}

// ---- advect ---------------------------------------------------------------------------------------------------------------------------
struct AdvGeom {
    double plo[3], dx[3];
    int dlo[3], dhi[3], per[3];
};

// trilinear interpolation of the face array of component D at x.  Stencil indices are clamped to the faces / cells of the domain at
// non-periodic faces (the library forms no BC-filled ghost faces: a stated deviation), and to the array:
// nothing is ever read outside the FAB whatever the position is
template <int D>
__device__ __forceinline__ double interp_face(const FabD& F, const AdvGeom& G, const double x[3])
{
    int i0[3], i1[3];
    double w[3];
    for (int e = 0; e < 3; ++e) {
        double l = (x[e] - G.plo[e]) / G.dx[e] - (e == D ? 0.0 : 0.5);
        l = fmin(fmax(l, -1.0e9), 1.0e9);                      // (a NaN takes the lower bound)
        const double fl = floor(l);
        w[e] = l - fl;
        int a = (int)fl + G.dlo[e], b = a + 1;
        if (!G.per[e]) {
            const int lo = G.dlo[e], hi = G.dhi[e] + (e == D ? 1 : 0);
            a = min(max(a, lo), hi); b = min(max(b, lo), hi);
        }
        const int flo = F.lo[e], fhi = F.lo[e] + F.n[e] - 1;
        i0[e] = min(max(a, flo), fhi); i1[e] = min(max(b, flo), fhi);
    }
    const double f000 = F(i0[0], i0[1], i0[2]), f100 = F(i1[0], i0[1], i0[2]), f010 = F(i0[0], i1[1], i0[2]), f110 = F(i1[0], i1[1], i0[2]);
    const double f001 = F(i0[0], i0[1], i1[2]), f101 = F(i1[0], i0[1], i1[2]), f011 = F(i0[0], i1[1], i1[2]), f111 = F(i1[0], i1[1], i1[2]);
    const double wx = w[0], wy = w[1], wz = w[2];
    // a + w (b - a): a uniform field is reproduced to the bit, whatever the weights
    const double a00 = f000 + wx * (f100 - f000), a10 = f010 + wx * (f110 - f010), a01 = f001 + wx * (f101 - f001), a11 = f011 + wx * (f111 - f011);
    const double b0 = a00 + wy * (a10 - a00), b1 = a01 + wy * (a11 - a01);
    return b0 + wz * (b1 - b0);
}

// PASS 1: r = x; x += dt/2 v(x).   PASS 2: x = r + dt v(x); r = v.   Particles p0 .. p0 + n - 1 (one level), one thread each
template <int PASS>
__global__ void __launch_bounds__(PB) k_part_advect(AdvGeom G, PArrays a, long p0, long n, const FabD* __restrict__ ux, const FabD* __restrict__ uy,
                                                    const FabD* __restrict__ uz, int nfab, double dt, int fixed_dir)
{
    const long t = (long)blockIdx.x * PB + threadIdx.x;
    if (t >= n) return;
    const long p = p0 + t;
    if (a.id[p] <= 0) return;
    const int f = a.box[p];
    if (f < 0 || f >= nfab) return;
    const double x[3] = {a.x[0][p], a.x[1][p], a.x[2][p]};
    const FabD U = ux[f], V = uy[f], W = uz[f];
    double v[3];
    v[0] = interp_face<0>(U, G, x);
    v[1] = interp_face<1>(V, G, x);
    v[2] = interp_face<2>(W, G, x);
    if (fixed_dir >= 0) v[fixed_dir] = 0.0;
    if (PASS == 1) {
        for (int e = 0; e < 3; ++e) { a.r[e][p] = x[e]; a.x[e][p] = x[e] + (0.5 * dt) * v[e]; }
    } else {
        for (int e = 0; e < 3; ++e) { a.x[e][p] = a.r[e][p] + dt * v[e]; a.r[e][p] = v[e]; }
    }
}

// ---- sample -----------------------------------------------------------------------------------------------------------------------------
// Cell-centred components at the particles: AMReX's cic_interpolate for cell data as the timestamp files use it (AMReX's source is not in
// the reference tree: UNPINNED like the rest of the container; tests/timestamp_numpy.py restates these expressions in this order).
struct SampleGeom {
    double plo[3], dx[3];
    int dlo[3];
};
struct SampleComps {
    int n;
    int c[Particles::MAX_SAMPLE];
};

// out[m * n + t] = component C.c[m] of the particle's box FAB, trilinear between the cell centres around particle p0 + t.  Per direction
// l = (x - plo) / dx - 0.5, i = floor(l), w = l - i, cells i and i + 1, clamped to the FAB's own index range ONLY: the array arrives
// FillPatched and its ghost cells hold the boundary values, so there is no clamp to the domain (unlike interp_face).  Nothing is read
// outside the array whatever the position is (a NaN takes the lower bound, as in interp_face).  The stencil and the weights are formed
// once per particle; a component costs its eight loads.  Particles with id <= 0 are skipped (the caller zeroed `out`)
__global__ void __launch_bounds__(PB) k_part_sample(SampleGeom G, PArrays a, long p0, long n, const FabD* __restrict__ tab, int nfab, SampleComps C,
                                                    double* __restrict__ out)
{
    const long t = (long)blockIdx.x * PB + threadIdx.x;
    if (t >= n) return;
    const long p = p0 + t;
    if (a.id[p] <= 0) return;
    const int f = a.box[p];
    if (f < 0 || f >= nfab) return;
    const FabD F = tab[f];
    const double x[3] = {a.x[0][p], a.x[1][p], a.x[2][p]};
    int i0[3], i1[3];
    double w[3];
    for (int e = 0; e < 3; ++e) {
        double l = (x[e] - G.plo[e]) / G.dx[e] - 0.5;
        l = fmin(fmax(l, -1.0e9), 1.0e9);                      // (a NaN takes the lower bound)
        const double fl = floor(l);
        w[e] = l - fl;
        const int ia = (int)fl + G.dlo[e], ib = ia + 1;
        const int flo = F.lo[e], fhi = F.lo[e] + F.n[e] - 1;
        i0[e] = min(max(ia, flo), fhi); i1[e] = min(max(ib, flo), fhi);
    }
    const long o000 = F.off(i0[0], i0[1], i0[2]), o100 = F.off(i1[0], i0[1], i0[2]), o010 = F.off(i0[0], i1[1], i0[2]), o110 = F.off(i1[0], i1[1], i0[2]);
    const long o001 = F.off(i0[0], i0[1], i1[2]), o101 = F.off(i1[0], i0[1], i1[2]), o011 = F.off(i0[0], i1[1], i1[2]), o111 = F.off(i1[0], i1[1], i1[2]);
    const double wx = w[0], wy = w[1], wz = w[2];
    for (int m = 0; m < C.n; ++m) {
        const auto* q = F.gp() + F.cs * C.c[m];
        const double f000 = q[o000], f100 = q[o100], f010 = q[o010], f110 = q[o110], f001 = q[o001], f101 = q[o101], f011 = q[o011], f111 = q[o111];
        // a + w (b - a): a uniform field is reproduced to the bit, whatever the weights
        const double a00 = f000 + wx * (f100 - f000), a10 = f010 + wx * (f110 - f010), a01 = f001 + wx * (f101 - f001), a11 = f011 + wx * (f111 - f011);
        const double b0 = a00 + wy * (a10 - a00), b1 = a01 + wy * (a11 - a01);
        out[(long)m * n + t] = b0 + wz * (b1 - b0);
    }
}

// ---- counts ---------------------------------------------------------------------------------------------------------------------------
// out(cell) += 1 for every particle of the levels lev .. lev_hi that sits in a valid cell of its own box: on level `lev` its cell, on a
// finer level that cell coarsened onto `lev` (NavierStokesBase::ParticleDerive, NavierStokesBase.cpp:3996-4048), where `lev` has a box
__global__ void __launch_bounds__(PB) k_part_count(PHierD H, PArrays a, long p0, long n, int lev, const FabD* __restrict__ out, int ocomp)
{
    const long t = (long)blockIdx.x * PB + threadIdx.x;
    if (t >= n) return;
    const long p = p0 + t;
    if (a.id[p] <= 0) return;
    const int L = a.lev[p];
    const PLevelD& lv = H.L[L];
    const double x[3] = {a.x[0][p], a.x[1][p], a.x[2][p]};
    int c[3];
    for (int e = 0; e < 3; ++e) {                              // no clamp: a particle outside the domain (an image) is in no valid cell
        const double l = fmin(fmax(floor((x[e] - H.plo[e]) / lv.dx[e]), -1.0), (double)lv.n[e]);
        c[e] = (int)l;
        if (c[e] < 0 || c[e] >= lv.n[e]) return;
    }
    const BoxD own = lv.boxes[a.box[p]];
    for (int e = 0; e < 3; ++e) if (c[e] + lv.dlo[e] < own.lo[e] || c[e] + lv.dlo[e] > own.hi[e]) return;
    int b = a.box[p];
    if (L > lev) {
        const PLevelD& cv = H.L[lev];
        for (int e = 0; e < 3; ++e) c[e] = (c[e] * cv.n[e]) / lv.n[e];      // n_fine = trr n_crse: the coarsening by trr
        b = box_at(cv, c[0], c[1], c[2]);
        if (b < 0) return;
    }
    const PLevelD& ov = H.L[lev];
    const FabD o = out[b];
    atomicAdd(&o.p[o.off(c[0] + ov.dlo[0], c[1] + ov.dlo[1], c[2] + ov.dlo[2]) + o.cs * ocomp], 1.0);
}

// after the levels changed: particles of the first `keep` levels (whose boxes stayed) keep their place, the others wait on the last kept
// level (box 0) for the redistribution that follows
__global__ void __launch_bounds__(PB) k_part_relevel(PArrays a, long n, int keep)
{
    const long p = (long)blockIdx.x * PB + threadIdx.x;
    if (p >= n) return;
    if (a.lev[p] >= keep) { a.lev[p] = keep > 0 ? keep - 1 : 0; a.box[p] = 0; }
}

inline unsigned nblocks(long n) { return (unsigned)((n + PB - 1) / PB); }

}  // namespace

// ---- container ------------------------------------------------------------------------------------------------------------------------
Particles::Particles(const std::vector<Geometry>& geoms, const std::vector<LayoutP>& layouts, int ratio) { define(geoms, layouts, ratio); }

Particles::~Particles()
{
    free_tables();
    if (m_block) Context::get().free(m_block);
}

void Particles::free_tables()
{
    for (int* t : m_tabs) if (t) (void)hipFree(t);
    m_tabs.clear();
}

void Particles::carve(PArrays& a, void* block, long cap)
{
    double* d = (double*)block;
    for (int e = 0; e < 3; ++e) { a.x[e] = d + (size_t)e * cap; a.r[e] = d + (size_t)(3 + e) * cap; }
    int* i = (int*)(d + (size_t)6 * cap);
    a.id = i; a.cpu = i + cap; a.lev = i + 2 * (size_t)cap; a.box = i + 3 * (size_t)cap;
}

static size_t block_bytes(long cap) { return (size_t)cap * (6 * sizeof(double) + 4 * sizeof(int)); }

void Particles::reserve(long cap)
{
    if (cap <= m_cap) return;
    auto& ctx = Context::get();
    cap = std::max(cap, std::max(1024L, 2 * m_cap));
    void* nb = ctx.alloc(block_bytes(cap));
    PArrays na;
    carve(na, nb, cap);
    if (m_np > 0) {
        for (int e = 0; e < 3; ++e) {
            IAMRX_HIP_CHECK(hipMemcpyAsync(na.x[e], m_a.x[e], m_np * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
            IAMRX_HIP_CHECK(hipMemcpyAsync(na.r[e], m_a.r[e], m_np * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
        }
        IAMRX_HIP_CHECK(hipMemcpyAsync(na.id, m_a.id, m_np * sizeof(int), hipMemcpyDeviceToDevice, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(na.cpu, m_a.cpu, m_np * sizeof(int), hipMemcpyDeviceToDevice, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(na.lev, m_a.lev, m_np * sizeof(int), hipMemcpyDeviceToDevice, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(na.box, m_a.box, m_np * sizeof(int), hipMemcpyDeviceToDevice, ctx.stream));
    }
    if (m_block) ctx.free(m_block);
    m_block = nb; m_a = na; m_cap = cap;
}

void Particles::define(const std::vector<Geometry>& geoms, const std::vector<LayoutP>& layouts, int ratio)
{
    auto& ctx = Context::get();
    const bool ranks = ctx.comm->nranks > 1;
    const int nl = (int)layouts.size();
    if (nl < 1 || nl > PHierD::MAXLEV || geoms.size() != layouts.size()) throw Error("iamrx Particles: 1 .. 8 levels, one geometry per level");
    if (nl > 1 && ratio < 2) throw Error("iamrx Particles: bad refinement ratio");
    for (int l = 1; l < nl; ++l)
        for (int e = 0; e < 3; ++e)
            if (geoms[l].domain.len(e) != ratio * geoms[l - 1].domain.len(e) || geoms[l].domain.lo[e] != ratio * geoms[l - 1].domain.lo[e])
                throw Error("iamrx Particles: the level domains are not refinements of one another");
    ctx.sync();                                               // kernels in flight may read the tables that go
    free_tables();
    int keep = 0;                                             // leading levels whose boxes stay
    while (keep < nl && keep < (int)m_layouts.size() && m_layouts[keep]->id == layouts[keep]->id) ++keep;
    m_geoms = geoms; m_layouts = layouts; m_ratio = ratio;
    m_h.nlev = nl;
    for (int e = 0; e < 3; ++e) { m_h.plo[e] = geoms[0].problo[e]; m_h.phi[e] = geoms[0].probhi[e]; m_h.per[e] = geoms[0].periodic[e]; }
    int key0 = 0;
    for (int l = 0; l < nl; ++l) {
        const Layout& lay = *layouts[l];
        const Geometry& g = geoms[l];
        PLevelD& lv = m_h.L[l];
        int gr = 0;
        for (int e = 0; e < 3; ++e) gr = std::gcd(gr, g.domain.len(e));
        const int nb = (int)lay.boxes.size();                 // the global list: what is built here is the same on every rank
        for (int q = 0; q < nb; ++q)
            for (int e = 0; e < 3; ++e) { gr = std::gcd(gr, lay.boxes[q].lo[e] - g.domain.lo[e]); gr = std::gcd(gr, lay.boxes[q].len(e)); }
        gr = std::max(gr, 1);
        lv.gran = gr;
        size_t nt = 1;
        for (int e = 0; e < 3; ++e) { lv.dlo[e] = g.domain.lo[e]; lv.n[e] = g.domain.len(e); lv.tn[e] = lv.n[e] / gr; lv.dx[e] = g.dx[e]; nt *= (size_t)lv.tn[e]; }
        std::vector<int> tab(nt, -1);
        for (int q = 0; q < nb; ++q) {
            const BoxD& b = lay.boxes[q];
            for (int e = 0; e < 3; ++e)
                if (b.lo[e] < g.domain.lo[e] || b.hi[e] > g.domain.hi[e]) throw Error("iamrx Particles: a box reaches outside its level's domain");
            for (int k = (b.lo[2] - lv.dlo[2]) / gr; k <= (b.hi[2] - lv.dlo[2]) / gr; ++k)
                for (int j = (b.lo[1] - lv.dlo[1]) / gr; j <= (b.hi[1] - lv.dlo[1]) / gr; ++j)
                    for (int i = (b.lo[0] - lv.dlo[0]) / gr; i <= (b.hi[0] - lv.dlo[0]) / gr; ++i) tab[i + (size_t)lv.tn[0] * (j + (size_t)lv.tn[1] * k)] = q;
        }
        if (l == 0 && std::find(tab.begin(), tab.end(), -1) != tab.end()) throw Error("iamrx Particles: level 0 does not cover the domain");
        int* dt = nullptr;
        IAMRX_HIP_CHECK(hipMalloc(&dt, nt * sizeof(int)));
        IAMRX_HIP_CHECK(hipMemcpy(dt, tab.data(), nt * sizeof(int), hipMemcpyHostToDevice));
        m_tabs.push_back(dt);
        lv.tab = dt; lv.boxes = lay.d_boxes; lv.key0 = key0; lv.nbox = lay.nlocal();
        lv.gboxes = lay.d_boxes; lv.owner = nullptr; lv.lidx = nullptr; lv.ngbox = nb;
        if (ranks) {                                          // one block: owner[nb], lidx[nb], then the nb global boxes
            static_assert(sizeof(BoxD) % sizeof(int) == 0, "BoxD is made of ints");
            std::vector<int> h((size_t)2 * nb + (size_t)nb * (sizeof(BoxD) / sizeof(int)));
            // (Layout::local_of is this rank's view; the local index ON THE OWNER is the box's place among its owner's boxes)
            std::vector<int> seen(ctx.comm->nranks, 0);
            for (int q = 0; q < nb; ++q) {
                if (lay.owner[q] < 0 || lay.owner[q] >= ctx.comm->nranks) throw Error("iamrx Particles: a box is owned by no rank of the communicator");
                h[q] = lay.owner[q];
                h[(size_t)nb + q] = seen[lay.owner[q]]++;
            }
            if (nb > 0) std::memcpy(h.data() + 2 * (size_t)nb, lay.boxes.data(), (size_t)nb * sizeof(BoxD));
            int* dg = nullptr;
            IAMRX_HIP_CHECK(hipMalloc(&dg, std::max<size_t>(h.size(), 1) * sizeof(int)));
            IAMRX_HIP_CHECK(hipMemcpy(dg, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
            m_tabs.push_back(dg);
            lv.owner = dg; lv.lidx = dg + nb; lv.gboxes = (const BoxD*)(dg + 2 * (size_t)nb);
        }
        key0 += lay.nlocal();
    }
    m_nkeys = key0;
    // the caller redistributes from level max(keep - 1, 0) or below; until then the per-level ranges are not meaningful
    m_lev_n.assign(nl, 0); m_lev_start.assign(nl, 0);
    m_lev_n[0] = m_np;
    if (m_np > 0) hipLaunchKernelGGL(k_part_relevel, dim3(nblocks(m_np)), dim3(PB), 0, ctx.stream, m_a, m_np, keep);
}

long Particles::add(long n, const double* xyz, const double* r, const int* ids, const int* cpus)
{
    auto& ctx = Context::get();
    const int nr = ctx.comm->nranks, me = ctx.comm->rank;
    bool bad = n < 0 || (n > 0 && !xyz);
    if (nr > 1) {
        // one allreduce (max): slot q the number of particles rank q adds without ids, then the id counter the ranks' ids ask for, then
        // whether a rank was called with arguments it must refuse (every rank then throws)
        std::vector<double> v((size_t)nr + 2, 0.0);
        if (!bad) {
            if (!ids) v[me] = (double)n;
            else for (long p = 0; p < n; ++p) v[nr] = std::max(v[nr], (double)ids[p] + 1.0);
        }
        v[(size_t)nr + 1] = bad ? 1.0 : 0.0;
        ctx.comm->allreduce(v.data(), nr + 2, ReduceOp::Max);
        bad = v[(size_t)nr + 1] > 0.0;
        if (!bad) {
            // without ids the new ids continue the counter in rank order: rank q's follow rank q - 1's
            long before = 0, all = 0;
            for (int q = 0; q < nr; ++q) { if (q < me) before += (long)v[q]; all += (long)v[q]; }
            const int first = next_id + (int)before;
            next_id = std::max(next_id + (int)all, (int)v[nr]);
            if (n > 0 && !ids) {
                std::vector<int> mine((size_t)n);
                std::iota(mine.begin(), mine.end(), first);
                const int keep = next_id;
                add_local(n, xyz, r, mine.data(), cpus);
                next_id = keep;
            } else if (n > 0) {
                const int keep = next_id;
                add_local(n, xyz, r, ids, cpus);
                next_id = keep;
            }
        }
    }
    if (bad) throw Error(n < 0 ? "iamrx Particles::add: negative count" : "iamrx Particles::add: null positions, or a call another rank had to refuse");
    if (nr == 1) add_local(n, xyz, r, ids, cpus);
    return redistribute(0, nlevels() - 1, 0);
}

// the caller's particles onto the end of this rank's arrays (level 0, box 0 until the redistribution that follows)
void Particles::add_local(long n, const double* xyz, const double* r, const int* ids, const int* cpus)
{
    if (n > 0) {
        auto& ctx = Context::get();
        reserve(m_np + n);
        std::vector<double> h((size_t)6 * n, 0.0);
        std::vector<int> hi((size_t)4 * n, 0);
        for (long p = 0; p < n; ++p) {
            for (int e = 0; e < 3; ++e) { h[(size_t)e * n + p] = xyz[3 * p + e]; if (r) h[(size_t)(3 + e) * n + p] = r[3 * p + e]; }
            hi[p] = ids ? ids[p] : next_id++;
            hi[(size_t)n + p] = cpus ? cpus[p] : 0;
        }
        if (ids) for (long p = 0; p < n; ++p) next_id = std::max(next_id, ids[p] + 1);
        for (int e = 0; e < 3; ++e) {
            IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.x[e] + m_np, h.data() + (size_t)e * n, n * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
            IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.r[e] + m_np, h.data() + (size_t)(3 + e) * n, n * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
        }
        IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.id + m_np, hi.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.cpu + m_np, hi.data() + n, n * sizeof(int), hipMemcpyHostToDevice, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.lev + m_np, hi.data() + 2 * (size_t)n, n * sizeof(int), hipMemcpyHostToDevice, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.box + m_np, hi.data() + 3 * (size_t)n, n * sizeof(int), hipMemcpyHostToDevice, ctx.stream));
        ctx.sync();                                            // the host vectors go
        m_np += n;
        m_lev_n[0] += n;                                       // provisional: level 0, box 0 until the redistribution
    }
}

void Particles::read(double* xyz, double* r, int* id, int* cpu, int* lev, int* box) const
{
    if (m_np == 0) return;
    auto& ctx = Context::get();
    const long n = m_np;
    std::vector<double> h((size_t)6 * n);
    for (int e = 0; e < 3; ++e) {
        IAMRX_HIP_CHECK(hipMemcpyAsync(h.data() + (size_t)e * n, m_a.x[e], n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(h.data() + (size_t)(3 + e) * n, m_a.r[e], n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
    }
    if (id) IAMRX_HIP_CHECK(hipMemcpyAsync(id, m_a.id, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    if (cpu) IAMRX_HIP_CHECK(hipMemcpyAsync(cpu, m_a.cpu, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    if (lev) IAMRX_HIP_CHECK(hipMemcpyAsync(lev, m_a.lev, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    if (box) IAMRX_HIP_CHECK(hipMemcpyAsync(box, m_a.box, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    for (long p = 0; p < n; ++p)
        for (int e = 0; e < 3; ++e) {
            if (xyz) xyz[3 * p + e] = h[(size_t)e * n + p];
            if (r) r[3 * p + e] = h[(size_t)(3 + e) * n + p];
        }
}

void Particles::set_positions(const double* xyz)
{
    if (m_np == 0) return;
    auto& ctx = Context::get();
    const long n = m_np;
    std::vector<double> h((size_t)3 * n);
    for (long p = 0; p < n; ++p) for (int e = 0; e < 3; ++e) h[(size_t)e * n + p] = xyz[3 * p + e];
    for (int e = 0; e < 3; ++e) IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.x[e], h.data() + (size_t)e * n, n * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
    ctx.sync();
}

void Particles::advect(int lev, const MultiFab* const umac[3], double dt)
{
    if (lev < 0 || lev >= nlevels()) throw Error("iamrx Particles::advect: no such level");
    const Layout& lay = *m_layouts[lev];
    for (int d = 0; d < 3; ++d) {
        const MultiFab& u = *umac[d];
        if (u.layout->id != lay.id) throw Error("iamrx Particles::advect: the face velocities are not on the level's boxes");
        const IndexType ft = face_type(d);
        if (u.type.t[0] != ft.t[0] || u.type.t[1] != ft.t[1] || u.type.t[2] != ft.t[2] || u.ncomp < 1 || u.ngrow < 1)
            throw Error("iamrx Particles::advect: umac[d] must be face-centred in d with at least one ghost layer");
    }
    const long n = m_lev_n[lev];
    if (n == 0) return;
    auto& ctx = Context::get();
    const Geometry& g = m_geoms[lev];
    AdvGeom G;
    for (int e = 0; e < 3; ++e) { G.plo[e] = g.problo[e]; G.dx[e] = g.dx[e]; G.dlo[e] = g.domain.lo[e]; G.dhi[e] = g.domain.hi[e]; G.per[e] = g.periodic[e]; }
    const dim3 grid(nblocks(n));
    hipLaunchKernelGGL(k_part_advect<1>, grid, dim3(PB), 0, ctx.stream, G, m_a, m_lev_start[lev], n, umac[0]->d_tab, umac[1]->d_tab, umac[2]->d_tab,
                       lay.nlocal(), dt, fixed_dir);
    hipLaunchKernelGGL(k_part_advect<2>, grid, dim3(PB), 0, ctx.stream, G, m_a, m_lev_start[lev], n, umac[0]->d_tab, umac[1]->d_tab, umac[2]->d_tab,
                       lay.nlocal(), dt, fixed_dir);
}

long Particles::redistribute(int lev_min, int lev_max, int ngrow)
{
    const int fin = nlevels() - 1;
    if (lev_min < 0 || lev_min > fin || lev_max < lev_min) throw Error("iamrx Particles::redistribute: bad level range");
    lev_max = std::min(lev_max, fin);
    if (ngrow < 0) throw Error("iamrx Particles::redistribute: negative ngrow");
    if (ngrow > 0) {
        const Layout& lay = *m_layouts[lev_min];
        for (auto& b : lay.boxes)                              // the global list: every rank decides alike
            for (int e = 0; e < 3; ++e)
                if (b.len(e) < ngrow) throw Error("iamrx Particles::redistribute: ngrow exceeds the length of a box");
    }
    auto& ctx = Context::get();
    if (ctx.comm->nranks > 1) return redistribute_ranks(lev_min, lev_max, ngrow);
    if (m_np == 0) return 0;
    const long n = m_np;
    const int nk = m_nkeys;
    int* ws = (int*)ctx.alloc(((size_t)n + 3 * (size_t)nk + 3) * sizeof(int));
    int *key = ws, *counts = ws + n, *offs = counts + nk + 3, *cursor = offs + nk;
    IAMRX_HIP_CHECK(hipMemsetAsync(counts, 0, (nk + 3) * sizeof(int), ctx.stream));
    hipLaunchKernelGGL(k_part_place<false>, dim3(nblocks(n)), dim3(PB), 0, ctx.stream, m_h, m_a, n, lev_min, lev_max, ngrow, nk, key, counts, 0,
                       (int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_part_prefix, dim3(1), dim3(PB), 0, ctx.stream, nk, counts, offs, cursor);
    std::vector<int> hc(nk + 3);
    IAMRX_HIP_CHECK(hipMemcpyAsync(hc.data(), counts, (nk + 3) * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    if (hc[nk + 1] > 0) {
        ctx.free(ws);
        throw Error("iamrx Particles::redistribute(" + std::to_string(lev_min) + ", " + std::to_string(lev_max) + ", " + std::to_string(ngrow) + "): " +
                    std::to_string(hc[nk + 1]) + " particles are in no box of levels " + std::to_string(lev_min) + " .. " + std::to_string(lev_max));
    }
    void* nb = ctx.alloc(block_bytes(m_cap));
    PArrays na;
    carve(na, nb, m_cap);
    hipLaunchKernelGGL(k_part_scatter, dim3(nblocks(n)), dim3(PB), 0, ctx.stream, m_h, m_a, na, n, key, offs, cursor);
    ctx.free(ws);
    ctx.free(m_block);
    m_block = nb; m_a = na;
    long total = 0;
    for (int l = 0; l <= fin; ++l) {
        long s = 0;
        for (int q = 0; q < m_h.L[l].nbox; ++q) s += hc[m_h.L[l].key0 + q];
        m_lev_start[l] = total; m_lev_n[l] = s;
        total += s;
    }
    m_np = total;
    n_removed += hc[nk];
    return hc[nk];
}

// Several ranks.  Collectives: ONE allreduce (the nranks x nranks matrix of send counts, each rank its row, with the numbers of particles
// that cannot be placed and that were removed) and ONE exchange, whatever the number of particles; a rank without particles or boxes
// takes part in both.  Read-backs: the place kernel's counters, and the group counters again once the arrivals are filed.
long Particles::redistribute_ranks(int lev_min, int lev_max, int ngrow)
{
    auto& ctx = Context::get();
    const int nr = ctx.comm->nranks, me = ctx.comm->rank, fin = nlevels() - 1;
    const long n = m_np;
    const int nk = m_nkeys, nc = nk + 3 + nr;
    // ints: key[n], dlev[n], dbox[n], counts[nc], offs[nk], cursor[nk], scursor[nr], rstart[nr + 1]; then the positions as they were
    const size_t nint = 3 * (size_t)n + (size_t)nc + 2 * (size_t)nk + 2 * (size_t)nr + 1;
    const size_t ioff = (nint * sizeof(int) + 7) / 8 * 8;
    char* ws = (char*)ctx.alloc(ioff + 3 * (size_t)n * sizeof(double) + 8);
    int *key = (int*)ws, *dlev = key + n, *dbox = dlev + n, *counts = dbox + n, *offs = counts + nc, *cursor = offs + nk, *scursor = cursor + nk,
        *rstart = scursor + nr;
    double* xkeep = (double*)(ws + ioff);
    IAMRX_HIP_CHECK(hipMemsetAsync(counts, 0, ((size_t)nc + 2 * (size_t)nk + nr) * sizeof(int), ctx.stream));      // counts, offs, cursor, scursor
    if (n > 0) {
        // the place kernel writes the wrapped / image position in place: kept aside so that a collective error leaves the container as it was
        for (int e = 0; e < 3; ++e) IAMRX_HIP_CHECK(hipMemcpyAsync(xkeep + (size_t)e * n, m_a.x[e], n * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
        hipLaunchKernelGGL(k_part_place<true>, dim3(nblocks(n)), dim3(PB), 0, ctx.stream, m_h, m_a, n, lev_min, lev_max, ngrow, nk, key, counts, me, dlev, dbox);
    }
    std::vector<int> hc(nc);
    IAMRX_HIP_CHECK(hipMemcpyAsync(hc.data(), counts, nc * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    std::vector<double> M((size_t)nr * nr + 2, 0.0);
    for (int q = 0; q < nr; ++q) M[(size_t)me * nr + q] = (double)hc[nk + 3 + q];
    M[(size_t)nr * nr] = (double)hc[nk + 1];
    M[(size_t)nr * nr + 1] = (double)hc[nk];
    ctx.comm->allreduce(M.data(), nr * nr + 2, ReduceOp::Sum);
    const long nbad = (long)M[(size_t)nr * nr], removed = (long)M[(size_t)nr * nr + 1];
    if (nbad > 0) {
        for (int e = 0; e < 3 && n > 0; ++e) IAMRX_HIP_CHECK(hipMemcpyAsync(m_a.x[e], xkeep + (size_t)e * n, n * sizeof(double), hipMemcpyDeviceToDevice, ctx.stream));
        ctx.free(ws);
        throw Error("iamrx Particles::redistribute(" + std::to_string(lev_min) + ", " + std::to_string(lev_max) + ", " + std::to_string(ngrow) + "): " +
                    std::to_string(nbad) + " particles are in no box of levels " + std::to_string(lev_min) + " .. " + std::to_string(lev_max));
    }
    long nsend = 0, nrecv = 0;
    std::vector<int> hr(nr + 1, 0);
    for (int q = 0; q < nr; ++q) { nsend += hc[nk + 3 + q]; hr[q + 1] = hr[q] + (int)M[(size_t)q * nr + me]; }
    nrecv = hr[nr];
    double *sbuf = nullptr, *rbuf = nullptr;
    int* akey = nullptr;
    if (nsend > 0) {
        sbuf = (double*)ctx.alloc((size_t)nsend * NREC * sizeof(double));
        hipLaunchKernelGGL(k_part_pack, dim3(nblocks(n)), dim3(PB), 0, ctx.stream, m_a, n, key, dlev, dbox, counts + nk + 3, scursor, sbuf);
    }
    if (nrecv > 0) {
        rbuf = (double*)ctx.alloc((size_t)nrecv * NREC * sizeof(double));
        akey = (int*)ctx.alloc((size_t)nrecv * sizeof(int));
    }
    // a peer appears on both sides exactly where the matrix says so: every rank read the same matrix
    std::vector<Message> sends, recvs;
    size_t so = 0;
    for (int q = 0; q < nr; ++q) {
        const size_t sc = (size_t)hc[nk + 3 + q], rc = (size_t)(hr[q + 1] - hr[q]);
        if (sc > 0) sends.push_back({q, sbuf + so * NREC, sc * NREC});
        if (rc > 0) recvs.push_back({q, rbuf + (size_t)hr[q] * NREC, rc * NREC});
        so += sc;
    }
    if (!sends.empty() || !recvs.empty()) ctx.comm->exchange(sends, recvs, ctx.stream);
    if (nrecv > 0) {
        ctx.upload_async(rstart, hr.data(), (nr + 1) * sizeof(int));
        hipLaunchKernelGGL(k_part_file, dim3(nblocks(nrecv)), dim3(PB), 0, ctx.stream, m_h, rbuf, rstart, nr, nrecv, me, nk, akey, counts);
        IAMRX_HIP_CHECK(hipMemcpyAsync(hc.data(), counts, (nk + 2) * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));      // the groups with the arrivals
    }
    if (nk > 0) hipLaunchKernelGGL(k_part_prefix, dim3(1), dim3(PB), 0, ctx.stream, nk, counts, offs, cursor);
    if (nrecv > 0) ctx.sync();
    const long misfiled = nrecv > 0 ? hc[nk + 1] : 0;          // (the place kernel's count there was zero, or the error above was thrown)
    long total = 0;
    for (int l = 0; l <= fin; ++l) {
        long s = 0;
        for (int q = 0; q < m_h.L[l].nbox; ++q) s += hc[m_h.L[l].key0 + q];
        m_lev_start[l] = total; m_lev_n[l] = s;
        total += s;
    }
    const long cap = std::max(m_cap, total > m_cap ? std::max(total, std::max(1024L, 2 * m_cap)) : 0L);
    if (cap > 0 && (n > 0 || nrecv > 0)) {
        void* nb = ctx.alloc(block_bytes(cap));
        PArrays na;
        carve(na, nb, cap);
        hipLaunchKernelGGL(k_part_scatter_ranks, dim3(nblocks(n + nrecv)), dim3(PB), 0, ctx.stream, m_h, m_a, na, n, key, rbuf, rstart, nr, nrecv, akey, offs, cursor);
        if (m_block) ctx.free(m_block);
        m_block = nb; m_a = na; m_cap = cap;
    }
    ctx.free(ws);
    if (sbuf) ctx.free(sbuf);
    if (rbuf) ctx.free(rbuf);
    if (akey) ctx.free(akey);
    m_np = total;
    n_removed += removed;
    if (misfiled > 0) throw Error("iamrx Particles::redistribute: " + std::to_string(misfiled) + " arriving particles name no box of this rank");
    return removed;
}

void Particles::global_count(long* per_level, long* total) const
{
    auto& ctx = Context::get();
    const int nl = nlevels();
    std::vector<double> v((size_t)nl + 1, 0.0);
    for (int l = 0; l < nl; ++l) v[l] = (double)m_lev_n[l];
    v[nl] = (double)m_np;
    if (ctx.comm->nranks > 1) ctx.comm->allreduce(v.data(), nl + 1, ReduceOp::Sum);
    if (per_level) for (int l = 0; l < nl; ++l) per_level[l] = (long)v[l];
    if (total) *total = (long)v[nl];
}

void Particles::particle_count(int lev, MultiFab& out, int ocomp)
{
    if (lev < 0 || lev >= nlevels()) throw Error("iamrx Particles::particle_count: no such level");
    if (out.layout->id != m_layouts[lev]->id || !out.type.cell() || ocomp < 0 || ocomp >= out.ncomp)
        throw Error("iamrx Particles::particle_count: out must be cell-centred on the level's boxes");
    out.setVal(0.0, ocomp, 1, out.ngrow);
    if (m_lev_n[lev] == 0) return;
    auto& ctx = Context::get();
    hipLaunchKernelGGL(k_part_count, dim3(nblocks(m_lev_n[lev])), dim3(PB), 0, ctx.stream, m_h, m_a, m_lev_start[lev], m_lev_n[lev], lev, out.d_tab, ocomp);
}

void Particles::total_particle_count(int lev, MultiFab& out, int ocomp)
{
    particle_count(lev, out, ocomp);
    const int fin = nlevels() - 1;
    if (lev == fin) return;
    if (Context::get().comm->nranks > 1) { add_finer_counts_ranks(lev, out, ocomp); return; }
    const long p0 = m_lev_start[lev + 1], n = m_np - p0;        // the groups are ordered by level: everything finer than lev
    if (n <= 0) return;
    auto& ctx = Context::get();
    hipLaunchKernelGGL(k_part_count, dim3(nblocks(n)), dim3(PB), 0, ctx.stream, m_h, m_a, p0, n, lev, out.d_tab, ocomp);
}

// Several ranks: a fine box and the coarse box under it may have different owners.  From the finest level down to lev + 1: the level's
// own count plus what the finer levels handed down, summed onto the level's boxes coarsened by the ratio (same owners: no communication),
// then copied to the boxes of the next coarser level wherever they are (parallel_copy).  Counts are small integers: every sum is exact.
void Particles::add_finer_counts_ranks(int lev, MultiFab& out, int ocomp)
{
    auto& ctx = Context::get();
    const int fin = nlevels() - 1, r = m_ratio;
    MultiFab carry;                                           // on the coarsened boxes of level lf + 1: the counts of the levels > lf
    for (int lf = fin; lf > lev; --lf) {
        const LayoutP& fl = m_layouts[lf];
        for (auto& b : fl->boxes)
            for (int e = 0; e < 3; ++e)
                if (b.lo[e] % r != 0 || b.len(e) % r != 0) throw Error("iamrx Particles::total_particle_count: a box of a refined level is not aligned to the ratio");
        MultiFab cur(fl, cell_type(), 1, 0);
        particle_count(lf, cur, 0);
        if (carry.defined()) {
            MultiFab below(fl, cell_type(), 1, 0);
            below.setVal(0.0);
            parallel_copy(below, carry, 0, 0, 1, 0, 0, nullptr);
            mf_saxpy(cur, 1.0, below, 0, 0, 1, 0);
        }
        LayoutP cl = fl->coarsened(r);
        MultiFab sum(cl, cell_type(), 1, 0);
        const FabD *ct = sum.d_tab, *ft = cur.d_tab;
        for_each(*cl, cell_type(), 0, ctx.stream, [=] __device__(int i, int j, int k, int f) {
            const FabD F = ft[f];
            double s = 0.0;
            for (int kk = 0; kk < r; ++kk)
                for (int jj = 0; jj < r; ++jj)
                    for (int ii = 0; ii < r; ++ii) s += F(r * i + ii, r * j + jj, r * k + kk);
            ct[f](i, j, k) = s;
        });
        carry = std::move(sum);
    }
    MultiFab below(m_layouts[lev], cell_type(), 1, 0);
    below.setVal(0.0);
    parallel_copy(below, carry, 0, 0, 1, 0, 0, nullptr);
    mf_saxpy(out, 1.0, below, 0, ocomp, 1, 0);
}

// ---- state at the particles; timestamp files ------------------------------------------------------------------------------------------------
void Particles::sample(int lev, const MultiFab& mf, const int* comps, int M, double* host_vals, int* id, int* cpu)
{
    if (lev < 0 || lev >= nlevels()) throw Error("iamrx Particles::sample: no such level");
    if (!mf.layout || mf.layout->id != m_layouts[lev]->id || !mf.type.cell()) throw Error("iamrx Particles::sample: mf must be cell-centred on the level's boxes");
    if (M < 1 || M > MAX_SAMPLE || !comps) throw Error("iamrx Particles::sample: 1 .. " + std::to_string(MAX_SAMPLE) + " components");
    SampleComps C;
    C.n = M;
    for (int m = 0; m < MAX_SAMPLE; ++m) C.c[m] = 0;
    for (int m = 0; m < M; ++m) {
        if (comps[m] < 0 || comps[m] >= mf.ncomp) throw Error("iamrx Particles::sample: component " + std::to_string(comps[m]) + " of an array of " + std::to_string(mf.ncomp));
        C.c[m] = comps[m];
    }
    const long n = m_lev_n[lev], p0 = m_lev_start[lev];
    if (n == 0) return;
    auto& ctx = Context::get();
    const Geometry& g = m_geoms[lev];
    SampleGeom G;
    for (int e = 0; e < 3; ++e) { G.plo[e] = g.problo[e]; G.dx[e] = g.dx[e]; G.dlo[e] = g.domain.lo[e]; }
    double* d_out = (double*)ctx.alloc((size_t)M * n * sizeof(double));
    IAMRX_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)M * n * sizeof(double), ctx.stream));
    hipLaunchKernelGGL(k_part_sample, dim3(nblocks(n)), dim3(PB), 0, ctx.stream, G, m_a, p0, n, mf.d_tab, m_layouts[lev]->nlocal(), C, d_out);
    if (!host_vals && !id && !cpu) { ctx.free(d_out); return; }
    std::vector<double> h;
    if (host_vals) {
        h.resize((size_t)M * n);
        IAMRX_HIP_CHECK(hipMemcpyAsync(h.data(), d_out, (size_t)M * n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
    }
    if (id) IAMRX_HIP_CHECK(hipMemcpyAsync(id, m_a.id + p0, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    if (cpu) IAMRX_HIP_CHECK(hipMemcpyAsync(cpu, m_a.cpu + p0, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
    ctx.sync();
    ctx.free(d_out);
    if (host_vals)
        for (long p = 0; p < n; ++p)
            for (int m = 0; m < M; ++m) host_vals[(size_t)p * M + m] = h[(size_t)m * n + p];
}

void Particles::set_timestamp(const std::string& basename, std::vector<int> indices)
{
    if ((int)indices.size() > MAX_SAMPLE) throw Error("iamrx Particles::set_timestamp: at most " + std::to_string(MAX_SAMPLE) + " indices");
    for (int i : indices) if (i < 0) throw Error("iamrx Particles::set_timestamp: negative index");
    // upstream caps the number of files at 64 and lets the ranks that share one take turns; here every rank has a file of its own
    if (!basename.empty() && Context::get().comm->nranks > 64) throw Error("iamrx Particles::set_timestamp: more than 64 ranks would share timestamp files");
    m_ts_base = basename;
    m_ts_indices = basename.empty() ? std::vector<int>() : std::move(indices);
}

void Particles::timestamp(int lev, const MultiFab* mf, double time)
{
    if (lev < 0 || lev >= nlevels()) throw Error("iamrx Particles::timestamp: no such level");
    if (m_ts_base.empty()) throw Error("iamrx Particles::timestamp: no basename set (set_timestamp)");
    const int M = mf ? (int)m_ts_indices.size() : 0;
    if (mf && M > mf->ncomp) throw Error("iamrx Particles::timestamp: mf holds fewer components than there are indices");
    const long n = m_lev_n[lev], p0 = m_lev_start[lev];
    if (n == 0) return;
    auto& ctx = Context::get();
    std::vector<double> vals((size_t)M * n), xr((size_t)6 * n);
    std::vector<int> id(n), cpu(n);
    for (int e = 0; e < 3; ++e) {
        IAMRX_HIP_CHECK(hipMemcpyAsync(xr.data() + (size_t)e * n, m_a.x[e] + p0, n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(xr.data() + (size_t)(3 + e) * n, m_a.r[e] + p0, n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
    }
    if (M > 0) {
        int comps[MAX_SAMPLE];
        for (int m = 0; m < M; ++m) comps[m] = m;
        sample(lev, *mf, comps, M, vals.data(), id.data(), cpu.data());      // (synchronises: the copies above have arrived too)
    } else {
        IAMRX_HIP_CHECK(hipMemcpyAsync(id.data(), m_a.id + p0, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
        IAMRX_HIP_CHECK(hipMemcpyAsync(cpu.data(), m_a.cpu + p0, n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
        ctx.sync();
    }
    // the order inside a box is not part of the container's contract: the lines of one call go out sorted by (id, cpu)
    std::vector<long> ord;
    for (long p = 0; p < n; ++p) if (id[p] > 0) ord.push_back(p);
    if (ord.empty()) return;
    std::sort(ord.begin(), ord.end(), [&](long a, long b) { return id[a] != id[b] ? id[a] < id[b] : (cpu[a] != cpu[b] ? cpu[a] < cpu[b] : a < b); });
    char buf[64];
    std::snprintf(buf, sizeof buf, "_%02d", ctx.comm->rank % 64);
    const std::string path = m_ts_base + buf;
    std::FILE* f = std::fopen(path.c_str(), "a");
    if (!f) throw Error("iamrx Particles::timestamp: cannot open " + path);
    std::string line;
    auto real = [&](double v) { std::snprintf(buf, sizeof buf, " %.10e", v); line += buf; };
    for (long p : ord) {
        std::snprintf(buf, sizeof buf, "%d %d", id[p], cpu[p]);
        line = buf;
        for (int e = 0; e < 3; ++e) if (e != fixed_dir) real(xr[(size_t)e * n + p]);
        real(time);
        for (int e = 0; e < 3; ++e) if (e != fixed_dir) real(xr[(size_t)(3 + e) * n + p]);
        for (int m = 0; m < M; ++m) real(vals[(size_t)p * M + m]);
        line += '\n';
        std::fputs(line.c_str(), f);
    }
    if (std::fclose(f) != 0) throw Error("iamrx Particles::timestamp: writing " + path + " failed");
}

// ---- ghost faces of a refined level for its particles ------------------------------------------------------------------------------------
void particles_grow_umac(MultiFab ug[3], const MultiFab* const umac_fine[3], const MultiFab* const umac_crse[3], const Geometry& cgeom,
                         const Geometry& fgeom, int ratio, int ng)
{
    const LayoutP fl = umac_fine[0]->layout;
    IAMRX_ASSERT(ng >= 1 && ratio >= 2);
    auto& ctx = Context::get();
    std::vector<BoxD> cb;
    for (auto& b : fl->boxes) cb.push_back(coarsen(grow(b, ng), ratio));
    LayoutP cl = std::make_shared<Layout>(cb, fl->owner, ctx.comm->rank);
    for (int d = 0; d < 3; ++d) {
        MultiFab& uf = ug[d];
        if (!uf.defined() || uf.layout->id != fl->id || uf.ngrow != ng) uf.define(fl, face_type(d), 1, ng);
        MultiFab cpatch(cl, face_type(d), 1, 0);
        cpatch.setVal(0.0);
        parallel_copy(cpatch, *umac_crse[d], 0, 0, 1, 0, 0, &cgeom);
        const FabD *ft = uf.d_tab, *ct = cpatch.d_tab;
        const int r = ratio;
        const double rinv = 1.0 / (double)ratio;
        // every face of the grown array from the coarse level: FaceLinear (linear between two coarse faces along d, constant across)
        for_each(*fl, face_type(d), ng, ctx.stream, [=] __device__(int i, int j, int k, int f) {
            const int fi[3] = {i, j, k};
            int c[3];
            for (int e = 0; e < 3; ++e) c[e] = fi[e] >= 0 ? fi[e] / r : -((-fi[e] + r - 1) / r);
            const FabD cf = ct[f];
            const int rem = fi[d] - c[d] * r;
            double v;
            if (rem == 0) v = cf(c[0], c[1], c[2]);
            else {
                const double w = (double)rem * rinv;
                int cp[3] = {c[0], c[1], c[2]};
                cp[d] += 1;
                v = (1.0 - w) * cf(c[0], c[1], c[2]) + w * cf(cp[0], cp[1], cp[2]);
            }
            ft[f](i, j, k) = v;
        });
        MultiFab::Copy(uf, *umac_fine[d], 0, 0, 1, 0);       // the level's own faces, for its neighbours' ghost layers
        uf.FillBoundary(fgeom);                              // fine and periodic neighbours where they exist
        MultiFab::Copy(uf, *umac_fine[d], 0, 0, 1, 1);       // valid faces and the divergence-fixed first layer as the level holds them
    }
}

}  // namespace iamrx
