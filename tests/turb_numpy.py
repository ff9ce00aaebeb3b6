"""The yardstick of the turbulent-forcing tests: a numpy restatement of the mode table of TurbulentForcing::init_turbulent_forcing (reference
Tutorials/HIT/TurbulentForcing_def.H:21-366, generator Tutorials/HIT/depRand.cpp) and of the per-cell mode sum of NavierStokesBase::getForce
(Tutorials/HIT/NS_getForce.cpp:553-686).  Written from the reference text in this file's own words and independent of the product: the
random stream is numpy's own MT19937, the field is the direct sum over the modes at every cell, in float64 or np.longdouble."""
import numpy as np

FIELDS = ("FTX", "TAT", "FPX", "FPY", "FPZ", "FAX", "FAY", "FAZ", "FPXX", "FPXY", "FPXZ", "FPYX", "FPYY", "FPYZ", "FPZX", "FPZY", "FPZZ")
IX = {n: q for q, n in enumerate(FIELDS)}
TWOPI = 2.0 * 3.141592653589793238462643383279502884197      # iamr_constants.H: a double
PI = 3.141592653589793238462643383279502884197
SEED = 111397


class Stream:
    """DepRand::Random(): MT19937 seeded by init_genrand, the 32-bit draw times 1 / (2^32 - 1) (depRand.cpp:46-59, 187-191).  numpy's
    RandomState(seed) is that generator with that seeding, and randint over the full uint32 range hands out its raw draws (seed 5489 gives
    3499211612, 581869302, 3890346734: the published head of the MT19937 stream)"""

    def __init__(self, seed=SEED, n=1 << 16):
        self.raw = np.random.RandomState(seed).randint(0, 2 ** 32, size=n, dtype=np.uint32)
        self.pos = 0

    def __call__(self):
        v = float(self.raw[self.pos]) * (1.0 / 4294967295.0)
        self.pos += 1
        return v


def modes(prob_lo, prob_hi, nmodes=4, mode_start=0, div_free=1):
    """-> (k (M, 3) int, data (M, 17) float64 in the order of FIELDS): the entries upstream's two loops write, in their order"""
    Lx, Ly, Lz = (float(prob_hi[d]) - float(prob_lo[d]) for d in range(3))
    assert Lx == Ly and Lz >= Lx
    Lmin = min(Lx, Ly, Lz)
    kappa_max = float(nmodes) / Lmin + 1.0e-8
    step = [int(L / Lmin + 0.5) for L in (Lx, Ly, Lz)]
    nmax = [nmodes * int(0.5 + L / Lmin) for L in (Lx, Ly, Lz)]
    fmin, fmax = 1.0 / 1.0, 1.0 / 0.5          # forcing_time_scale_max / min
    rnd = Stream()
    ks, rows = [], []

    def one(kx, ky, kz):
        kappa = np.sqrt((float(kx) * kx) / (Lx * Lx) + (float(ky) * ky) / (Ly * Ly) + (float(kz) * kz) / (Lz * Lz))
        if not kappa <= kappa_max:
            return
        r = np.zeros(17)
        r[IX["FTX"]] = (fmin + (fmax - fmin) * rnd()) * TWOPI
        r[IX["TAT"]] = rnd() * TWOPI
        for n in ("FPX", "FPY", "FPZ"):
            r[IX[n]] = rnd() * TWOPI
        if div_free:
            for n in ("FPXX", "FPYX", "FPZX", "FPXY", "FPYY", "FPZY", "FPXZ", "FPYZ", "FPZZ"):
                r[IX[n]] = rnd() * TWOPI
        theta = rnd() * TWOPI
        phi = rnd() * PI
        px, py, pz = np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)
        mp2 = px * px + py * py + pz * pz
        if not kappa < 0.000001:
            ekh = 1.0 / (kappa * kappa)
            if div_free:
                ekh /= kappa
            for q in (kx, ky, kz):
                if q == 0:
                    ekh /= 2.0
            r[IX["FAX"]], r[IX["FAY"]], r[IX["FAZ"]] = 1.0 * px * ekh / mp2, 1.0 * py * ekh / mp2, 1.0 * pz * ekh / mp2
        ks.append((kx, ky, kz))
        rows.append(r)

    for kz in range(mode_start * step[2], nmax[2] + 1, step[2]):
        for ky in range(mode_start * step[1], nmax[1] + 1, step[1]):
            for kx in range(mode_start * step[0], nmax[0] + 1, step[0]):
                one(kx, ky, kz)
    for kz in range(1, step[2]):
        for ky in range(mode_start, nmax[1] + 1, step[1]):
            for kx in range(mode_start, nmax[0] + 1, step[0]):
                one(kx, ky, kz)
    return np.array(ks, dtype=np.int64).reshape(-1, 3), np.array(rows).reshape(-1, 17)


def centres(prob_lo, prob_hi, n, lo, hi, dom_lo=(0, 0, 0), dtype=np.float64):
    """cell centres x = prob_lo + (i - dom_lo + 0.5) dx of the index range lo .. hi (inclusive) of a level with n cells, dx in float64"""
    out = []
    for d in range(3):
        dx = (float(prob_hi[d]) - float(prob_lo[d])) / float(n[d])
        i = np.arange(lo[d], hi[d] + 1) - dom_lo[d]
        out.append(dtype(prob_lo[d]) + (i.astype(dtype) + dtype(0.5)) * dtype(dx))
    return out


def field(k, data, div_free, prob_lo, prob_hi, x, y, z, t, dtype=np.float64):
    """the direct per-cell sum: f (nx, ny, nz, 3) at the cell centres x, y, z (1-D arrays) and time t"""
    T = dtype
    X, Y, Z = x.astype(T)[:, None, None], y.astype(T)[None, :, None], z.astype(T)[None, None, :]
    Lx, Ly, Lz = (T(float(prob_hi[d]) - float(prob_lo[d])) for d in range(3))
    tp = T(TWOPI)
    f = np.zeros((len(x), len(y), len(z), 3), dtype=T)
    for (kx, ky, kz), r in zip(k, data):
        v = {n: T(r[q]) for n, q in IX.items()}
        kx, ky, kz = int(kx), int(ky), int(kz)
        xT = np.cos(v["FTX"] * T(t) + v["TAT"])
        ax, ay, az = tp * T(kx) * X / Lx, tp * T(ky) * Y / Ly, tp * T(kz) * Z / Lz
        if div_free:
            f[..., 0] += xT * (v["FAZ"] * tp * (T(ky) / Ly) * np.sin(ax + v["FPZX"]) * np.cos(ay + v["FPZY"]) * np.sin(az + v["FPZZ"])
                               - v["FAY"] * tp * (T(kz) / Lz) * np.sin(ax + v["FPYX"]) * np.sin(ay + v["FPYY"]) * np.cos(az + v["FPYZ"]))
            f[..., 1] += xT * (v["FAX"] * tp * (T(kz) / Lz) * np.sin(ax + v["FPXX"]) * np.sin(ay + v["FPXY"]) * np.cos(az + v["FPXZ"])
                               - v["FAZ"] * tp * (T(kx) / Lx) * np.cos(ax + v["FPZX"]) * np.sin(ay + v["FPZY"]) * np.sin(az + v["FPZZ"]))
            f[..., 2] += xT * (v["FAY"] * tp * (T(kx) / Lx) * np.cos(ax + v["FPYX"]) * np.sin(ay + v["FPYY"]) * np.sin(az + v["FPYZ"])
                               - v["FAX"] * tp * (T(ky) / Ly) * np.sin(ax + v["FPXX"]) * np.cos(ay + v["FPXY"]) * np.sin(az + v["FPXZ"]))
        else:
            f[..., 0] += xT * v["FAX"] * np.cos(ax + v["FPX"]) * np.sin(ay + v["FPY"]) * np.sin(az + v["FPZ"])
            f[..., 1] += xT * v["FAY"] * np.sin(ax + v["FPX"]) * np.cos(ay + v["FPY"]) * np.sin(az + v["FPZ"])
            f[..., 2] += xT * v["FAZ"] * np.sin(ax + v["FPX"]) * np.sin(ay + v["FPY"]) * np.cos(az + v["FPZ"])
    return f


def scale(k, data, prob_lo, prob_hi):
    """S = sum over the modes of 2 * 2 pi * max_d(k_d / L_d) * max(|FAX|, |FAY|, |FAZ|): the size of the sum of the terms' magnitudes"""
    L = np.array([float(prob_hi[d]) - float(prob_lo[d]) for d in range(3)])
    amp = np.abs(data[:, IX["FAX"]:IX["FAZ"] + 1]).max(axis=1)
    return float(np.sum(2.0 * TWOPI * (np.asarray(k, dtype=float) / L).max(axis=1) * amp))


def gravity_mode(g, omega=0.0):
    """one mode, k = 0, for the form without the curl: the uniform acceleration (0, 0, g cos(omega t))"""
    r = np.zeros((1, 17))
    r[0, IX["FTX"]] = omega
    r[0, IX["FPX"]] = r[0, IX["FPY"]] = np.pi / 2
    r[0, IX["FAZ"]] = g
    return np.zeros((1, 3), dtype=np.int32), r
