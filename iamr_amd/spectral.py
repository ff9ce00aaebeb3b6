"""The way back from mode space on a triply periodic level (include/iamrx.h: iamrx_mf_noise / iamrx_mf_filter / iamrx_mf_solenoidal /
iamrx_mf_synthesize; kernels in csrc/k_spectrum.hip): counter-based white noise, low-pass filters (sharp, Gaussian, box), the solenoidal
projection for the exact or the centred-difference wavenumber, and a random solenoidal field with a prescribed shell spectrum -- the
start of the decaying isotropic box (prob.probtype = 101, probinit.py).  The model spectrum and the reader of a `k E` table are host
code; everything else calls the library."""
import ctypes as C
import math
import numpy as np

KINDS = {"identity": 0, "sharp": 1, "gaussian": 2, "box": 3}
WAVENUMBERS = {"exact": 0, "centred": 1}


def _kind(kind):
    if isinstance(kind, str):
        if kind not in KINDS:
            raise ValueError(f"filter kind {kind!r}: one of {', '.join(KINDS)}")
        return KINDS[kind]
    return int(kind)


def _wavenumber(w):
    if isinstance(w, str):
        if w not in WAVENUMBERS:
            raise ValueError(f"wavenumber form {w!r}: one of {', '.join(WAVENUMBERS)}")
        return WAVENUMBERS[w]
    return int(w)


def mf_noise(geom, mf, seed, comp=0, ncomp=1):
    """iamrx_mf_noise: the valid cells of components comp .. comp + ncomp - 1 of a cell-centred MultiFab that tiles the domain of geom
    take white noise, uniform in (-1/2, 1/2), that depends on (seed, component, global cell index) alone."""
    from .lib import lib, check
    check(lib().iamrx_mf_noise(C.byref(geom), mf.h, int(comp), int(ncomp), C.c_ulonglong(int(seed))))


def mf_filter(geom, dst, src, kind, kc, dcomp=0, scomp=0, ncomp=1):
    """iamrx_mf_filter: dst(dcomp + q) = the low-pass filtered src(scomp + q), q < ncomp.  kind: 0 / "identity", 1 / "sharp", 2 / "gaussian",
    3 / "box"; kc: the cut-off in units of 2 pi / L_max (filter width Delta = L_max / (2 kc)).  dst may be src.  Collective."""
    from .lib import lib, check
    check(lib().iamrx_mf_filter(C.byref(geom), dst.h, int(dcomp), src.h, int(scomp), int(ncomp), _kind(kind), C.c_double(float(kc))))


def mf_solenoidal(geom, dst, src, wavenumber="centred", dcomp=0, scomp=0):
    """iamrx_mf_solenoidal: dst(dcomp .. dcomp + 2) = the solenoidal part of src(scomp .. scomp + 2).  wavenumber: 0 / "exact" (the
    continuous field becomes divergence-free) or 1 / "centred" (the centred difference of "diveru" does).  Collective."""
    from .lib import lib, check
    check(lib().iamrx_mf_solenoidal(C.byref(geom), dst.h, int(dcomp), src.h, int(scomp), _wavenumber(wavenumber)))


def mf_synthesize(geom, dst, E_target, seed=42, wavenumber="centred", comp=0):
    """iamrx_mf_synthesize: dst(comp .. comp + 2) = a random solenoidal field whose kinetic-energy spectrum per shell is E_target (one
    entry per shell of geom: spectrum.nbins_of).  The same seed gives the same bits for any box layout and rank count.  Collective."""
    from .lib import lib, check
    E = np.ascontiguousarray(E_target, dtype=np.float64)
    check(lib().iamrx_mf_synthesize(C.byref(geom), dst.h, int(comp), C.c_ulonglong(int(seed)), int(E.size),
                                    E.ctypes.data_as(C.POINTER(C.c_double)), _wavenumber(wavenumber)))


def level_filtered(ns, names, kind, kc):
    """NavierStokes.filtered / Amr.filtered: the named fields of a level (any names derive_fields knows) filtered into a new MultiFab on
    the level's layout, component q = names[q]"""
    names = [names] if isinstance(names, str) else list(names)
    f = ns.derive_fields(names)
    mf_filter(ns.geom, f, f, kind, kc, 0, 0, len(names))
    return f


def hit_spectrum(nbins, L, k0, urms0, normalize=True, n=None):
    """the model spectrum of the HIT tutorial's initial condition as a shell table: E(k) = urms0^2 16 sqrt(2 / pi) k^4 / k0^5
    exp(-2 k^2 / k0^2) with k in units of 2 pi / L_max (its integral over k is 3/2 urms0^2), sampled at k_s = s with shell width 1;
    zero for s = 0 and, when the extents n are given, beyond min_d(n_d r_d) / 2 with r_d = L_max / L_d (the largest sphere every axis
    resolves).  normalize: rescaled so that the table sums to 3/2 urms0^2."""
    from .spectrum import ratios
    s = np.arange(int(nbins), dtype=np.float64)
    E = float(urms0) ** 2 * 16.0 * math.sqrt(2.0 / math.pi) * s ** 4 / float(k0) ** 5 * np.exp(-2.0 * s * s / float(k0) ** 2)
    E[0] = 0.0
    if n is not None:
        r = ratios(L)
        E[s > min(int(n[d]) * r[d] for d in range(3)) / 2.0] = 0.0
    if normalize:
        want = 1.5 * float(urms0) ** 2
        for _ in range(3):
            tot = math.fsum(E)
            if not tot > 0.0:
                raise ValueError("hit_spectrum: the table is empty (k0 beyond the shells of the grid?)")
            E = E * (want / tot)
    return E


def write_spectrum_table(path, E, k=None):
    """two columns `k E`, k in units of 2 pi / L_max (default: the shell numbers), 17 significant digits"""
    E = np.asarray(E, dtype=np.float64)
    k = np.arange(len(E), dtype=np.float64) if k is None else np.asarray(k, dtype=np.float64)
    with open(path, "w") as f:
        f.write("# k E\n")
        for a, b in zip(k, E):
            f.write("%.17g %.17g\n" % (float(a), float(b)))


def read_spectrum_table(path, nbins):
    """a text file of two columns `k E` (blank, comma or semicolon separated; lines starting with '#' and a first line of column names
    are skipped), k in units of 2 pi / L_max and increasing -> the table on the shells s = 0 .. nbins - 1: linear interpolation, an
    entry at k = s is taken as it stands, zero for s = 0 and outside the range of the file"""
    ks, Es = [], []
    with open(path) as f:
        for line in f:
            t = line.replace(",", " ").replace(";", " ").split()
            if not t or t[0].startswith("#"):
                continue
            try:
                a, b = float(t[0]), float(t[1])
            except (ValueError, IndexError):
                if not ks:
                    continue                      # a heading
                raise ValueError(f"{path}: cannot read the line {line.strip()!r}")
            ks.append(a)
            Es.append(b)
    if not ks:
        raise ValueError(f"{path}: no `k E` lines")
    k, E = np.array(ks), np.array(Es)
    if np.any(np.diff(k) <= 0.0) or np.any(E < 0.0) or not np.all(np.isfinite(E)):
        raise ValueError(f"{path}: k must increase and E be finite and non-negative")
    s = np.arange(int(nbins), dtype=np.float64)
    out = np.interp(s, k, E, left=0.0, right=0.0)
    out[0] = 0.0
    return out
