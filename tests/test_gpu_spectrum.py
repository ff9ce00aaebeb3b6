"""GPU: shell-summed power spectra (include/iamrx.h: iamrx_mf_spectrum / iamrx_ns_spectrum / iamrx_amr_spectrum; kernels in
iamr_amd/csrc/k_spectrum.hip) through the C-ABI against the numpy yardstick of tests/spectrum_numpy.py on the same data.

The yardstick is np.fft.fftn / N with math.fsum per shell; the tolerance is its derived bound
|dP(s)| <= 2 eps sqrt(P(s) P_tot) + eps^2 P_tot + count(s) 2^-53 P(s), eps = 16 log2(N) 2^-53 (spectrum_numpy's docstring).  The data
are white noise of order one with a non-zero mean, every ghost cell holds NaN.  The shapes are the smallest at which each path can go
wrong: unequal extents, a non-cubic domain, one box against eight, the longest transform on each axis, a row of exactly one
wavefront."""
import ctypes as C
import functools
import math
import os
import numpy as np
import pytest
import spectrum_numpy as SN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
FORCED = os.path.join(GOLD, "inputs.3d.forced")
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]
UNIT = (1.0, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def reference(n, L, seed=3, ncomp=1):
    """(f (n, ncomp), [(P, count) per component]): computed once per shape and shared, never written to"""
    f = SN.noise(n, seed, ncomp)
    f.setflags(write=False)
    return f, [SN.spectrum_reference(f[..., q], L) for q in range(ncomp)]


def make_mf(n, f, max_grid_size=None, ngrow=1):
    """a cell-centred MultiFab over the domain: f on the valid cells of every box, NaN in ALL ghost cells (also those between boxes)"""
    from iamr_amd import lib as L
    lay = L.Layout.single(n) if max_grid_size is None else L.Layout.decompose(tuple(n), max_grid_size)
    mf = L.MultiFab(lay, L.CELL, f.shape[3], ngrow)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (f.shape[3],), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    return mf, lay


def geom_of(n, L=UNIT, periodic=(1, 1, 1)):
    from iamr_amd import lib
    return lib.Geom.make(list(n), prob_hi=tuple(L), periodic=periodic)


def check(got, ref, N, tag):
    """got (nbins,) against the yardstick's (P, count); prints the largest error in units of the bound"""
    P, count = ref
    bd = SN.bound(P, count, N)
    assert got.shape == P.shape, (tag, got.shape, P.shape)
    err = np.abs(got - P)
    worst = float(np.max(err / bd))
    print(f"{tag}: {len(P)} shells, max |got - yardstick| = {float(err.max()):.3e}, worst error / bound = {worst:.4f}")
    assert np.all(err <= bd), (tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------ 1. one array
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), (1.0, 1.0, 2.0)),
                                 ((1024, 4, 4), UNIT), ((4, 1024, 4), UNIT), ((4, 4, 1024), UNIT), ((64, 4, 4), UNIT), ((4, 64, 4), UNIT)])
def test_one_box(gpu, n, L):
    """unequal extents (an axis mix-up shows); a non-cubic domain with r = (2, 2, 1); the longest transform on each axis; a length of
    exactly one wavefront.  count is the yardstick's exactly and sums to N; a second call gives the same bits."""
    f, refs = reference(n, L)
    mf, lay = make_mf(n, f)
    g = geom_of(n, L)
    P, count = gpu.mf_spectrum(g, mf, 0, 1)
    assert P.shape == (1, len(refs[0][0]))
    check(P[0], refs[0], f.size, f"{n} L {L}")
    assert count.dtype == np.int64 and np.array_equal(count, refs[0][1]) and int(count.sum()) == f.size
    P2, count2 = gpu.mf_spectrum(g, mf, 0, 1)
    assert P2.tobytes() == P.tobytes() and np.array_equal(count2, count)
    assert abs(math.fsum(P[0]) - float(np.mean(f * f))) <= SN.eps_of(f.size) * float(np.mean(f * f))        # Parseval


def test_one_box_against_eight(gpu):
    """32^3 as one box and as eight 16^3 boxes, two components: both inside the bound, and equal to the bit (only the pack differs);
    count may be NULL"""
    n = (32, 32, 32)
    f, refs = reference(n, UNIT, 7, 2)
    g = geom_of(n)
    one, _ = make_mf(n, f)
    eight, lay8 = make_mf(n, f, 16)
    assert len(lay8.boxes) == 8
    Pa, ca = gpu.mf_spectrum(g, one, 0, 2)
    Pb, cb = gpu.mf_spectrum(g, eight, 0, 2)
    for q in range(2):
        check(Pa[q], refs[q], f[..., q].size, f"32^3 one box, component {q}")
        check(Pb[q], refs[q], f[..., q].size, f"32^3 eight boxes, component {q}")
    assert Pa.tobytes() == Pb.tobytes() and np.array_equal(ca, cb) and np.array_equal(ca, refs[0][1])
    # the second component alone, without the counts
    out, nb = np.zeros(29), C.c_int()
    assert gpu.lib().iamrx_mf_spectrum(C.byref(g), eight.h, 1, 1, 29, out.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(nb)) == 0
    assert nb.value == 29 and out.tobytes() == Pa[1].tobytes()


def test_switches_keep_the_bits(gpu):
    """the two measurement switches of the transform change how the work is cut, not what is added to what: one
    butterfly stage per barrier instead of two, and every size of the LDS image, give the bits of the defaults"""
    cases = [((8, 16, 32), UNIT), ((1024, 4, 4), UNIT), ((4, 4, 1024), UNIT)]
    base = {}
    for n, L in cases:
        f, _ = reference(n, L)
        base[n] = (make_mf(n, f)[0], geom_of(n, L))
        base[n] += (gpu.mf_spectrum(base[n][1], base[n][0], 0, 1)[0].tobytes(),)
    try:
        for key, values, dflt in (("SPECTRUM_PAIR_STAGES", (0,), 1), ("SPECTRUM_TILE_ELEMS", (256, 1024, 4096), 2048)):
            for v in values:
                gpu.tuning_set(key, v)
                for n, (mf, g, want) in base.items():
                    assert gpu.mf_spectrum(g, mf, 0, 1)[0].tobytes() == want, (key, v, n)
            gpu.tuning_set(key, dflt)
    finally:
        gpu.tuning_set("SPECTRUM_PAIR_STAGES", 1)
        gpu.tuning_set("SPECTRUM_TILE_ELEMS", 2048)


def test_single_cosine_mode(gpu):
    """cos(2 pi (3 i + 4 j) / 16) at 16^3: P(5) = 1/2 within the bound, every other shell <= eps^2 P_tot"""
    n = (16, 16, 16)
    f = SN.cosine_mode(n)[..., None]
    mf, _ = make_mf(n, f)
    P, count = gpu.mf_spectrum(geom_of(n), mf, 0, 1)
    ref = SN.spectrum_reference(f[..., 0], UNIT)
    eps = SN.eps_of(16 ** 3)
    others = float(np.delete(P[0], 5).max())
    print(f"cosine mode: |P(5) - 1/2| = {abs(P[0][5] - 0.5):.3e} (bound {SN.bound(*ref, 16 ** 3)[5]:.3e}); largest other shell {others:.3e} (bound {eps * eps * 0.5:.3e})")
    assert abs(P[0][5] - 0.5) <= SN.bound(*ref, 16 ** 3)[5]
    assert others <= eps * eps * 0.5
    assert np.array_equal(count, ref[1])


def test_errors(gpu):
    from iamr_amd.lib import IamrxError
    f = SN.noise((24, 16, 16), 1)
    mf, _ = make_mf((24, 16, 16), f)
    with pytest.raises(IamrxError, match=r"n_x = 24"):                              # not a power of two: the message names the extent
        gpu.mf_spectrum(geom_of((24, 16, 16)), mf, 0, 1)
    n = (8, 16, 32)
    f, refs = reference(n, UNIT)
    mf, lay = make_mf(n, f)
    with pytest.raises(IamrxError, match="periodic"):
        gpu.mf_spectrum(geom_of(n, periodic=(1, 0, 1)), mf, 0, 1)
    with pytest.raises(IamrxError, match="component"):
        gpu.mf_spectrum(geom_of(n), mf, 1, 1)
    with pytest.raises(IamrxError, match="cover"):                                  # the array's one box is half of this domain
        gpu.mf_spectrum(geom_of((8, 16, 64)), mf, 0, 1)
    nbins = len(refs[0][0])
    out, nb = np.zeros(nbins), C.c_int()
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    g = geom_of(n)
    assert gpu.lib().iamrx_mf_spectrum(C.byref(g), mf.h, 0, 1, nbins - 1, ptr, None, C.byref(nb)) != 0       # capacity too small ...
    assert nb.value == nbins and not out.any()                                                                # ... *nbins all the same
    assert gpu.lib().iamrx_mf_spectrum(C.byref(g), mf.h, 0, 1, nbins, ptr, None, C.byref(nb)) == 0 and nb.value == nbins


# ------------------------------------------------------------------------------------------------------------------ 2. level, hierarchy
def state_dict_check(s, S, L, tag):
    """the dict of NavierStokes.spectrum / Amr.spectrum against the yardstick on the state S (n, >= 5): u v w . c"""
    n, N = S.shape[:3], S[..., 0].size
    refs = [SN.spectrum_reference(np.ascontiguousarray(S[..., q]), L) for q in (0, 1, 2, 4)]
    for key, ref in zip(("Euu", "Evv", "Eww", "Ecc"), refs):
        check(2.0 * s[key], ref, N, f"{tag} {key}")
    assert np.array_equal(s["E"], 0.5 * ((2.0 * s["Euu"] + 2.0 * s["Evv"]) + 2.0 * s["Eww"]))
    assert np.array_equal(s["count"], refs[0][1]) and int(s["count"].sum()) == N
    assert np.array_equal(s["k"], np.arange(len(s["E"])) * (2.0 * math.pi / max(L))) and s["n"] == tuple(n) and s["L"] == tuple(L)
    return refs


def test_level(gpu):
    """iamrx_ns_spectrum on a 16^3 level whose new-time state was set from outside: the four columns u, v, w, c"""
    from test_gpu_profile import random_state, one_level
    n = (16, 16, 16)
    S = random_state(n, 12)
    ns, lay = one_level(n, S, 8)
    s = ns.spectrum()
    state_dict_check(s, S, UNIT, "level 16^3")
    assert ns.spectrum()["E"].tobytes() == s["E"].tobytes()


def test_hierarchy(gpu):
    """iamrx_amr_spectrum on inputs.3d.taylorgreen_amr16 after one coarse step: the yardstick on level 0's state read back; the sum of E
    over the shells is the level-0 kinetic energy per volume of the same read-back (not sum_integrated's, which weights by rho)"""
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([AMR16]).problem()
    amr, lays, g0 = R.build_amr(pr, L, N)
    amr.post_init(pr["stop_time"])
    amr.coarse_step()
    n = tuple(amr.geom0.n)
    assert n == (16, 16, 16) and amr.nlev > 1
    s = amr.spectrum()
    S = amr.levels[0].data(amr.levels[0].S_NEW).gather_valid(n)
    Lside = tuple(amr.geom0.prob_hi[d] - amr.geom0.prob_lo[d] for d in range(3))
    refs = state_dict_check(s, S, Lside, "hierarchy level 0")
    ke = 0.5 * math.fsum((S[..., 0] ** 2 + S[..., 1] ** 2 + S[..., 2] ** 2).ravel()) / S[..., 0].size
    tol = 0.5 * sum(float(np.sum(SN.bound(P, c, S[..., 0].size))) for P, c in refs[:3])
    print(f"sum of E = {math.fsum(s['E']):.17g}, kinetic energy per volume of level 0 = {ke:.17g}, difference {abs(math.fsum(s['E']) - ke):.3e} (bound {tol:.3e})")
    assert ke > 0.0 and abs(math.fsum(s["E"]) - ke) <= tol


# ------------------------------------------------------------------------------------------------------------------ 3. driver
def test_driver_writes_the_files(gpu, tmp_path, monkeypatch):
    """inputs.3d.forced at 16^3, two steps with ns.spectrum_interval = 1: spec00000 .. spec00002 appear in the working directory and hold
    NavierStokes.spectrum of that moment bit for bit; without the key no file appears"""
    from iamr_amd import run as R
    from iamr_amd.spectrum import read_spectrum
    over = ["amr.n_cell=16 16 16", "max_step=2", "amr.derive_plot_vars=NONE"] + QUIET
    seen = {}

    def observe(ns, step, dt):
        seen[step] = (ns.time, ns.spectrum())

    d1 = tmp_path / "on"; d1.mkdir()
    monkeypatch.chdir(d1)
    assert R.main([FORCED, "ns.spectrum_interval=1"] + over, observe) == 0
    assert sorted(os.listdir(d1)) == ["spec00000", "spec00001", "spec00002"]
    for step in range(3):
        time, s = seen[step]
        r = read_spectrum(str(d1 / f"spec{step:05d}"))
        assert (r["step"], r["time"], r["n"]) == (step, time, (16, 16, 16)) and r["sum_E"] == math.fsum(s["E"]) > 0.0
        for k in ("k", "count", "E", "Euu", "Evv", "Eww", "Ecc"):
            assert r[k].tobytes() == s[k].tobytes(), (step, k)
    d2 = tmp_path / "off"; d2.mkdir()
    monkeypatch.chdir(d2)
    assert R.main([FORCED] + over) == 0
    assert os.listdir(d2) == []
