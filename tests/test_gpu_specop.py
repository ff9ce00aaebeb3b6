"""GPU: the way back from mode space (include/iamrx.h: iamrx_mf_noise / iamrx_mf_filter / iamrx_mf_solenoidal / iamrx_mf_synthesize;
kernels in iamr_amd/csrc/k_spectrum.hip) through the C-ABI against the numpy yardstick of tests/specop_numpy.py on the same data, inside
the bounds its docstring derives.  Every ghost cell holds NaN before a call and must hold it afterwards.  The shapes are the smallest
at which each path can go wrong: unequal extents, a non-cubic domain, one box against eight, the longest transform on each axis, a
row shorter than a wavefront."""
import functools
import math
import os
import numpy as np
import pytest
import spectrum_numpy as SN
import specop_numpy as SO
from test_gpu_spectrum import make_mf, geom_of, reference, UNIT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FORCED = os.path.join(GOLD, "inputs.3d.forced")
DECAY = os.path.join(GOLD, "inputs.3d.decay16")
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]
LONG = (1.0, 1.0, 2.0)


def nan_mf(n, ncomp, max_grid_size=None, ngrow=1):
    return make_mf(n, np.full(tuple(n) + (ncomp,), np.nan), max_grid_size, ngrow)


def all_nan(mf):
    return all(np.isnan(mf.to_numpy(li)[0]).all() for li in range(mf.nlocal()))


def ghosts_nan(mf, lay):
    """every cell outside the valid box of every fab is still NaN, and no valid cell is"""
    for li in range(mf.nlocal()):
        a, glo = mf.to_numpy(li)
        lo, hi, _ = lay.local_box(li)
        inside = np.zeros(a.shape[:3], dtype=bool)
        inside[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = True
        if not (np.isnan(a[~inside]).all() and not np.isnan(a[inside]).any()):
            return False
    return True


def valid(mf, n):
    return np.ascontiguousarray(mf.gather_valid(n))


@functools.lru_cache(maxsize=None)
def vector(n, seed=21):
    f = SO.noise(n, seed, 3) * 2.0 + np.array([0.3, -0.2, 0.1])
    f.setflags(write=False)
    return f


def diveru_rms(gpu, g, mf, lay, n):
    """rms over the cells of "diveru" of components 0 .. 2 of mf after a periodic ghost fill"""
    mf.fill_boundary(g)
    out = gpu.MultiFab(lay, gpu.CELL, 1, 0)
    gpu.derive_velgrad(g, out, mf, "diveru")
    return SO.norm2(valid(out, n)) / math.sqrt(n[0] * n[1] * n[2])


# ------------------------------------------------------------------------------------------------------------------ 1. noise
@pytest.mark.parametrize("mgs", [None, 8])
def test_noise_has_the_bits_of_the_generator(gpu, mgs):
    n = (8, 16, 32)
    mf, lay = nan_mf(n, 3, mgs)
    gpu.mf_noise(geom_of(n), mf, 9, comp=1, ncomp=2)
    got = valid(mf, n)
    assert got[..., 1:].tobytes() == np.ascontiguousarray(SO.noise(n, 9, 2)).tobytes()
    for li in range(mf.nlocal()):
        a, glo = mf.to_numpy(li)
        lo, hi, _ = lay.local_box(li)
        v = tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))
        assert np.isnan(a[..., 0]).all()                                   # the component in front is not touched
        keep = a[..., 1:].copy()
        keep[v] = np.nan
        assert np.isnan(keep).all() and not np.isnan(a[..., 1:][v]).any()   # ghost cells are not written


# ------------------------------------------------------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), LONG), ((1024, 4, 4), UNIT), ((4, 1024, 4), UNIT), ((4, 4, 1024), UNIT),
                                 ((64, 4, 4), UNIT)])
def test_round_trip(gpu, n, L):
    f, _ = reference(n, L)
    src, _ = make_mf(n, f)
    dst, lay = nan_mf(n, 1)
    g = geom_of(n, L)
    gpu.mf_filter(g, dst, src, "identity", 1.0)
    got = valid(dst, n)
    err, bd = SO.norm2(got[..., 0] - f[..., 0]), SO.filter_bound(f[..., 0])
    print(f"{n} L {L}: ||round trip - f|| = {err:.3e}, bound {bd:.3e}, ratio {err / bd:.4f}")
    assert err <= bd
    assert ghosts_nan(dst, lay)
    gpu.mf_filter(g, dst, src, "identity", 1.0)
    assert valid(dst, n).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 3. filters
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), LONG)])
def test_filter_kinds(gpu, n, L):
    f, refs = reference(n, L)
    N = f[..., 0].size
    src, _ = make_mf(n, f)
    dst, lay = nan_mf(n, 1)
    g = geom_of(n, L)
    bd = SO.filter_bound(f[..., 0])
    for kind, kc in (("sharp", 4.5), ("gaussian", 3.0), ("box", 3.0), ("gaussian", 0.75), ("box", 11.0)):
        gpu.mf_filter(g, dst, src, kind, kc)
        ref = SO.filter_reference(f[..., 0], L, SO_KIND[kind], kc)
        err = SO.norm2(valid(dst, n)[..., 0] - ref)
        print(f"{n} {kind} kc {kc}: ||got - yardstick|| = {err:.3e}, bound {bd:.3e}, ratio {err / bd:.4f}; ||filtered|| / ||f|| = {SO.norm2(ref) / SO.norm2(f):.4f}")
        assert err <= bd and ghosts_nan(dst, lay)
    # sharp: the spectrum of the result is the input's up to shell 4 (kappa < 4.5 <=> s <= 4) and nothing beyond
    gpu.mf_filter(g, dst, src, 1, 4.5)
    P, count = refs[0]
    got, _ = gpu.mf_spectrum(g, dst, 0, 1)
    eps = SN.eps_of(N) + SO.filter_eps(N)
    sb = SO.shell_bound(P, count, eps)
    print(f"{n} sharp: below the cut worst error / bound {float(np.max(np.abs(got[0][:5] - P[:5]) / sb[:5])):.4f}; "
          f"largest shell above {float(got[0][5:].max()):.3e} (bound {eps * eps * math.fsum(P):.3e})")
    assert np.all(np.abs(got[0][:5] - P[:5]) <= sb[:5])
    assert float(got[0][5:].max()) <= eps * eps * math.fsum(P)


SO_KIND = {"identity": 0, "sharp": 1, "gaussian": 2, "box": 3}


def test_filter_scales_a_cosine_mode(gpu):
    """cos(2 pi (3 i + 4 j) / 16) at 16^3, kappa = 5: the Gaussian and the box return it scaled by the analytic G"""
    n = (16, 16, 16)
    f = SN.cosine_mode(n)
    src, _ = make_mf(n, f[..., None])
    dst, _ = nan_mf(n, 1)
    g = geom_of(n)
    kc = 4.0
    sinc = lambda x: math.sin(x) / x
    for kind, G in (("gaussian", math.exp(-25.0 * math.pi ** 2 / (24.0 * kc * kc))), ("box", sinc(3.0 * math.pi / (2.0 * kc)) * sinc(4.0 * math.pi / (2.0 * kc)))):
        gpu.mf_filter(g, dst, src, kind, kc)
        err = SO.norm2(valid(dst, n)[..., 0] - G * f)
        print(f"cosine mode, {kind}: G = {G:.6f}, ||got - G f|| = {err:.3e}, bound {SO.filter_bound(f):.3e}")
        assert 0.05 < G < 0.95 and err <= SO.filter_bound(f)


def test_filter_one_box_against_eight_and_in_place(gpu):
    n = (32, 32, 32)
    f, _ = reference(n, UNIT, 7, 2)
    g = geom_of(n)
    one, _ = make_mf(n, f)
    eight, lay8 = make_mf(n, f, 16)
    assert len(lay8.boxes) == 8
    d1, _ = nan_mf(n, 2)
    d8, _ = nan_mf(n, 2, 16)
    gpu.mf_filter(g, d1, one, "gaussian", 5.0, ncomp=2)
    gpu.mf_filter(g, d8, eight, "gaussian", 5.0, ncomp=2)
    a = valid(d1, n)
    assert a.tobytes() == valid(d8, n).tobytes()
    for q in range(2):
        assert SO.norm2(a[..., q] - SO.filter_reference(f[..., q], UNIT, 2, 5.0)) <= SO.filter_bound(f[..., q])
    gpu.mf_filter(g, d1, eight, "gaussian", 5.0, ncomp=2)                 # from eight boxes into one: different layouts of one domain
    assert valid(d1, n).tobytes() == a.tobytes()
    gpu.mf_filter(g, eight, eight, "gaussian", 5.0, ncomp=2)              # dst is src
    assert valid(eight, n).tobytes() == a.tobytes() and ghosts_nan(eight, lay8)
    gpu.mf_filter(g, one, one, "gaussian", 5.0, dcomp=1, scomp=0, ncomp=1)   # one array, component 0 into component 1
    b = valid(one, n)
    assert b[..., 1].tobytes() == a[..., 0].tobytes() and b[..., 0].tobytes() == np.ascontiguousarray(f[..., 0]).tobytes()


# ------------------------------------------------------------------------------------------------------------------ 4. projection
def test_solenoidal(gpu):
    n, L = (16, 16, 32), LONG
    N = n[0] * n[1] * n[2]
    f = vector(n)
    g = geom_of(n, L)
    src, _ = make_mf(n, f, 16)
    cen, layc = nan_mf(n, 3, 16)
    exa, laye = nan_mf(n, 3)
    gpu.mf_solenoidal(g, cen, src, "centred")
    gpu.mf_solenoidal(g, exa, src, "exact")
    assert ghosts_nan(cen, layc) and ghosts_nan(exa, laye)
    uc, ue = valid(cen, n), valid(exa, n)
    pb = SO.projection_bound(f)
    for got, wn in ((ue, 0), (uc, 1)):
        err = SO.norm2(got - SO.solenoidal_reference(f, L, wn))
        print(f"projection form {wn}: ||got - yardstick|| = {err:.3e}, bound {pb:.3e}, ratio {err / pb:.4f}")
        assert err <= pb
    db = SO.divergence_bound(f, uc, L)
    dc, de = diveru_rms(gpu, g, cen, layc, n), diveru_rms(gpu, g, exa, laye, n)
    print(f"rms diveru: centred {dc:.3e} (bound {db:.3e}, ratio {dc / db:.4f}), exact {de:.3e}")
    assert dc <= db and de > 1000.0 * db
    # twice changes nothing; the exact projection of the centred field removes what the yardstick's mode-by-mode expression says
    again, _ = nan_mf(n, 3)
    gpu.mf_solenoidal(g, again, cen, "centred")
    assert SO.norm2(valid(again, n) - uc) <= pb
    gpu.mf_solenoidal(g, again, exa, 0)
    assert SO.norm2(valid(again, n) - ue) <= pb
    gpu.mf_solenoidal(g, again, cen, "exact")
    removed, want = SO.norm2(valid(again, n) - uc), SO.cross_removed(uc, L, 0)
    print(f"the exact projection removes {removed:.6e} from the centred field, the yardstick says {want:.6e}")
    assert want > 1e-3 * SO.norm2(uc) and abs(removed - want) <= pb
    # a pure gradient comes back zero: the centred difference of a potential for `centred`, i k phi for `exact`
    phi = SO.noise(n, 5, 1)[..., 0]
    dx = [L[d] / n[d] for d in range(3)]
    grad_c = np.stack([(np.roll(phi, -1, d) - np.roll(phi, 1, d)) * (0.5 / dx[d]) for d in range(3)], axis=-1)
    q = SO.wave_vector(n, L, 0)
    grad_e = np.stack([np.fft.ifftn(1j * q[d] * np.fft.fftn(phi)).real for d in range(3)], axis=-1)
    for grad, wn in ((grad_c, "centred"), (grad_e, "exact")):
        gm, _ = make_mf(n, grad)
        gpu.mf_solenoidal(g, again, gm, wn)
        left = SO.norm2(valid(again, n))
        print(f"gradient field, {wn}: ||projected|| = {left:.3e}, bound {SO.projection_bound(grad):.3e}")
        assert left <= SO.projection_bound(grad)


# ------------------------------------------------------------------------------------------------------------------ 5. synthesis
@pytest.mark.parametrize("n,L", [((16, 16, 16), UNIT), ((16, 16, 32), LONG)])
def test_synthesis(gpu, n, L):
    from iamr_amd.spectral import hit_spectrum
    from iamr_amd.spectrum import nbins_of
    N = n[0] * n[1] * n[2]
    nbins = nbins_of(n, L)
    E = hit_spectrum(nbins, L, 3.0, 1.0, n=n)
    g = geom_of(n, L)
    dst, lay = nan_mf(n, 4)
    gpu.mf_synthesize(g, dst, E, seed=42, wavenumber="centred", comp=1)
    got = valid(dst, n)
    assert ghosts_nan_comp(dst, lay, 1, 3)
    u = np.ascontiguousarray(got[..., 1:])
    ref, info = SO.synth_reference(n, L, 42, E, 1)
    err, bd = SO.norm2(u - ref) / math.sqrt(N), SO.synth_field_bound(E, info, N)
    print(f"{n}: rms(got - yardstick) = {err:.3e}, bound {bd:.3e}, ratio {err / bd:.4f}")
    assert err <= bd
    vel, layv = nan_mf(n, 3, 8)
    gpu.mf_synthesize(g, vel, E, 42, "centred")
    assert valid(vel, n).tobytes() == u.tobytes() and len(layv.boxes) >= 8          # one box and eight (or more): the same bits
    P, count = gpu.mf_spectrum(g, vel, 0, 3)
    Eg = 0.5 * ((P[0] + P[1]) + P[2])
    sb = SO.synth_spectrum_bound(E, info, N)
    print(f"{n}: spectrum of the result: worst |E - E_target| / bound = {float(np.max(np.abs(Eg - E) / sb)):.4f}; E(0) = {Eg[0]:.3e} (bound {sb[0]:.3e}); "
          f"sum E = {math.fsum(Eg):.15g}")
    assert np.all(np.abs(Eg - E) <= sb) and Eg[0] <= sb[0]
    d, db = diveru_rms(gpu, g, vel, layv, n), SO.synth_divergence_bound(E, info, u, L)
    print(f"{n}: rms diveru = {d:.3e}, bound {db:.3e}")
    assert d <= db
    gpu.mf_synthesize(g, dst, E, 42, "centred", 1)
    assert valid(dst, n)[..., 1:].tobytes() == u.tobytes()                           # the same seed: the same bits
    gpu.mf_synthesize(g, dst, E, 43, "centred", 1)
    other = valid(dst, n)[..., 1:]
    assert SO.norm2(other - u) > 0.5 * SO.norm2(u)                                   # another seed: another field
    gpu.mf_synthesize(g, dst, E, 42, "exact", 1)
    ex = np.ascontiguousarray(valid(dst, n)[..., 1:])
    refx, infox = SO.synth_reference(n, L, 42, E, 0)
    assert SO.norm2(ex - refx) / math.sqrt(N) <= SO.synth_field_bound(E, infox, N)


def ghosts_nan_comp(mf, lay, c0, nc):
    """components c0 .. c0 + nc - 1 hold numbers in the valid cells and NaN in the ghost cells; every other component is NaN everywhere"""
    for li in range(mf.nlocal()):
        a, glo = mf.to_numpy(li)
        lo, hi, _ = lay.local_box(li)
        v = tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))
        w = a[..., c0:c0 + nc].copy()
        if np.isnan(w[v]).any():
            return False
        w[v] = np.nan
        rest = np.delete(a, np.s_[c0:c0 + nc], axis=3)
        if not (np.isnan(w).all() and np.isnan(rest).all()):
            return False
    return True


def test_synthesis_refuses_an_empty_shell(gpu):
    """4^3 cells on a 1 x 1 x 4 box: shell 3 holds no mode (test_cpu_specop.py); energy asked for there is an error, dst stays as it was"""
    from iamr_amd.lib import IamrxError
    n, L = (4, 4, 4), (1.0, 1.0, 4.0)
    s, nbins, _ = SN.shell_index(n, L)
    g = geom_of(n, L)
    dst, lay = nan_mf(n, 3)
    E = np.zeros(nbins)
    E[2] = 1.0
    E[3] = 1.0
    with pytest.raises(IamrxError, match="shell 3"):
        gpu.mf_synthesize(g, dst, E, 1, "centred")
    assert all_nan(dst)
    E[3] = 0.0
    gpu.mf_synthesize(g, dst, E, 1, "centred")
    ref, info = SO.synth_reference(n, L, 1, E, 1)
    assert SO.norm2(valid(dst, n) - ref) / 8.0 <= SO.synth_field_bound(E, info, 64)


# ------------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors_leave_dst_untouched(gpu):
    from iamr_amd.lib import IamrxError
    from iamr_amd.spectrum import nbins_of
    n = (8, 16, 32)
    f = vector(n)
    src, _ = make_mf(n, f)
    dst, _ = nan_mf(n, 3)
    g = geom_of(n)
    E = np.zeros(nbins_of(n, UNIT))
    E[2] = 1.0

    def each(gm, d=dst, s=src):
        return (lambda: gpu.mf_filter(gm, d, s, 2, 3.0), lambda: gpu.mf_solenoidal(gm, d, s, 1), lambda: gpu.mf_synthesize(gm, d, E, 1, 1))

    for call in each(geom_of(n, periodic=(1, 0, 1))):
        with pytest.raises(IamrxError, match="periodic"):
            call()
    m12 = (12, 16, 16)
    s12, _ = make_mf(m12, SN.noise(m12, 1, 3))
    d12, _ = nan_mf(m12, 3)
    for call in each(geom_of(m12), d12, s12):
        with pytest.raises(IamrxError, match=r"n_x = 12"):
            call()
    assert all_nan(d12)
    nodal = gpu.MultiFab(gpu.Layout.single(n), gpu.NODE, 3, 1)
    for call in (lambda: gpu.mf_filter(g, nodal, src, 2, 3.0), lambda: gpu.mf_filter(g, dst, nodal, 2, 3.0), lambda: gpu.mf_solenoidal(g, nodal, src, 1),
                 lambda: gpu.mf_synthesize(g, nodal, E, 1, 1), lambda: gpu.mf_noise(g, nodal, 1)):
        with pytest.raises(IamrxError, match="cell-centred"):
            call()
    for call in (lambda: gpu.mf_filter(g, dst, src, 2, 3.0, dcomp=2, ncomp=2), lambda: gpu.mf_filter(g, dst, src, 2, 3.0, scomp=3),
                 lambda: gpu.mf_filter(g, dst, src, 2, 3.0, ncomp=0), lambda: gpu.mf_solenoidal(g, dst, src, 1, dcomp=1),
                 lambda: gpu.mf_solenoidal(g, dst, src, 1, scomp=-1), lambda: gpu.mf_synthesize(g, dst, E, 1, 1, comp=1), lambda: gpu.mf_noise(g, dst, 1, 2, 2)):
        with pytest.raises(IamrxError, match="component"):
            call()
    with pytest.raises(IamrxError, match="cover"):
        gpu.mf_filter(geom_of((8, 16, 64)), dst, src, 2, 3.0)
    for kind in (-1, 4):
        with pytest.raises(IamrxError, match="kind"):
            gpu.mf_filter(g, dst, src, kind, 3.0)
    for wn in (-1, 2):
        with pytest.raises(IamrxError, match="wavenumber"):
            gpu.mf_solenoidal(g, dst, src, wn)
        with pytest.raises(IamrxError, match="wavenumber"):
            gpu.mf_synthesize(g, dst, E, 1, wn)
    for kc in (0.0, -1.0, float("nan"), float("inf")):
        for kind in (0, 1, 2, 3):
            with pytest.raises(IamrxError, match="kc"):
                gpu.mf_filter(g, dst, src, kind, kc)
    with pytest.raises(IamrxError, match="shells"):
        gpu.mf_synthesize(g, dst, E[:-1], 1, 1)
    with pytest.raises(IamrxError, match="negative"):
        gpu.mf_synthesize(g, dst, -E, 1, 1)
    with pytest.raises(ValueError):
        gpu.mf_filter(g, dst, src, "tophat", 3.0)
    assert all_nan(dst)
    assert valid(src, n).tobytes() == np.ascontiguousarray(f).tobytes()


# ------------------------------------------------------------------------------------------------------------------ 7. level, driver
def test_level_filtered(gpu):
    """NavierStokes.filtered on the level of inputs.3d.forced at 16^3 is mf_filter of derive_fields of the same names, to the bit"""
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    inp = Inputs([FORCED], ["amr.n_cell=16 16 16", "amr.derive_plot_vars=NONE"] + QUIET)
    ns, lay, g, pr = R.build(inp, gpu, N)
    ns.post_init(pr["stop_time"])
    names = ["x_velocity", "enstrophy"]
    F = ns.filtered(names, kind=2, kc=4)
    D = ns.derive_fields(names)
    out = gpu.MultiFab(lay, gpu.CELL, 2, 0)
    gpu.mf_filter(ns.geom, out, D, "gaussian", 4.0, ncomp=2)
    n = (16, 16, 16)
    a, b, d = valid(F, n), valid(out, n), valid(D, n)
    assert a.shape == (16, 16, 16, 2) and a.tobytes() == b.tobytes()
    for q in range(2):
        assert 0.0 < SO.norm2(a[..., q]) < SO.norm2(d[..., q])
        assert SO.norm2(a[..., q] - SO.filter_reference(d[..., q], UNIT, 2, 4.0)) <= SO.filter_bound(d[..., q])


def test_driver_decaying_box(gpu, tmp_path, monkeypatch):
    """python -m iamr_amd.run tests/golden/inputs.3d.decay16, in this process: it finishes; the spectrum file of step 0 holds 3/2 urms0^2
    within 1 % (the synthesised field is solenoidal for the centred difference, so the initial projection has little to remove); the
    kinetic energy of the spectrum files decreases from step to step"""
    from iamr_amd import run as R
    from iamr_amd.spectrum import read_spectrum
    monkeypatch.chdir(tmp_path)
    seen = {}

    def observe(ns, step, dt):
        seen[step] = ns.spectrum()

    assert R.main([DECAY], observe) == 0
    files = sorted(os.listdir(tmp_path))
    assert files == [f"spec{q:05d}" for q in range(5)], files
    sums = [read_spectrum(str(tmp_path / f))["sum_E"] for f in files]
    print("sum_E of the steps:", " ".join(f"{v:.12g}" for v in sums), f"; step 0 against 3/2: {abs(sums[0] - 1.5) / 1.5:.3e}")
    assert sums[0] == math.fsum(seen[0]["E"])
    assert abs(sums[0] - 1.5) <= 0.01 * 1.5
    assert all(b < a for a, b in zip(sums, sums[1:]))
    assert seen[0]["E"][0] <= 1e-20 and int(np.argmax(seen[0]["E"])) == 3
