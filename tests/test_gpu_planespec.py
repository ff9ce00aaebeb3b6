"""GPU: plane spectra, the ring-summed 2-D spectra along a normal axis (include/iamrx.h: iamrx_mf_plane_spectrum /
iamrx_mf_plane_cospectrum / iamrx_ns_plane_spectrum / iamrx_amr_plane_spectrum; kernels in iamr_amd/csrc/k_spectrum.hip) through the
C-ABI against the numpy yardstick of tests/planespec_numpy.py on the same data.

The yardstick is np.fft.fftn over the two axes of the plane / M with math.fsum per (plane, ring); the tolerance is its derived bound
|dP(p, s)| <= 2 eps sqrt(P(p, s) P_tot(p)) + eps^2 P_tot(p) + count(s) 2^-53 P(p, s), eps = 16 log2(M) 2^-53.  The data are white noise
of order one with a non-zero mean; every ghost cell holds NaN, also those beyond a wall.  The shapes (planespec_numpy.SHAPES) are the
smallest at which each path can go wrong: normal extents that are no power of two, odd or one, non-unit ratios, the longest transform
on each axis, a row of exactly one wavefront, more planes than a wavefront has lanes and one plane past a wavefront."""
import ctypes as C
import functools
import math
import os
import numpy as np
import pytest
import planespec_numpy as PS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT16 = os.path.join(ROOT, "tests", "golden", "inputs.3d.rayleightaylor_planes16")
U3 = PS.U3
PER_DIR = {2: ((8, 16, 6), U3), 1: ((8, 6, 16), U3), 0: ((6, 8, 16), U3)}          # one shape per direction for the layout tests


@functools.lru_cache(maxsize=None)
def reference(n, L, dir, seed=3):
    """(f (n, 1), (P, count)): computed once per shape and shared, never written to"""
    f = PS.noise(n, seed)
    f.setflags(write=False)
    return f, PS.plane_spectrum_reference(f[..., 0], L, dir)


def unequal_boxes(n):
    """the domain cut once along every axis that has two cells or more, away from the middle: up to eight boxes of unequal sizes"""
    cuts = [[0, n[d]] if n[d] < 2 else [0, max(1, (3 * n[d]) // 8), n[d]] for d in range(3)]
    return [((cuts[0][i], cuts[1][j], cuts[2][k]), (cuts[0][i + 1] - 1, cuts[1][j + 1] - 1, cuts[2][k + 1] - 1))
            for k in range(len(cuts[2]) - 1) for j in range(len(cuts[1]) - 1) for i in range(len(cuts[0]) - 1)]


def make_mf(n, f, boxes=None, ngrow=1):
    """a cell-centred MultiFab over the domain: f on the valid cells of every box, NaN in ALL ghost cells"""
    from iamr_amd import lib as L
    lay = L.Layout.single(n) if boxes is None else L.Layout(boxes)
    mf = L.MultiFab(lay, L.CELL, f.shape[3], ngrow)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (f.shape[3],), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    return mf, lay


def geom_of(n, L=U3, periodic=(1, 1, 1)):
    from iamr_amd import lib
    return lib.Geom.make(list(n), prob_hi=tuple(L), periodic=periodic)


def check(got, ref, M, tag):
    """got (nplanes, nrings) against the yardstick's (P, count); prints the largest error in units of the bound"""
    P, count = ref
    bd = PS.bound(P, count, M)
    assert got.shape == P.shape, (tag, got.shape, P.shape)
    err = np.abs(got - P)
    worst = float(np.max(err / bd))
    print(f"{tag}: {P.shape[0]} planes of {P.shape[1]} rings, max |got - yardstick| = {float(err.max()):.3e}, worst error / bound = {worst:.4f}")
    assert np.all(err <= bd), (tag, worst)
    return worst


def plane_count(n, dir):
    a, b = PS.axes_of(dir)
    return n[a] * n[b]


# ------------------------------------------------------------------------------------------------------------------ 1. one array
@pytest.mark.parametrize("n,L,dir", PS.SHAPES)
def test_one_box(gpu, n, L, dir):
    """every shape against the yardstick; count is the yardstick's exactly and sums to M; Parseval per plane; the same bits again"""
    f, ref = reference(n, L, dir)
    M = plane_count(n, dir)
    mf, _ = make_mf(n, f)
    g = geom_of(n, L)
    P, count = gpu.mf_plane_spectrum(g, mf, dir, 0, 1)
    assert P.shape == (1,) + ref[0].shape
    check(P[0], ref, M, f"{n} L {L} dir {dir}")
    assert count.dtype == np.int64 and np.array_equal(count, ref[1]) and int(count.sum()) == M
    fp = np.moveaxis(f[..., 0], dir, 0)
    for p in range(n[dir]):
        msq = math.fsum((fp[p] * fp[p]).ravel()) / M
        assert abs(math.fsum(P[0][p]) - msq) <= PS.eps_of(M) * msq, (p, math.fsum(P[0][p]), msq)
    P2, count2 = gpu.mf_plane_spectrum(g, mf, dir, 0, 1)
    assert P2.tobytes() == P.tobytes() and np.array_equal(count2, count)


@pytest.mark.parametrize("dir", [2, 1, 0])
def test_one_box_against_unequal_boxes(gpu, dir):
    """one box and up to eight boxes of unequal sizes, cut along every axis (the normal one too), two components: both inside the bound
    and equal to the bit (only the pack sees the boxes)"""
    n, L = PER_DIR[dir]
    f = PS.noise(n, 7, 2)
    refs = [PS.plane_spectrum_reference(f[..., q], L, dir) for q in range(2)]
    boxes = unequal_boxes(n)
    assert len(boxes) == 8 and len({tuple(h[d] - l[d] for d in range(3)) for l, h in boxes}) == 8
    g = geom_of(n, L)
    one, _ = make_mf(n, f)
    many, _ = make_mf(n, f, boxes)
    Pa, ca = gpu.mf_plane_spectrum(g, one, dir, 0, 2)
    Pb, cb = gpu.mf_plane_spectrum(g, many, dir, 0, 2)
    for q in range(2):
        check(Pa[q], refs[q], plane_count(n, dir), f"dir {dir} one box, component {q}")
        check(Pb[q], refs[q], plane_count(n, dir), f"dir {dir} eight boxes, component {q}")
    assert Pa.tobytes() == Pb.tobytes() and np.array_equal(ca, cb) and np.array_equal(ca, refs[0][1])


@pytest.mark.parametrize("dir,n", [(2, (16, 16, 5)), (1, (16, 5, 16)), (0, (5, 16, 16))])
def test_cosine_planes(gpu, dir, n):
    """f = A(p) cos(2 pi (3 x_a + 4 x_b) / 16) with a different amplitude in every plane: P(p, 5) = A(p)^2 / 2, every other ring inside the
    bound of zero -- a plane reversal or an axis mix-up shows"""
    amp = 1.0 + 0.5 * np.arange(5)
    f = PS.cosine_planes(n, dir, amp)[..., None]
    mf, _ = make_mf(n, f)
    P, count = gpu.mf_plane_spectrum(geom_of(n), mf, dir, 0, 1)
    exact = np.zeros((5, len(count)))
    exact[:, 5] = 0.5 * amp * amp
    bd = PS.bound(exact, count, 256)
    err = np.abs(P[0] - exact)
    print(f"dir {dir}: |P(p, 5) - A^2 / 2| = {err[:, 5]} (bound {bd[:, 5]}); largest other ring {float(np.delete(err, 5, axis=1).max()):.3e} (bound {float(bd[:, 0].min()):.3e})")
    assert np.all(err <= bd)
    assert np.array_equal(count, PS.plane_spectrum_reference(f[..., 0], U3, dir)[1])


# ------------------------------------------------------------------------------------------------------------------ 2. co-spectrum
@pytest.mark.parametrize("dir", [2, 1, 0])
def test_cospectrum(gpu, dir):
    """two noise fields on different layouts through one packed transform: C_ab inside the per-plane co-spectrum bound of the yardstick,
    its sum over the rings the plane mean of a b, P_a and P_b inside the bound of the plain call's values"""
    n, L = PER_DIR[dir]
    M = plane_count(n, dir)
    f = PS.noise(n, 11, 2)
    fa, fb = np.ascontiguousarray(f[..., 0]), np.ascontiguousarray(f[..., 1])
    Cr, Par, Pbr, cr = PS.plane_cospectrum_reference(fa, fb, L, dir)
    g = geom_of(n, L)
    A, _ = make_mf(n, f[..., 0:1])
    B, _ = make_mf(n, f[..., 1:2], unequal_boxes(n))
    Cab, Pa, Pb, count = gpu.mf_plane_cospectrum(g, A, B, dir, 0, 0)
    bd = PS.cospectrum_bound(Par, Pbr, cr, M)
    err = np.abs(Cab - Cr)
    print(f"dir {dir}: co-spectrum worst error / bound = {float(np.max(err / bd)):.4f}")
    assert Cab.shape == Cr.shape and np.all(err <= bd) and np.array_equal(count, cr)
    ap, bp = np.moveaxis(fa, dir, 0), np.moveaxis(fb, dir, 0)
    for p in range(n[dir]):
        mab = math.fsum((ap[p] * bp[p]).ravel()) / M
        assert abs(math.fsum(Cab[p]) - mab) <= float(np.sum(bd[p])), (p, math.fsum(Cab[p]), mab)
    Pplain_a, _ = gpu.mf_plane_spectrum(g, A, dir, 0, 1)
    Pplain_b, _ = gpu.mf_plane_spectrum(g, B, dir, 0, 1)
    for got, plain, tag in ((Pa, Pplain_a[0], "P_a"), (Pb, Pplain_b[0], "P_b")):
        b2 = PS.bound(plain, count, M)
        worst = float(np.max(np.abs(got - plain) / b2))
        print(f"dir {dir}: {tag} of the packed pair against the plain call: worst difference / bound = {worst:.4f}")
        assert np.all(np.abs(got - plain) <= b2), (tag, worst)
    C2 = gpu.mf_plane_cospectrum(g, A, B, dir, 0, 0)[0]
    assert C2.tobytes() == Cab.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 3. walls, errors
@pytest.mark.parametrize("dir", [2, 1, 0])
def test_normal_direction_need_not_be_periodic(gpu, dir):
    """walls along the normal direction are accepted, and the same data with that direction declared periodic give the same bits"""
    n, L = PER_DIR[dir]
    f, ref = reference(n, L, dir)
    mf, _ = make_mf(n, f)
    walls = [1, 1, 1]
    walls[dir] = 0
    Pw, cw = gpu.mf_plane_spectrum(geom_of(n, L, tuple(walls)), mf, dir, 0, 1)
    Pp, cp = gpu.mf_plane_spectrum(geom_of(n, L), mf, dir, 0, 1)
    check(Pw[0], ref, plane_count(n, dir), f"dir {dir}, walls along the normal")
    assert Pw.tobytes() == Pp.tobytes() and np.array_equal(cw, cp)


def test_errors(gpu):
    from iamr_amd.lib import IamrxError
    from iamr_amd import lib as L
    n = (8, 16, 6)
    f, ref = reference(n, U3, 2)
    mf, lay = make_mf(n, f)
    g = geom_of(n)
    with pytest.raises(IamrxError, match=r"dir = 3 outside 0 .. 2"):
        gpu.mf_plane_spectrum(g, mf, 3, 0, 1)
    with pytest.raises(IamrxError, match=r"dir = -1 outside 0 .. 2"):
        gpu.mf_plane_cospectrum(g, mf, mf, -1, 0, 0)
    nodal = L.MultiFab(lay, L.NODE, 1, 0)
    with pytest.raises(IamrxError, match="not cell-centred"):
        gpu.mf_plane_spectrum(g, nodal, 2, 0, 1)
    with pytest.raises(IamrxError, match="component 1 outside 0 .. 0"):
        gpu.mf_plane_spectrum(g, mf, 2, 1, 1)
    with pytest.raises(IamrxError, match="component"):
        gpu.mf_plane_cospectrum(g, mf, mf, 2, 0, 3)
    with pytest.raises(IamrxError, match=r"direction y is not periodic"):               # the message names the axis
        gpu.mf_plane_spectrum(geom_of(n, periodic=(1, 0, 1)), mf, 2, 0, 1)
    with pytest.raises(IamrxError, match=r"direction z is not periodic"):
        gpu.mf_plane_spectrum(geom_of(n, periodic=(1, 1, 0)), mf, 1, 0, 1)
    with pytest.raises(IamrxError, match=r"n_z = 6 is not a power of two"):             # z is transformed when the normal is x
        gpu.mf_plane_spectrum(g, mf, 0, 0, 1)
    with pytest.raises(IamrxError, match="no length"):
        gpu.mf_plane_spectrum(L.Geom.make(list(n), prob_hi=(1.0, 0.0, 1.0)), mf, 2, 0, 1)
    big = (1024, 4, 1)
    fb = PS.noise(big, 1)
    mfb, _ = make_mf(big, fb)
    with pytest.raises(IamrxError, match="more than 2048 rings"):                        # r_x = 8: kappa(-512, -2) = 4096
        gpu.mf_plane_spectrum(geom_of(big, (1.0, 8.0, 1.0)), mfb, 2, 0, 1)
    with pytest.raises(IamrxError, match="cover"):                                       # the array's one box is half of this domain
        gpu.mf_plane_spectrum(geom_of((8, 16, 12)), mf, 2, 0, 1)
    npl, nr = ref[0].shape
    out, a, b = np.zeros(npl * nr), C.c_int(), C.c_int()
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    f_ = gpu.lib().iamrx_mf_plane_spectrum
    assert f_(C.byref(g), mf.h, 0, 1, 2, npl, nr - 1, ptr, None, C.byref(a), C.byref(b)) != 0            # capacity too small ...
    assert (a.value, b.value) == (npl, nr) and not out.any()                                               # ... both counts all the same
    a.value = b.value = 0
    assert f_(C.byref(g), mf.h, 0, 1, 2, npl - 1, nr, ptr, None, C.byref(a), C.byref(b)) != 0 and (a.value, b.value) == (npl, nr)
    assert f_(C.byref(g), mf.h, 0, 1, 2, npl, nr, ptr, None, C.byref(a), C.byref(b)) == 0                  # count may be NULL
    assert out.reshape(npl, nr).tobytes() == gpu.mf_plane_spectrum(g, mf, 2, 0, 1)[0][0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 4. level, driver
def test_driver_level_and_hierarchy(gpu, tmp_path, monkeypatch):
    """inputs.3d.rayleightaylor_planes16 (periodic in x and y, slip walls in z) with ns.plane_spectrum_interval = 1: a pspec file for
    step 0 and for every step; the last one holds NavierStokes.plane_spectrum(2) of that moment bit for bit; against plane_profile(2),
    sum_s Euu(p, s) = uu(p) / 2 and Euu(p, 0) = u(p)^2 / 2 within the Parseval bound plus the profile's own summation error M 2^-53 times
    the value; a one-level hierarchy gives the bits of its level"""
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    from iamr_amd.planespec import read_plane_spectrum, COLUMNS
    seen = {}

    def observe(ns, step, dt):
        seen[step] = (ns.time, ns.plane_spectrum(2), ns.plane_profile(2))

    monkeypatch.chdir(tmp_path)
    assert R.main([RT16, "ns.plane_spectrum_interval=1"], observe) == 0
    last = max(seen)
    assert last >= 1 and sorted(os.listdir(tmp_path)) == [f"pspec{s:05d}" for s in range(last + 1)]
    time, s, prof = seen[last]
    r = read_plane_spectrum(str(tmp_path / f"pspec{last:05d}"))
    assert (r["step"], r["time"], r["n"], r["dir"]) == (last, time, (16, 16, 32), 2) and r["sum_E"] == math.fsum(s["E"].ravel())
    for k in ("k", "count", "coord") + COLUMNS:
        assert r[k].tobytes() == s[k].tobytes(), k
    assert s["E"].shape == (32, PS.ring_index((16, 16, 32), (26.75, 26.75, 53.5), 2)[1]) and int(s["count"].sum()) == 256
    assert np.array_equal(s["coord"], prof["coord"])
    M, eps = 256, PS.eps_of(256)
    for p in range(32):
        uu, u = float(prof["uu"][p]), float(prof["u"][p])
        tol, tol0 = 0.5 * eps * uu + M * 2.0 ** -53 * 0.5 * uu, 0.5 * eps * uu + M * 2.0 ** -53 * 0.5 * u * u
        assert abs(math.fsum(s["Euu"][p]) - 0.5 * uu) <= tol, (p, math.fsum(s["Euu"][p]), 0.5 * uu, tol)
        assert abs(s["Euu"][p, 0] - 0.5 * u * u) <= tol0, (p, s["Euu"][p, 0], 0.5 * u * u, tol0)
    assert float(s["Err"][:, 0].min()) > 0.0 and float(s["Euu"].max()) > 0.0          # the flow has started: the spectra are not empty
    # a one-level hierarchy of the same file: Amr.plane_spectrum is the call of its level 0
    pr = Inputs([RT16]).problem()
    amr, lays, g0 = R.build_amr(pr, L, N)
    amr.post_init(pr["stop_time"])
    a, l0 = amr.plane_spectrum(2), amr.levels[0].plane_spectrum(2)
    for k in ("k", "count", "coord") + COLUMNS:
        assert a[k].tobytes() == l0[k].tobytes(), k
    assert a["E"].shape == s["E"].shape
