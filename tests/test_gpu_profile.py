"""GPU: plane-averaged profiles along one axis (include/iamrx.h: iamrx_ns_plane_profile / iamrx_amr_plane_profile; kernels in
iamr_amd/csrc/k_profile.hip) through the C-ABI against the numpy restatement of tests/profile_numpy.py on the same data.

The reference is math.fsum per bin (exact up to two roundings).  Tolerance, derived: a mean of N terms summed in any order is within
N 2^-52 mean |q| of the exact mean (profile_numpy's docstring), per bin with N the counted cells of that bin.  The shapes are the smallest
at which each path of the kernels can go wrong: unequal extents, rows that are no multiple of a wavefront and rows shorter than one,
several unequal boxes, three levels with folding and spreading."""
import os
import numpy as np
import pytest
import profile_numpy as PN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
REGRID16 = os.path.join(GOLD, "inputs.3d.tracer_regrid16")
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]


def random_state(n, seed):
    """u v w rho c of order one, every component with a mean of its own"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=tuple(n) + (5,)) + np.array([0.3, -0.2, 0.1, 1.5, 0.5])


def put_state(level, lay, S):
    """the new-time state of a level := S on the valid cells of every box, NaN in ALL ghost cells (also those between boxes)"""
    from iamr_amd import lib as L
    mf = L.MultiFab(lay, L.CELL, 5, 1)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (5,), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = S[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    level.set_data(level.S_NEW, mf)


def one_level(n, S, max_grid_size=None):
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    g = L.Geom.make(list(n), periodic=(1, 1, 1))
    lay = L.Layout.single(n) if max_grid_size is None else L.Layout.decompose(tuple(n), max_grid_size)
    ns = N.NavierStokes(g, lay, N.ns_params())
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    return ns, lay


def as_array(p):
    return np.stack([p[k] for k in PN.NAMES])


def check(got, ref, tag):
    """got (14, nbins) against profile_reference's (mean, N, meanabs); prints the largest error in units of the bound"""
    mean, N, meanabs = ref
    bd = PN.bound(N, meanabs)
    assert got.shape == mean.shape, (tag, got.shape, mean.shape)
    err = np.abs(got - mean)
    worst = float(np.max(err / bd))
    print(f"{tag}: max |got - fsum| = {float(err.max()):.3e}, worst error / bound = {worst:.3f} (N per bin {int(N.min())} .. {int(N.max())})")
    assert np.all(err <= bd), (tag, worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------ 1. one box
@pytest.mark.parametrize("n,dirs", [((20, 12, 6), (0, 1, 2)), ((4, 8, 8), (0,))])
def test_one_box(gpu, n, dirs):
    """unequal extents (an axis mix-up shows), nx neither a multiple nor a divisor of 64; then a row shorter than a wavefront"""
    S = random_state(n, 5)
    ns, lay = one_level(n, S)
    for d in dirs:
        p = ns.plane_profile(d)
        assert p["names"] == PN.NAMES and p["one"].shape == (n[d],)
        assert np.array_equal(p["coord"], (np.arange(n[d]) + 0.5) * (1.0 / n[d]))
        check(as_array(p), PN.profile_reference([S], [lay.boxes], list(n), d, 0), f"{n} dir {d}")
        assert np.all(np.abs(p["one"] - 1.0) <= 4 * 2.0 ** -52)


def test_errors(gpu):
    from iamr_amd.lib import IamrxError, lib
    import ctypes as C
    n = (4, 8, 8)
    ns, lay = one_level(n, random_state(n, 1))
    out, nb = np.zeros(14 * 8), C.c_int()
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    for d in (-1, 3):
        with pytest.raises(IamrxError, match="dir"):
            ns.plane_profile(d)
    assert lib().iamrx_ns_plane_profile(ns.h, 1, 7, ptr, C.byref(nb)) != 0            # capacity too small
    assert lib().iamrx_ns_plane_profile(ns.h, 1, 8, ptr, C.byref(nb)) == 0 and nb.value == 8


# ------------------------------------------------------------------------------------------------------------------ 2. unequal boxes
N2 = (24, 16, 20)


def test_several_unequal_boxes(gpu):
    """max_grid_size 16: boxes of 16 and 8 cells along x and of 16 and 4 along z; the same data in one box give the same profile"""
    S = random_state(N2, 9)
    many, lay = one_level(N2, S, 16)
    assert sorted({hi[0] - lo[0] + 1 for lo, hi in lay.boxes}) == [8, 16] and sorted({hi[2] - lo[2] + 1 for lo, hi in lay.boxes}) == [4, 16]
    one, lay1 = one_level(N2, S)
    for d in range(3):
        ref = PN.profile_reference([S], [lay.boxes], list(N2), d, 0)
        a, b = as_array(many.plane_profile(d)), as_array(one.plane_profile(d))
        check(a, ref, f"4 boxes dir {d}")
        check(b, ref, f"1 box   dir {d}")
        assert np.all(np.abs(a - b) <= PN.bound(ref[1], ref[2]))


# ------------------------------------------------------------------------------------------------------------------ 3 - 5. hierarchy
def hierarchy():
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    pr = Inputs([AMR16]).problem()
    amr, lays, g0 = R.build_amr(pr, L, N)
    assert amr.nlev == 3 and list(amr.geom0.n) == [16, 16, 16]
    return amr


def hierarchy_states(amr, seed, nan_covered):
    n0 = [16, 16, 16]
    boxes = [amr.layouts[l].boxes for l in range(amr.nlev)]
    counted = PN.counted_masks(boxes, n0)
    states = []
    for l in range(amr.nlev):
        S = random_state([v << l for v in n0], seed + l)
        if nan_covered:
            S[PN.box_mask(boxes[l], S.shape[:3]) & ~counted[l]] = np.nan       # what a finer level covers must not reach a bin
        states.append(S)
    return states, boxes, n0


def put_hierarchy(amr, states):
    for l in range(amr.nlev):
        put_state(amr.levels[l], amr.layouts[l], states[l])


def test_hierarchy(gpu):
    """three levels, random data, NaN under the finer levels: every axis and every bin level against the restatement; the uncovered
    volume fraction is 1; the same call three times gives the same bits; sum of <rho> * slab volume = the composite integral"""
    amr = hierarchy()
    states, boxes, n0 = hierarchy_states(amr, 20, True)
    put_hierarchy(amr, states)
    for d in range(3):
        for B in range(3):
            p = amr.plane_profile(d, B)
            assert p["one"].shape == (16 << B,) and p["bin_level"] == B
            got = as_array(p)
            check(got, PN.profile_reference(states, boxes, n0, d, B), f"hierarchy dir {d} B {B}")
            assert np.all(np.abs(got[0] - 1.0) <= 4 * 2.0 ** -52), (d, B, float(np.abs(got[0] - 1.0).max()))
            for _ in range(2):                                                      # the same bits on every call
                assert as_array(amr.plane_profile(d, B)).tobytes() == got.tobytes(), (d, B)
    # finite data under the finer levels for the integrals: sum_integrated skips them too, and must agree
    states, boxes, n0 = hierarchy_states(amr, 40, False)
    put_hierarchy(amr, states)
    mass, trac, _ = amr.sum_integrated()
    ncount = int(sum(m.sum() for m in PN.counted_masks(boxes, n0)))
    for d in range(3):
        for B in range(3):
            p = amr.plane_profile(d, B)
            mean, N, meanabs = PN.profile_reference(states, boxes, n0, d, B)
            slab = 1.0 / len(p["rho"])
            for name, want in (("rho", mass), ("c", trac)):
                q = PN.NAMES.index(name)
                tol = ncount * 2.0 ** -52 * float(np.sum(meanabs[q]) * slab)
                diff = abs(float(np.sum(p[name])) * slab - want)
                print(f"dir {d} B {B}: |sum <{name}> slab - integral| = {diff:.3e} (bound {tol:.3e})")
                assert diff <= tol, (d, B, name, diff, tol)
    from iamr_amd.lib import IamrxError
    for d, B in ((0, 3), (0, -1), (3, 0)):
        with pytest.raises(IamrxError):
            amr.plane_profile(d, B)


def test_nan_rule(gpu):
    """one NaN in u of one uncovered cell: u, uu, uv, uw are NaN in that cell's bin(s) only, every other entry keeps its bits.  A level-0
    cell under bin level 1 spans two bins (spread); a level-2 cell lies in one (fold)."""
    amr = hierarchy()
    states, boxes, n0 = hierarchy_states(amr, 60, True)
    counted = PN.counted_masks(boxes, n0)
    put_hierarchy(amr, states)
    d, B = 2, 1
    clean = as_array(amr.plane_profile(d, B))
    assert np.isfinite(clean).all()
    hit = {n: PN.NAMES.index(n) for n in ("u", "uu", "uv", "uw")}
    for l, cell, bins in ((0, (0, 0, 0), [0, 1]), (2, (24, 22, 26), [13])):
        assert counted[l][cell]
        keep = states[l][cell + (0,)]
        states[l][cell + (0,)] = np.nan
        put_state(amr.levels[l], amr.layouts[l], states[l])
        got = as_array(amr.plane_profile(d, B))
        states[l][cell + (0,)] = keep
        put_state(amr.levels[l], amr.layouts[l], states[l])
        bad = np.zeros(got.shape, dtype=bool)
        for q in hit.values():
            bad[q, bins] = True
        assert np.array_equal(np.isnan(got), bad), (l, np.argwhere(np.isnan(got) != bad))
        assert got[~bad].tobytes() == clean[~bad].tobytes(), l
    assert as_array(amr.plane_profile(d, B)).tobytes() == clean.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 6. known answer
def test_known_answer(gpu):
    """rho(z) = 1 + tanh((z - 1/2) / 0.1), fluid at rest, 16^3: along z the profile is rho at the bin centres and has no variance inside a
    bin; along x every bin holds the same constant, the mean of rho over z"""
    n = (16, 16, 16)
    z = (np.arange(16) + 0.5) / 16
    rho = 1.0 + np.tanh((z - 0.5) / 0.1)
    S = np.zeros(n + (5,))
    S[..., 3] = rho[None, None, :]
    ns, lay = one_level(n, S)
    p = ns.plane_profile(2)
    b1 = 256 * 2.0 ** -52 * np.abs(rho)                     # the bound for <rho>: 256 cells per bin
    b2 = 256 * 2.0 ** -52 * rho * rho                       # ... and for <rho rho>
    assert np.array_equal(p["coord"], z)
    e1 = np.abs(p["rho"] - rho)
    var = p["rhorho"] - p["rho"] * p["rho"]
    # <rho rho> - <rho>^2 with both means off by their bounds, plus the rounding of the product and of the difference
    bv = b2 + 2.0 * np.abs(rho) * b1 + 2.0 ** -52 * rho * rho
    print(f"z profile: max |<rho> - rho(z)| = {float(e1.max()):.3e} (bound {float(b1.max()):.3e}); max |variance| = {float(np.abs(var).max()):.3e} (bound {float(bv.max()):.3e})")
    assert np.all(e1 <= b1) and np.all(np.abs(var) <= bv)
    for k in ("u", "v", "w", "c", "uu", "vw", "cc"):
        assert not p[k].any(), k
    px = ns.plane_profile(0)
    import math
    mean = math.fsum(rho) / 16
    ex = np.abs(px["rho"] - mean)
    print(f"x profile: max |<rho> - mean| = {float(ex.max()):.3e} (bound {256 * 2.0 ** -52 * mean:.3e})")
    assert np.all(ex <= 256 * 2.0 ** -52 * mean)


# ------------------------------------------------------------------------------------------------------------------ 8. driver
def test_driver_writes_the_files(gpu, tmp_path, monkeypatch):
    """inputs.3d.tracer_regrid16, two steps with ns.profile_interval = 1 and a bin level the hierarchy may not have: prof00000 .. prof00002
    appear in the working directory, the last equals Amr.plane_profile after the step bit for bit, the bin level in every header is the
    requested one clamped to the finest level of that moment; without the keys no file appears"""
    from iamr_amd import run as R
    from iamr_amd.profile import read_profile, NAMES
    seen = {}

    def observe(amr, step, dt):
        B = min(2, amr.nlev - 1)
        seen[step] = (amr.nlev, amr.time, amr.plane_profile(2, B))

    d1 = tmp_path / "on"; d1.mkdir()
    monkeypatch.chdir(d1)
    assert R.main([REGRID16, "max_step=2", "ns.profile_interval=1", "ns.profile_level=2"] + QUIET, observe) == 0
    assert sorted(os.listdir(d1)) == ["prof00000", "prof00001", "prof00002"]
    for step in range(3):
        nlev, time, p = seen[step]
        r = read_profile(str(d1 / f"prof{step:05d}"))
        assert (r["step"], r["time"], r["dir"], r["names"]) == (step, time, 2, NAMES)
        assert r["bin_level"] == min(2, nlev - 1) <= nlev - 1
        assert len(r["coord"]) == 16 << r["bin_level"]
        for k in NAMES + ("coord",):
            assert r[k].tobytes() == p[k].tobytes(), (step, k)
        assert np.all(np.abs(r["one"] - 1.0) <= 4 * 2.0 ** -52)
    assert max(v[0] for v in seen.values()) > 1                                   # a hierarchy, not one level
    d2 = tmp_path / "off"; d2.mkdir()
    monkeypatch.chdir(d2)
    assert R.main([REGRID16, "max_step=2"] + QUIET) == 0
    assert os.listdir(d2) == []


def test_driver_single_level(gpu, tmp_path):
    """the one-level loop of the driver (inputs.3d.lid_driven_cavity16, one step, profiles across the cavity into a named file): the
    files hold Navierstokes.plane_profile of that moment bit for bit; a requested bin level above the only level is clamped to 0"""
    from iamr_amd import run as R
    from iamr_amd.profile import read_profile, NAMES
    seen = {}

    def observe(ns, step, dt):
        seen[step] = (ns.time, ns.plane_profile(1))

    root = str(tmp_path / "cavity_y")
    LDC16 = os.path.join(GOLD, "inputs.3d.lid_driven_cavity16")
    assert R.main([LDC16, "max_step=1", "ns.profile_interval=1", "ns.profile_dir=1", "ns.profile_level=1", f"ns.profile_file={root}"] + QUIET, observe) == 0
    assert sorted(os.listdir(tmp_path)) == ["cavity_y00000", "cavity_y00001"]
    for step in (0, 1):
        r = read_profile(f"{root}{step:05d}")
        assert (r["step"], r["time"], r["dir"], r["bin_level"]) == (step, seen[step][0], 1, 0)
        for k in NAMES + ("coord",):
            assert r[k].tobytes() == seen[step][1][k].tobytes(), (step, k)
    assert float(np.abs(read_profile(f"{root}00001")["u"]).max()) > 0.0               # the lid has set the fluid in motion
