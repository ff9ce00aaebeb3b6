"""GPU: structure functions and two-point correlations along the axes (include/iamrx.h: iamrx_mf_strfn / iamrx_ns_strfn /
iamrx_amr_strfn; kernels in iamr_amd/csrc/k_strfn.hip) through the C-ABI against the numpy yardstick of tests/strfn_numpy.py on the
same data.

The yardstick forms the pairs with np.roll (periodic) or slices (walls) and sums with math.fsum; the tolerance is its derived bound
|got - ref| <= gamma_{K + 2 p + 2} mean|t_k| (strfn_numpy's docstring; K the pair count).  The data are white noise of order one with a
non-zero mean, every ghost cell holds NaN, pmax = 4 and rmax = -1 unless stated.  The shapes are the smallest at which each path can
go wrong: unequal extents, extents that are no powers of two, walls on some or all axes, the longest pencil on each axis, a pencil of
exactly one wavefront and one more, the smallest level.

Largest error / bound seen on an MI355X: see DESIGN.md section 4, "Structure functions"."""
import ctypes as C
import functools
import os
import numpy as np
import pytest
import strfn_numpy as SF
from test_gpu_spectrum import make_mf, geom_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
FORCED = os.path.join(GOLD, "inputs.3d.forced")
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]
UNIT = (1.0, 1.0, 1.0)
PER = (1, 1, 1)
LONG = (1024, 4, 4)


@functools.lru_cache(maxsize=None)
def reference(n, periodic=PER, pmax=4, rmax=(-1, -1, -1), seed=3, ncomp=1):
    """(f (n, ncomp), [SF.reference per component]): computed once per case and shared, never written to"""
    f = SF.noise(n, seed, ncomp)
    f.setflags(write=False)
    return f, [SF.reference(f[..., q], periodic, pmax, rmax) for q in range(ncomp)]


@functools.lru_cache(maxsize=None)
def long_reference(axis):
    """the longest pencil on `axis`: the (1024, 4, 4) noise with its axes swapped, so that the one yardstick run serves all three"""
    f, refs = reference(LONG)
    if axis == 0:
        return f, refs
    avg, count, meanabs, mean = refs[0]
    perm = [0, 1, 2]
    perm[0], perm[axis] = axis, 0
    g = np.ascontiguousarray(np.swapaxes(f, 0, axis))
    g.setflags(write=False)
    return g, [(avg[perm], count[perm], meanabs[perm], mean)]


def check(s, ref, q, tag, f=None):
    """component q of the raw dict s against the yardstick's (avg, count, meanabs, mean): every column inside the bound, the counts and
    the zeros beyond rmax exact, the mean inside its bound if the field f is given; prints the largest error in units of the bound"""
    avg, count, meanabs, mean = ref
    pmax = s["pmax"]
    bd = SF.bound(count, meanabs, pmax)
    got = s["avg"][:, q]
    assert got.shape == avg.shape, (tag, got.shape, avg.shape)
    assert s["count"].dtype == np.int64 and np.array_equal(s["count"], count), tag
    err = np.abs(got - avg)
    live = bd > 0.0
    assert not got[(count == 0)[:, None, :].repeat(got.shape[1], axis=1)].any(), tag          # nothing beyond rmax or on a skipped axis
    worst = float(np.max(err[live] / bd[live])) if live.any() else 0.0
    print(f"{tag}: max |got - yardstick| = {float(err.max()):.3e}, worst error / bound = {worst:.4f}")
    assert np.all(err <= bd), (tag, worst)
    if f is not None:
        assert abs(s["mean"][q] - mean) <= SF.mean_bound(f), (tag, s["mean"][q], mean)
    return worst


# ------------------------------------------------------------------------------------------------------------------ 1. one array
@pytest.mark.parametrize("n,periodic", [((8, 16, 32), PER), ((12, 6, 10), PER), ((8, 16, 32), (1, 0, 1)), ((8, 16, 32), (0, 0, 0)),
                                        ((64, 4, 4), (0, 1, 1)), ((65, 4, 4), (0, 1, 1)), ((2, 2, 2), PER)])
def test_one_box(gpu, n, periodic):
    """unequal extents (an axis mix-up shows); extents that are no powers of two (the wrap); walls on one axis and on all (no wrap, the
    pair counts, r = n - 1); a pencil of one wavefront and of one more; the smallest level.  A second call gives the same bits."""
    f, refs = reference(n, periodic)
    mf, _ = make_mf(n, f)
    g = geom_of(n, UNIT, periodic)
    s = gpu.mf_structure(g, mf, 0, 1)
    rm = SF.resolve(n, periodic, (-1, -1, -1))
    assert s["rmax"] == rm and s["avg"].shape == (3, 1, 7, 1 + max(rm)) and s["periodic"] == periodic and s["n"] == n
    check(s, refs[0], 0, f"{n} periodic {periodic}", f[..., 0])
    s2 = gpu.mf_structure(g, mf, 0, 1)
    assert s2["avg"].tobytes() == s["avg"].tobytes() and s2["mean"].tobytes() == s["mean"].tobytes()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_longest_pencil(gpu, axis):
    """1024 cells along one axis, 4 along the others: r up to 512"""
    f, refs = long_reference(axis)
    n = f.shape[:3]
    assert n[axis] == 1024 and sorted(n) == [4, 4, 1024]
    mf, _ = make_mf(n, f)
    s = gpu.mf_structure(geom_of(n), mf, 0, 1)
    assert s["avg"].shape == (3, 1, 7, 513)
    check(s, refs[0], 0, f"{n}", f[..., 0])


@pytest.mark.parametrize("pmax", [1, 8])
def test_lowest_and_highest_order(gpu, pmax):
    n = (8, 16, 32)
    f, refs = reference(n, PER, pmax)
    mf, _ = make_mf(n, f)
    s = gpu.mf_structure(geom_of(n), mf, 0, 1, pmax=pmax)
    assert s["avg"].shape == (3, 1, SF.ncol_of(pmax), 17)
    check(s, refs[0], 0, f"{n} pmax {pmax}")


def test_some_separations_and_a_skipped_axis(gpu):
    """rmax = (3, 0, -1): x up to 3, y skipped -- all of it zero, the counts too -- z up to 16"""
    n, rmax = (8, 16, 32), (3, 0, -1)
    f, refs = reference(n, PER, 4, rmax)
    mf, _ = make_mf(n, f)
    s = gpu.mf_structure(geom_of(n), mf, 0, 1, rmax=rmax)
    assert s["rmax"] == (3, 0, 16) and s["avg"].shape == (3, 1, 7, 17)
    check(s, refs[0], 0, f"{n} rmax {rmax}")
    assert not s["avg"][1].any() and not s["count"][1].any() and not s["avg"][0, :, :, 4:].any() and not s["count"][0, 4:].any()
    assert s["avg"][0, 0, 0, :4].all() and s["avg"][2, 0, 0].all()


@pytest.mark.parametrize("periodic", [PER, (1, 0, 1)])
def test_identities_on_the_device_result(gpu, periodic):
    """within twice the bound: <delta^2> = 2 (R(0) - R(r)) on periodic axes; <|delta|> >= |<delta>|; <delta> = 0 on periodic axes,
    against the bound of its own mean|t|"""
    n = (8, 16, 32)
    f, refs = reference(n, periodic)
    avg_ref, count, meanabs, _ = refs[0]
    bd = SF.bound(count, meanabs, 4)
    mf, _ = make_mf(n, f)
    a = gpu.mf_structure(geom_of(n, UNIT, periodic), mf, 0, 1)["avg"][:, 0]
    for d in range(3):
        rm = SF.limit_of(n[d], periodic[d])
        r = slice(0, rm + 1)
        assert np.all(a[d, 5, r] >= np.abs(a[d, 1, r]) - 2.0 * (bd[d, 5, r] + bd[d, 1, r]))
        if periodic[d]:
            lhs, rhs = a[d, 2, r], 2.0 * (a[d, 0, 0] - a[d, 0, r])
            tol = 2.0 * (bd[d, 2, r] + 2.0 * (bd[d, 0, 0] + bd[d, 0, r]))
            print(f"axis {d}: max |S2 - 2 (R(0) - R(r))| / tolerance = {float(np.max(np.abs(lhs - rhs) / tol)):.4f}, "
                  f"max |S1| / bound = {float(np.max(np.abs(a[d, 1, 1:rm + 1]) / bd[d, 1, 1:rm + 1])):.4f}")
            assert np.all(np.abs(lhs - rhs) <= tol)
            assert np.all(np.abs(a[d, 1, r]) <= 2.0 * bd[d, 1, r])


def test_cosine_and_linear_fields(gpu):
    """cos(2 pi 2 i / 12) along periodic y against the closed forms R = cos(t r) / 2, <delta^2> = 1 - cos(t r), <delta^3> = 0 (within the
    bound and the closed form's own evaluation, 64 u); 4 i along a wall axis: <delta^p> = (4 r)^p, the count and R exact"""
    n = (6, 12, 10)
    f = SF.cosine(n, 1, 2)[..., None]
    ref = SF.reference(f[..., 0], PER, 4)
    mf, _ = make_mf(n, f)
    s = gpu.mf_structure(geom_of(n), mf, 0, 1)
    check(s, ref, 0, "cosine")
    bd = SF.bound(ref[1], ref[2], 4)
    r = np.arange(7)
    c = np.cos(2.0 * np.pi * 2 * r / 12)
    closed = 64.0 * SF.U
    assert np.all(np.abs(s["avg"][1, 0, 0, :7] - 0.5 * c) <= bd[1, 0, :7] + closed)
    assert np.all(np.abs(s["avg"][1, 0, 2, :7] - (1.0 - c)) <= bd[1, 2, :7] + closed)
    assert np.all(np.abs(s["avg"][1, 0, 3, :7]) <= bd[1, 3, :7] + closed)
    for n, d in (((10, 4, 3), 0), ((3, 9, 4), 1), ((4, 3, 16), 2)):
        per = tuple(0 if q == d else 1 for q in range(3))
        f = SF.linear(n, d)[..., None]
        avg, count, _, mean = SF.reference(f[..., 0], per, 4)
        mf, _ = make_mf(n, f)
        s = gpu.mf_structure(geom_of(n, UNIT, per), mf, 0, 1)
        assert s["avg"][:, 0].tobytes() == avg.tobytes() and np.array_equal(s["count"], count) and s["mean"][0] == mean, (n, d)
        for rr in range(n[d]):
            assert [s["avg"][d, 0, p, rr] for p in range(1, 5)] == [(4.0 * rr) ** p for p in range(1, 5)]


def test_one_box_against_eight(gpu):
    """32^3 as one box and as eight 16^3 boxes, two components: both inside the bound and equal to the byte (only the pack differs); a
    second call gives the same bytes; count and mean may be NULL; a component taken alone gives its bytes"""
    n = (32, 32, 32)
    f, refs = reference(n, PER, 4, (-1, -1, -1), 7, 2)
    g = geom_of(n)
    one, _ = make_mf(n, f)
    eight, lay8 = make_mf(n, f, 16)
    assert len(lay8.boxes) == 8
    a, b = gpu.mf_structure(g, one, 0, 2), gpu.mf_structure(g, eight, 0, 2)
    for q in range(2):
        check(a, refs[q], q, f"32^3 one box, component {q}", f[..., q])
        check(b, refs[q], q, f"32^3 eight boxes, component {q}", f[..., q])
    assert a["avg"].tobytes() == b["avg"].tobytes() and a["mean"].tobytes() == b["mean"].tobytes() and np.array_equal(a["count"], b["count"])
    assert gpu.mf_structure(g, eight, 0, 2)["avg"].tobytes() == b["avg"].tobytes()
    out = np.zeros(3 * 7 * 17)
    rmax = (C.c_int * 3)(-1, -1, -1)
    assert gpu.lib().iamrx_mf_strfn(C.byref(g), eight.h, 1, 1, 4, rmax, 17, out.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0
    assert out.reshape(3, 7, 17).tobytes() == np.ascontiguousarray(a["avg"][:, 1]).tobytes()


# ------------------------------------------------------------------------------------------------------------------ 2. level, hierarchy
def state_check(s, S, periodic, tag):
    """the dict of NavierStokes.structure_functions / Amr.structure_functions against the yardstick on the state S (n, >= 5): u v w . c"""
    from iamr_amd import strfn as P
    for q, comp in enumerate((0, 1, 2, 4)):
        check(s, SF.reference(np.ascontiguousarray(S[..., comp]), periodic, s["pmax"]), q, f"{tag} {P.COMPONENTS[q]}", S[..., comp])
    again = P.derive(P.raw_dict(s["avg"], s["count"], s["mean"], s["n"], s["L"], s["periodic"], s["pmax"], s["rmax"]))
    for k in ("SL", "ST", "Sc", "SLabs", "RL", "RT", "f", "g", "integral_scale", "taylor_scale"):
        assert np.array_equal(s[k], again[k], equal_nan=True), k
    for d in range(3):
        assert np.array_equal(s["SL"][d, 2], s["avg"][d, d, 2]) and s["f"][d, 0] == 1.0
        assert s["integral_scale"][d] > 0.0 and s["taylor_scale"][d] > 0.0


def test_level(gpu):
    """iamrx_ns_strfn on a 16^3 periodic level in eight boxes whose new-time state was set from outside: u, v, w, c"""
    from test_gpu_profile import random_state, one_level
    n = (16, 16, 16)
    S = random_state(n, 12)
    ns, lay = one_level(n, S, 8)
    s = ns.structure_functions()
    assert s["avg"].shape == (3, 4, 7, 9) and s["rmax"] == (8, 8, 8)
    state_check(s, S, PER, "level 16^3")
    assert ns.structure_functions()["avg"].tobytes() == s["avg"].tobytes()
    s2 = ns.structure_functions(pmax=2, rmax=(4, 0, 2))
    assert s2["avg"].shape == (3, 4, 4, 5) and s2["rmax"] == (4, 0, 2) and not s2["avg"][1].any() and not s2["avg"][2, :, :, 3:].any()
    assert np.isnan(s2["integral_scale"][1]) and s2["integral_scale"][0] > 0.0


def test_hierarchy(gpu):
    """iamrx_amr_strfn on inputs.3d.taylorgreen_amr16 after one coarse step: the mf entry on level 0's state, to the byte, and the
    yardstick on that state read back"""
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
    s = amr.structure_functions()
    lev0 = amr.levels[0]
    state = lev0.data(lev0.S_NEW)
    direct = gpu.mf_structure(amr.geom0, state, 0, 3)
    assert np.ascontiguousarray(s["avg"][:, :3]).tobytes() == direct["avg"].tobytes() and s["mean"][:3].tobytes() == direct["mean"].tobytes()
    tracer = gpu.mf_structure(amr.geom0, state, 4, 1)
    assert np.ascontiguousarray(s["avg"][:, 3:]).tobytes() == tracer["avg"].tobytes() and np.array_equal(s["count"], direct["count"])
    S = state.gather_valid(n)
    for q, comp in enumerate((0, 1, 2, 4)):
        check(s, SF.reference(np.ascontiguousarray(S[..., comp]), PER, 4), q, f"hierarchy level 0, component {q}", S[..., comp])


# ------------------------------------------------------------------------------------------------------------------ 3. driver
def test_driver_writes_the_files(gpu, tmp_path, monkeypatch):
    """inputs.3d.forced at 16^3, four steps with ns.strfn_interval = 2: sf00000, sf00002 and sf00004 appear in the working directory and
    hold NavierStokes.structure_functions of that moment bit for bit"""
    from iamr_amd import run as R
    from iamr_amd.strfn import read_strfn
    over = ["amr.n_cell=16 16 16", "max_step=4", "amr.derive_plot_vars=NONE"] + QUIET
    seen = {}

    def observe(ns, step, dt):
        if step % 2 == 0:
            seen[step] = (ns.time, ns.structure_functions())

    monkeypatch.chdir(tmp_path)
    assert R.main([FORCED, "ns.strfn_interval=2"] + over, observe) == 0
    assert sorted(os.listdir(tmp_path)) == ["sf00000", "sf00002", "sf00004"]
    for step in (0, 2, 4):
        time, s = seen[step]
        r = read_strfn(str(tmp_path / f"sf{step:05d}"))
        assert (r["step"], r["time"], r["n"], r["pmax"], r["rmax"]) == (step, time, (16, 16, 16), 4, (8, 8, 8))
        assert sorted(r) == sorted(list(s) + ["step", "time"])
        for k, v in s.items():
            if isinstance(v, np.ndarray):
                assert r[k].tobytes() == v.tobytes(), (step, k)
            else:
                assert r[k] == v, (step, k)
    assert seen[4][1]["avg"].tobytes() != seen[0][1]["avg"].tobytes()


# ------------------------------------------------------------------------------------------------------------------ 4. errors
def test_errors(gpu):
    from iamr_amd.lib import IamrxError
    n = (8, 16, 32)
    f, _ = reference(n)
    mf, _ = make_mf(n, f)
    with pytest.raises(IamrxError, match="cover"):                                  # the array's one box is half of this domain
        gpu.mf_structure(geom_of((8, 16, 64)), mf, 0, 1)
    with pytest.raises(IamrxError, match="component"):
        gpu.mf_structure(geom_of(n), mf, 1, 1)
    with pytest.raises(IamrxError, match="not cell-centred"):
        gpu.mf_structure(geom_of(n), gpu.MultiFab(gpu.Layout.single(n), gpu.NODE, 1, 0), 0, 1)
    with pytest.raises(IamrxError, match=r"rmax_y = 9"):                            # periodic: n / 2 = 8
        gpu.mf_structure(geom_of(n), mf, 0, 1, rmax=(4, 9, 16))
    with pytest.raises(IamrxError, match=r"rmax_x = 8"):                            # walls: n - 1 = 7
        gpu.mf_structure(geom_of(n, UNIT, (0, 1, 1)), mf, 0, 1, rmax=(8, 8, 16))
    big = (2048, 2, 2)
    fb = SF.noise(big, 1)
    mfb, _ = make_mf(big, fb)
    with pytest.raises(IamrxError, match=r"n_x = 2048"):
        gpu.mf_structure(geom_of(big), mfb, 0, 1)
    assert gpu.mf_structure(geom_of(big), mfb, 0, 1, rmax=(0, -1, -1))["rmax"] == (0, 1, 1)        # ... unless the axis is skipped
    g = geom_of(n)
    out = np.zeros(3 * 7 * 17)
    ptr, rmax = out.ctypes.data_as(C.POINTER(C.c_double)), (C.c_int * 3)(-1, -1, -1)
    assert gpu.lib().iamrx_mf_strfn(C.byref(g), mf.h, 0, 1, 4, rmax, 16, ptr, None, None) != 0          # rcap too small
    assert b"rcap" in gpu.lib().iamrx_last_error() and not out.any()
    assert gpu.lib().iamrx_mf_strfn(C.byref(g), mf.h, 0, 1, 9, rmax, 17, ptr, None, None) != 0          # pmax out of range
    assert b"pmax" in gpu.lib().iamrx_last_error() and not out.any()
    assert gpu.lib().iamrx_mf_strfn(C.byref(g), mf.h, 0, 1, 4, rmax, 17, ptr, None, None) == 0 and out.any()
