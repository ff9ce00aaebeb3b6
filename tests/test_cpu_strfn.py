"""CPU suite: structure functions and two-point correlations along the axes (iamr_amd/strfn.py, the ns.strfn_* keys of
iamr_amd/inputs.py, the entries of include/iamrx.h) -- everything about them that needs no device.  The numpy yardstick the GPU tests
compare with (tests/strfn_numpy.py) is itself checked here against fields whose answer is written out."""
import math
import os
import re
import numpy as np
import pytest
import strfn_numpy as SF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TG16 = os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
FORCED = os.path.join(HERE, "golden", "inputs.3d.forced")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")
# a closed form evaluated in double: every term is a product or a difference of two cosines, each within an ulp or two of the true value,
# and the yardstick's sum is exact: 64 u covers it with room (the values are of order one)
CLOSED = 64.0 * SF.U


# ------------------------------------------------------------------------------------------------------------------ 1. the yardstick
@pytest.mark.parametrize("n,d,m", [((16, 4, 4), 0, 1), ((4, 12, 6), 1, 2), ((4, 6, 20), 2, 3)])
def test_yardstick_on_a_cosine(n, d, m):
    """f = cos(2 pi m i / n) along a periodic axis: R(r) = cos(2 pi m r / n) / 2, <delta^2> = 1 - cos(2 pi m r / n), <delta^3> = 0,
    <delta> = 0, count = N; the other two axes see a constant: R = <f^2> = 1/2 and every delta zero"""
    f = SF.cosine(n, d, m)
    avg, count, meanabs, mean = SF.reference(f, (1, 1, 1), 4)
    N = f.size
    r = np.arange(n[d] // 2 + 1)
    c = np.cos(2.0 * np.pi * m * r / n[d])
    assert np.all(count[d, :len(r)] == N) and abs(mean) <= CLOSED
    assert np.max(np.abs(avg[d, 0, :len(r)] - 0.5 * c)) <= CLOSED
    assert np.max(np.abs(avg[d, 2, :len(r)] - (1.0 - c))) <= CLOSED
    assert np.max(np.abs(avg[d, 1, :len(r)])) <= CLOSED and np.max(np.abs(avg[d, 3, :len(r)])) <= CLOSED
    for o in range(3):
        if o != d:
            ro = n[o] // 2 + 1
            assert np.max(np.abs(avg[o, 0, :ro] - 0.5)) <= CLOSED and not avg[o, 1:, :].any()


@pytest.mark.parametrize("n,d", [((10, 4, 3), 0), ((3, 9, 4), 1), ((4, 3, 16), 2)])
def test_yardstick_on_a_linear_field_with_walls(n, d):
    """f = 4 i along a wall axis: <delta^p> = (4 r)^p exactly, <|delta|^p> the same, count = (n - r) N / n, r up to n - 1"""
    f = SF.linear(n, d)
    per = tuple(0 if q == d else 1 for q in range(3))
    avg, count, meanabs, mean = SF.reference(f, per, 4)
    N = f.size
    assert avg.shape == (3, 7, max(n[d], max(n) // 2 + 1))
    for r in range(n[d]):
        assert count[d, r] == (n[d] - r) * N // n[d]
        for p in range(1, 5):
            assert avg[d, p, r] == (4.0 * r) ** p
        assert avg[d, 5, r] == 4.0 * r and avg[d, 6, r] == (4.0 * r) ** 3
        i = np.arange(n[d] - r)
        assert avg[d, 0, r] == math.fsum((16.0 * i * (i + r)).tolist()) / (n[d] - r)
    assert mean == 2.0 * (n[d] - 1)


def test_yardstick_columns_and_bound():
    assert [SF.ncol_of(p) for p in (1, 2, 4, 8)] == [3, 4, 7, 13]
    assert [SF.col_power(4, c) for c in range(7)] == [1, 1, 2, 3, 4, 1, 3]
    assert [SF.col_power(8, c) for c in range(9, 13)] == [1, 3, 5, 7] and SF.col_power(1, 2) == 1
    cnt = np.array([[4096, 2048, 0]] * 3)
    bd = SF.bound(cnt, np.ones((3, 7, 3)), 4)
    assert bd[0, 4, 0] == SF.gamma(4096 + 8 + 2) and bd[1, 0, 1] == SF.gamma(2048 + 2 + 2) and 4.5e-13 < bd[0, 4, 0] < 4.6e-13


# ------------------------------------------------------------------------------------------------------------------ 2. header, library
def test_header_declares_and_library_exports_the_entries():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    tail = (r"int\s+pmax,\s*const\s+int\s+rmax\s*\[\s*3\s*\],\s*int\s+rcap,\s*double\s*\*\s*out,\s*long\s+long\s*\*\s*count,"
            r"\s*double\s*\*\s*mean")
    L = lib.lib()
    for name, args in (("iamrx_strfn_ncol", r"int\s+pmax"), ("iamrx_strfn_nq", r"void"),
                       ("iamrx_mf_strfn", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+ncomp,\s*" + tail),
                       ("iamrx_ns_strfn", r"iamrx_ns\s+ns,\s*" + tail),
                       ("iamrx_amr_strfn", r"iamrx_amr\s+a,\s*" + tail),
                       ("iamrx_strfn_bench", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+pmax,\s*const\s+int\s+rmax\s*\[\s*3\s*\],"
                                             r"\s*int\s+reps,\s*float\s*\*\s*ms")):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", txt), name
        assert hasattr(L, name), name
    assert L.iamrx_strfn_nq() == 4
    assert [L.iamrx_strfn_ncol(p) for p in (2, 4, 8)] == [4, 7, 13] and L.iamrx_strfn_ncol(1) == 3
    assert L.iamrx_strfn_ncol(0) < 0 and L.iamrx_strfn_ncol(9) < 0
    from iamr_amd.ns import ns_params, NavierStokes
    from iamr_amd.amr import Amr
    from iamr_amd import strfn as S
    assert not [f for f, _ in type(ns_params())._fields_ if "strfn" in f or "structure" in f]
    assert callable(NavierStokes.structure_functions) and callable(Amr.structure_functions) and callable(lib.mf_structure)
    assert [S.ncol_of(p) for p in (1, 2, 4, 8)] == [SF.ncol_of(p) for p in (1, 2, 4, 8)]
    assert [S.abs_col(4, 1), S.abs_col(4, 3), S.abs_col(8, 7)] == [5, 6, 12]


# ------------------------------------------------------------------------------------------------------------------ 3. inputs
def test_strfn_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([TG16]).problem()
    assert off["strfn"] == dict(interval=-1, pmax=4, rmax=(-1, -1, -1), file="sf")
    on = Inputs([TG16], ["ns.strfn_interval=5", "ns.strfn_pmax=6", "ns.strfn_rmax=4 0 -1", "ns.strfn_file=out/S"]).problem()
    assert on["strfn"] == dict(interval=5, pmax=6, rmax=(4, 0, -1), file="out/S")
    assert on["params"] == off["params"] and not any("strfn" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "strfn"} == {k: v for k, v in off.items() if k != "strfn"}
    assert Inputs([TG16], ["ns.strfn_rmax=3"]).problem()["strfn"]["rmax"] == (3, 3, 3)
    # walls and extents that are no powers of two are fine: the cavity, with the longest separation of a wall axis
    ldc = Inputs([LDC], ["ns.strfn_interval=1", "ns.strfn_rmax=15"]).problem()
    assert ldc["strfn"]["interval"] == 1 and ldc["strfn"]["rmax"] == (15, 15, 15)
    assert Inputs([TG16], ["ns.strfn_interval=1", "amr.n_cell=16 24 16", "amr.max_level=0"]).problem()["strfn"]["interval"] == 1
    forced = Inputs([FORCED], ["ns.strfn_interval=2"]).problem()
    assert forced["strfn"] == dict(interval=2, pmax=4, rmax=(-1, -1, -1), file="sf")
    assert Inputs([POIS2D], ["ns.strfn_interval=0"]).problem()["strfn"]["interval"] == 0


def test_strfn_refusals_name_the_reason():
    from iamr_amd.inputs import Inputs
    with pytest.raises(ValueError, match=r"pmax = 9"):
        Inputs([TG16], ["ns.strfn_pmax=9"]).problem()
    with pytest.raises(ValueError, match=r"pmax = 0"):
        Inputs([TG16], ["ns.strfn_interval=1", "ns.strfn_pmax=0"]).problem()
    with pytest.raises(ValueError, match=r"rmax_y = 9"):                            # periodic 16: n / 2 = 8
        Inputs([TG16], ["ns.strfn_interval=1", "ns.strfn_rmax=8 9 8"]).problem()
    with pytest.raises(ValueError, match=r"rmax_x = 16"):                           # walls, 16 cells: n - 1 = 15
        Inputs([LDC], ["ns.strfn_interval=1", "ns.strfn_rmax=16"]).problem()
    with pytest.raises(ValueError, match=r"rmax_z = -2"):
        Inputs([TG16], ["ns.strfn_rmax=1 1 -2"]).problem()
    with pytest.raises(ValueError, match="one or three"):
        Inputs([TG16], ["ns.strfn_rmax=1 2"]).problem()
    with pytest.raises(NotImplementedError, match="two-dimensional"):               # a slab file, like ns.spectrum_interval
        Inputs([POIS2D], ["ns.strfn_interval=1"]).problem()


# ------------------------------------------------------------------------------------------------------------------ 4. dict, files
def cosine_level(n, m, pmax=4):
    """the raw dict a level would return for u = cos(2 pi m i / n_x), v = cos(2 pi m j / n_y), w = cos(2 pi m k / n_z), c = 0.25 + u"""
    from iamr_amd import strfn as S
    per = (1, 1, 1)
    fields = [SF.cosine(n, 0, m), SF.cosine(n, 1, m), SF.cosine(n, 2, m), 0.25 + SF.cosine(n, 0, m)]
    refs = [SF.reference(f, per, pmax) for f in fields]
    avg = np.stack([r[0] for r in refs], axis=1)
    rm = SF.resolve(n, per, (-1, -1, -1))
    return S.raw_dict(avg, refs[0][1], [r[3] for r in refs], n, (1.0, 2.0, 4.0), per, pmax, rm)


def test_derived_scales_on_the_cosine_field():
    """u_d = cos(2 pi i_d / 16): u'^2 = 1/2, f(r) = cos(pi r / 8) with its first zero at r = 4, so the integral scale is the trapezoid
    dx (1/2 + cos(pi/8) + cos(pi/4) + cos(3 pi/8)) and lambda^2 = dx^2 / (1 - cos(pi/8)); the transverse components are constant
    along d: g has no variance to be normalised with"""
    from iamr_amd import strfn as S
    n = (16, 16, 16)
    s = S.derive(cosine_level(n, 1))
    trap = 0.5 + math.cos(math.pi / 8) + math.cos(math.pi / 4) + math.cos(3 * math.pi / 8)
    for d in range(3):
        dx = s["dx"][d]
        assert dx == (1.0, 2.0, 4.0)[d] / 16
        assert np.max(np.abs(s["f"][d] - np.cos(np.pi * np.arange(9) / 8))) <= 4 * CLOSED
        assert abs(s["integral_scale"][d] - trap * dx) <= 8 * CLOSED * dx
        assert abs(s["taylor_scale"][d] - dx / math.sqrt(1.0 - math.cos(math.pi / 8))) <= 64 * CLOSED * dx
        assert np.array_equal(s["SL"][d, 2], s["avg"][d, d, 2]) and np.array_equal(s["SLabs"][d, 3], s["avg"][d, d, 6])
        assert not s["SLabs"][d, 2].any() and not s["SL"][d, 0].any()
        a, b = [q for q in range(3) if q != d]
        assert np.array_equal(s["ST"][d, 2], 0.5 * (s["avg"][d, a, 2] + s["avg"][d, b, 2])) and not s["ST"][d, 2].any()
        assert np.array_equal(s["RT"][d], 0.5 * (s["avg"][d, a, 0] + s["avg"][d, b, 0]))
        assert np.array_equal(s["Sc"][d, 2], s["avg"][d, 3, 2]) and np.array_equal(s["Rc"][d], s["avg"][d, 3, 0])
    assert np.max(np.abs(s["Sc"][0, 2] - s["SL"][0, 2])) <= CLOSED                 # a shifted copy of u: the same differences
    assert S.integral_scale(np.array([1.0, 0.5, -0.5, 1.0]), 2.0, 3) == 2.0 * (0.75 + 0.5 * 0.5 * 0.5)
    assert S.integral_scale(np.array([1.0, 0.5, 0.25]), 1.0, 2) == 0.75 + 0.375


def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import strfn as S
    rng = np.random.default_rng(5)
    n, per, pmax, rm = (12, 6, 10), (1, 0, 1), 5, (6, 0, 3)
    ncol, rcap = S.ncol_of(pmax), 7
    avg = rng.standard_normal((3, 4, ncol, rcap)) * 10.0 ** rng.integers(-30, 3, size=(3, 4, ncol, rcap))
    count = rng.integers(1, 10 ** 9, size=(3, rcap))
    avg[:, :, 0, 0] = np.abs(avg[:, :, 0, 0]) + 1.0                                 # R(0) above mean^2: a variance to normalise with
    for d in range(3):                                                              # nothing beyond an axis's rmax, nothing on a skipped axis
        avg[d, :, :, rm[d] + 1 if rm[d] > 0 else 0:] = 0.0
        count[d, rm[d] + 1 if rm[d] > 0 else 0:] = 0
    s = S.derive(S.raw_dict(avg, count, 0.1 * rng.standard_normal(4), n, (1.0, 0.5, 2.0), per, pmax, rm))
    path = str(tmp_path / "sf00007")
    S.write_strfn(path, s, 7, 0.1 + 0.2)
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head == lines[:len(head)] and len(lines) == len(head) + (6 + 1) + (3 + 1)
    assert head[0] == "# step = 7" and head[2] == "# n = 12 6 10" and head[5] == "# pmax = 5" and head[6] == "# rmax = 6 0 3"
    assert [l.split()[:2] for l in lines[len(head):]] == [["0", str(r)] for r in range(7)] + [["2", str(r)] for r in range(4)]
    assert all(len(l.split()) == 3 + 4 * ncol for l in lines[len(head):])
    r = S.read_strfn(path)
    assert (r["step"], r["time"], r["n"], r["L"], r["periodic"], r["pmax"], r["rmax"]) == (7, 0.1 + 0.2, n, (1.0, 0.5, 2.0), per, pmax, rm)
    assert sorted(r) == sorted(list(s) + ["step", "time"])
    assert r["count"].dtype == np.int64 and np.array_equal(r["count"], s["count"])
    for key in s:
        if isinstance(s[key], np.ndarray):
            assert r[key].dtype == s[key].dtype and r[key].tobytes() == s[key].tobytes(), key
        else:
            assert r[key] == s[key], key
