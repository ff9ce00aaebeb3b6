"""CPU suite: plane-averaged profiles (iamr_amd/profile.py, the ns.profile_* keys of iamr_amd/inputs.py, the entries of
include/iamrx.h) -- everything about them that needs no device.  The numpy restatement the GPU tests compare with
(tests/profile_numpy.py) is itself checked here on a case whose answer is written out."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import profile_numpy as PN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")


# ------------------------------------------------------------------------------------------------------------------ 1. the restatement
def _row_case():
    """a coarse row of 4 cells (4 x 1 x 1) with a fine patch over the coarse cells 1 and 2: fine cells 2..5 x 2 x 2.  rho = 1, 2, 3, 4 on
    the coarse row (cells 1, 2 are covered: NaN, they must not be read); on the fine patch rho = 10 i + j + 2 k; u = rho / 2"""
    S0 = np.zeros((4, 1, 1, 5))
    S0[:, 0, 0, 3] = [1.0, np.nan, np.nan, 4.0]
    S0[:, 0, 0, 0] = S0[:, 0, 0, 3] / 2
    S1 = np.full((8, 2, 2, 5), np.nan)
    i, j, k = np.meshgrid(np.arange(2, 6), np.arange(2), np.arange(2), indexing="ij")
    S1[2:6] = 0.0
    S1[2:6, :, :, 3] = 10.0 * i + j + 2.0 * k
    S1[2:6, :, :, 0] = S1[2:6, :, :, 3] / 2
    boxes = [[((0, 0, 0), (3, 0, 0))], [((2, 0, 0), (5, 1, 1))]]
    return [S0, S1], boxes, [4, 1, 1]


def test_restatement_on_a_hand_made_row():
    states, boxes, n0 = _row_case()
    q = {n: i for i, n in enumerate(PN.NAMES)}
    # fine planes i = 2..5: rho over (j, k) = 10 i + {0, 1, 2, 3}: mean 10 i + 1.5, mean of squares (10 i + 1.5)^2 + 1.25
    fine = {i: 10.0 * i + 1.5 for i in range(2, 6)}
    fine2 = {i: fine[i] ** 2 + 1.25 for i in fine}
    # B = 0: four bins; bin 1 = fine planes 2, 3 (8 cells), bin 2 = fine planes 4, 5
    mean, N, meanabs = PN.profile_reference(states, boxes, n0, 0, 0)
    assert mean.shape == (14, 4) and list(N) == [1, 8, 8, 1]
    assert list(mean[q["one"]]) == [1.0, 1.0, 1.0, 1.0]
    assert list(mean[q["rho"]]) == [1.0, (fine[2] + fine[3]) / 2, (fine[4] + fine[5]) / 2, 4.0]
    assert list(mean[q["rhorho"]]) == [1.0, (fine2[2] + fine2[3]) / 2, (fine2[4] + fine2[5]) / 2, 16.0]
    assert list(mean[q["u"]]) == [0.5, (fine[2] + fine[3]) / 4, (fine[4] + fine[5]) / 4, 2.0]
    assert list(mean[q["uu"]]) == [0.25, (fine2[2] + fine2[3]) / 8, (fine2[4] + fine2[5]) / 8, 4.0]
    assert not mean[q["v"]].any() and not mean[q["c"]].any() and not mean[q["uv"]].any()
    assert np.array_equal(meanabs[q["rho"]], mean[q["rho"]])
    # B = 1: eight bins; a coarse cell spreads over two of them, a fine plane is a bin
    mean, N, _ = PN.profile_reference(states, boxes, n0, 0, 1)
    assert mean.shape == (14, 8) and list(N) == [1, 1, 4, 4, 4, 4, 1, 1]
    assert list(mean[q["one"]]) == [1.0] * 8
    assert list(mean[q["rho"]]) == [1.0, 1.0, fine[2], fine[3], fine[4], fine[5], 4.0, 4.0]
    assert list(mean[q["rhorho"]]) == [1.0, 1.0, fine2[2], fine2[3], fine2[4], fine2[5], 16.0, 16.0]
    # the sum over the bins is conservative: (mean * slab volume) summed = the composite integral, for either bin level
    vol = (1.0 + 4.0) + 0.125 * sum(4 * fine[i] for i in fine)      # coarse cells of volume 1, fine cells of volume 1 / 8
    for B in (0, 1):
        m = PN.profile_reference(states, boxes, n0, 0, B)[0][q["rho"]]
        assert float(np.sum(m)) * (4.0 / len(m)) == vol
    # along the other axes there is one level-0 bin: the whole composite
    for d in (1, 2):
        mean, N, _ = PN.profile_reference(states, boxes, n0, d, 0)
        assert mean.shape == (14, 1) and N[0] == 18 and mean[q["one"], 0] == 1.0 and mean[q["rho"], 0] == vol / 4.0
    # a NaN in a counted cell reaches the bins of that cell and no other
    states[0][3, 0, 0, 0] = np.nan
    mean, _, _ = PN.profile_reference(states, boxes, n0, 0, 1)
    bad = np.isnan(mean)
    assert sorted(PN.NAMES[i] for i in np.where(bad.any(axis=1))[0]) == ["u", "uu", "uv", "uw"]
    assert list(np.where(bad.any(axis=0))[0]) == [6, 7]


# ------------------------------------------------------------------------------------------------------------------ 2. inputs
def test_profile_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([LDC]).problem()
    assert off["profile"] == dict(interval=-1, dir=2, level=0, file="prof")
    on = Inputs([LDC], ["ns.profile_interval=10", "ns.profile_dir=0", "ns.profile_level=3", "ns.profile_file=out/zmean"]).problem()
    assert on["profile"] == dict(interval=10, dir=0, level=3, file="out/zmean")
    assert on["params"] == off["params"] and not any("profile" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "profile"} == {k: v for k, v in off.items() if k != "profile"}
    # a two-dimensional file names the 2-D directions; they are lifted as gravity is: x -> x, y -> z
    assert Inputs([POIS2D]).problem()["profile"]["dir"] == 2
    assert Inputs([POIS2D], ["ns.profile_dir=1"]).problem()["profile"]["dir"] == 2
    assert Inputs([POIS2D], ["ns.profile_dir=0"]).problem()["profile"]["dir"] == 0
    for files, d in (([LDC], 3), ([LDC], -1), ([POIS2D], 2)):
        with pytest.raises(ValueError, match="profile_dir"):
            Inputs(files, [f"ns.profile_dir={d}"]).problem()
    with pytest.raises(ValueError, match="profile_level"):
        Inputs([LDC], ["ns.profile_level=-1"]).problem()


# ------------------------------------------------------------------------------------------------------------------ 3. files, stresses
def _made_up(nbins=7, seed=3):
    from iamr_amd import profile as P
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal(14 * nbins) * 10.0 ** rng.integers(-12, 12, size=14 * nbins)
    return P.as_dict(raw, nbins, -0.3, 1.1, 1, 2), raw.reshape(14, nbins)


def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import profile as P
    p, raw = _made_up()
    assert p["names"] == P.NAMES == PN.NAMES and len(P.NAMES) == 14
    assert np.array_equal(p["coord"], -0.3 + (np.arange(7) + 0.5) * ((1.1 + 0.3) / 7))
    path = str(tmp_path / "prof00010")
    P.write_profile(path, p, 10, 0.1 + 0.2)
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head == lines[:len(head)] and len(lines) == len(head) + 7
    assert head[-1] == "# columns = coord " + " ".join(P.NAMES)
    assert all(len(l.split()) == 15 for l in lines[len(head):])
    r = P.read_profile(path)
    assert (r["step"], r["time"], r["dir"], r["bin_level"], r["names"]) == (10, 0.1 + 0.2, 1, 2, P.NAMES)
    for q, n in enumerate(P.NAMES):
        assert r[n].dtype == np.float64 and r[n].tobytes() == raw[q].tobytes(), n
    assert r["coord"].tobytes() == p["coord"].tobytes()


def test_reynolds_stresses():
    from iamr_amd import profile as P
    rng = np.random.default_rng(11)
    # three bins of samples: the profile is made of their plain means, the stresses must be their covariances
    X = rng.standard_normal((3, 500, 5)) + np.array([1.0, -2.0, 0.5, 3.0, 0.25])
    Q = PN.quantities(X).mean(axis=1).T                                    # (14, 3)
    p = P.as_dict(Q.ravel(), 3, 0.0, 1.0, 2, 0)
    R = P.reynolds_stresses(p)
    assert sorted(R) == sorted(["uu", "vv", "ww", "uv", "uw", "vw", "rhorho", "cc"])
    for key, (a, b) in dict(uu=(0, 0), vv=(1, 1), ww=(2, 2), uv=(0, 1), uw=(0, 2), vw=(1, 2), rhorho=(3, 3), cc=(4, 4)).items():
        cov = np.array([np.mean((X[k, :, a] - X[k, :, a].mean()) * (X[k, :, b] - X[k, :, b].mean())) for k in range(3)])
        assert R[key].shape == (3,) and np.allclose(R[key], cov, rtol=0, atol=1e-12), key
    assert np.all(R["uu"] > 0.5) and np.all(R["rhorho"] > 0.5)


# ------------------------------------------------------------------------------------------------------------------ 4. header, library
def test_header_declares_and_library_exports_the_entries():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    L = lib.lib()
    for name, args in (("iamrx_profile_nq", r"void"),
                       ("iamrx_ns_plane_profile", r"iamrx_ns\s+\w+,\s*int\s+dir,\s*int\s+nbins_cap,\s*double\s*\*\s*out,\s*int\s*\*\s*nbins"),
                       ("iamrx_amr_plane_profile", r"iamrx_amr\s+\w+,\s*int\s+dir,\s*int\s+bin_level,\s*int\s+nbins_cap,\s*double\s*\*\s*out,\s*int\s*\*\s*nbins")):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", txt), name
        assert hasattr(L, name), name
    assert L.iamrx_profile_nq() == 14
    # the struct the parameters travel in is untouched: the keys live outside it
    from iamr_amd.ns import ns_params
    assert not [f for f, _ in type(ns_params())._fields_ if "profile" in f]
