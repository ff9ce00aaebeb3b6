"""CPU suite: plane spectra (iamr_amd/planespec.py, the ns.plane_spectrum_* keys of iamr_amd/inputs.py, the entries of include/iamrx.h)
-- everything about them that needs no device.  The numpy yardstick the GPU tests compare with (tests/planespec_numpy.py) is itself
checked here: Parseval per plane, the plane mean in ring 0, and its bound against an independent radix-2 transform."""
import math
import os
import re
import numpy as np
import pytest
import planespec_numpy as PS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT16 = os.path.join(HERE, "golden", "inputs.3d.rayleightaylor_planes16")
RT = os.path.join(HERE, "golden", "regtest.3d.rayleightaylor")
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")


# ------------------------------------------------------------------------------------------------------------------ 1. the yardstick
@pytest.mark.parametrize("n,L,dir", PS.SHAPES)
def test_yardstick_parseval_and_bound(n, L, dir):
    """per plane: the sum over the rings = the plane mean of f^2, ring 0 = the plane mean squared; count sums to M; every mode of the
    shapes of the GPU tests keeps away from a ring boundary; an independent radix-2 transform stays far inside the bound (printed)"""
    f = PS.noise(n, 3)[..., 0]
    a, b = PS.axes_of(dir)
    M = n[a] * n[b]
    P, count = PS.plane_spectrum_reference(f, L, dir)
    s, nrings, dist = PS.ring_index(n, L, dir)
    assert P.shape == (n[dir], nrings) and len(count) == nrings and int(count.sum()) == M and count[0] == 1
    assert dist > 4e-3
    fp = np.moveaxis(f, dir, 0)
    for p in range(n[dir]):
        msq = math.fsum((fp[p] * fp[p]).ravel()) / M
        assert abs(math.fsum(P[p]) - msq) <= PS.eps_of(M) * msq
        assert abs(P[p, 0] - (math.fsum(fp[p].ravel()) / M) ** 2) <= PS.eps_of(M) * msq
    P2, c2 = PS.power_from(PS.radix2(f, dir), n, L, dir)
    worst = float(np.max(np.abs(P2 - P) / PS.bound(P, count, M)))
    print(f"{n} L {L} dir {dir}: {nrings} rings, closest mode to a ring boundary {dist:.2e}, radix-2 against numpy: worst error / bound = {worst:.4f}")
    assert np.array_equal(c2, count) and worst <= 0.03


def test_yardstick_cosine_planes():
    """A(p) cos(2 pi (3 x_a + 4 x_b) / 16): P(p, 5) = A(p)^2 / 2 in every direction, nothing anywhere else"""
    for dir, n in ((2, (16, 16, 5)), (1, (16, 5, 16)), (0, (5, 16, 16))):
        amp = 1.0 + 0.5 * np.arange(5)
        P, count = PS.plane_spectrum_reference(PS.cosine_planes(n, dir, amp), PS.U3, dir)
        assert np.all(np.abs(P[:, 5] - 0.5 * amp * amp) <= PS.bound(P, count, 256)[:, 5])
        assert float(np.delete(P, 5, axis=1).max()) <= PS.eps_of(256) ** 2 * 0.5 * amp.max() ** 2


def test_yardstick_refuses_a_tie():
    """L_x = 1.5 L_y puts the mode (0, 1) at kappa = 1.5"""
    with pytest.raises(AssertionError):
        PS.ring_index((8, 8, 8), (1.5, 1.0, 1.0), 2)


def test_python_ring_count_is_the_yardsticks():
    from iamr_amd import planespec as P
    for n, L, dir in PS.SHAPES:
        assert P.nrings_of(n, L, dir) == PS.ring_index(n, L, dir)[1], (n, L, dir)
    assert P.nrings_of((4, 3, 1024), (1.0, 5.0, 2.0), 1) == PS.ring_index((4, 3, 1024), (1.0, 1e9, 2.0), 1)[1]          # the normal length does not enter
    assert [P.axes_of(d) for d in range(3)] == [(1, 2), (0, 2), (0, 1)]
    with pytest.raises(ValueError, match="outside 0 .. 2"):
        P.nrings_of((8, 8, 8), PS.U3, 3)


# ------------------------------------------------------------------------------------------------------------------ 2. inputs
def test_plane_spectrum_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([RT]).problem()
    assert off["plane_spectrum"] == dict(interval=0, dir=2, file="pspec")
    on = Inputs([RT], ["ns.plane_spectrum_interval=5", "ns.plane_spectrum_dir=2", "ns.plane_spectrum_file=out/Ekz"]).problem()
    assert on["plane_spectrum"] == dict(interval=5, dir=2, file="out/Ekz")
    assert on["params"] == off["params"] and not any("plane_spectrum" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "plane_spectrum"} == {k: v for k, v in off.items() if k != "plane_spectrum"}
    # with the interval off nothing is checked: walls all round, a two-dimensional file
    assert Inputs([LDC], ["ns.plane_spectrum_dir=1"]).problem()["plane_spectrum"] == dict(interval=0, dir=1, file="pspec")
    assert Inputs([POIS2D], ["ns.plane_spectrum_interval=0"]).problem()["plane_spectrum"]["interval"] == 0


def test_plane_spectrum_refusals_name_the_reason():
    from iamr_amd.inputs import Inputs
    with pytest.raises(ValueError, match=r"plane_spectrum: direction z is not periodic"):          # RT along x: z would be transformed
        Inputs([RT], ["ns.plane_spectrum_interval=1", "ns.plane_spectrum_dir=0"]).problem()
    with pytest.raises(ValueError, match=r"plane_spectrum: direction x is not periodic"):          # walls all round
        Inputs([LDC], ["ns.plane_spectrum_interval=1"]).problem()
    with pytest.raises(ValueError, match=r"plane_spectrum: extent n_y = 24 is not a power of two in 4 .. 1024"):
        Inputs([RT], ["ns.plane_spectrum_interval=1", "amr.n_cell=16 24 16", "amr.max_level=0"]).problem()
    with pytest.raises(ValueError, match=r"plane_spectrum: dir = 3 outside 0 .. 2"):
        Inputs([RT], ["ns.plane_spectrum_interval=1", "ns.plane_spectrum_dir=3"]).problem()
    with pytest.raises(NotImplementedError, match="two-dimensional"):
        Inputs([POIS2D], ["ns.plane_spectrum_interval=1"]).problem()
    # the normal extent needs no power of two
    assert Inputs([RT], ["ns.plane_spectrum_interval=1", "amr.n_cell=16 16 24", "amr.max_level=0"]).problem()["plane_spectrum"]["interval"] == 1


def test_the_new_fixture_parses():
    from iamr_amd.inputs import Inputs
    inp = Inputs([RT16])
    pr = inp.problem()
    assert pr["plane_spectrum"] == dict(interval=1, dir=2, file="pspec")
    assert tuple(pr["n"]) == (16, 16, 32) and [int(v) for v in pr["periodic"]] == [1, 1, 0] and pr["prob"]["probtype"] == 10
    assert pr.get("max_level", 0) == 0
    assert not [k for k in inp.ignored if "plane_spectrum" in k]
    dx = [(pr["prob_hi"][d] - pr["prob_lo"][d]) / pr["n"][d] for d in range(3)]
    assert dx[0] == dx[1] == dx[2]


# ------------------------------------------------------------------------------------------------------------------ 3. files
def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import planespec as S
    rng = np.random.default_rng(5)
    n, L, dir = (16, 8, 3), (2.0, 1.0, 1.5), 2
    nr = S.nrings_of(n, L, dir)
    P = np.abs(rng.standard_normal((5, 3, nr))) * 10.0 ** rng.integers(-30, 3, size=(5, 3, nr))
    count = rng.integers(1, 10 ** 9, size=nr)
    coord = 0.1 + 0.5 * (np.arange(3) + 0.5)
    s = S.as_dict(P, count, n, L, dir, coord)
    assert sorted(s) == sorted(["k", "count", "coord", "dir", "E", "Euu", "Evv", "Eww", "Err", "Ecc", "n", "L"])
    assert np.array_equal(s["k"], np.arange(nr) * (2.0 * math.pi / 2.0)) and s["dir"] == 2
    assert np.array_equal(s["Euu"], 0.5 * P[0]) and np.array_equal(s["Err"], 0.5 * P[3]) and np.array_equal(s["Ecc"], 0.5 * P[4])
    assert np.array_equal(s["E"], 0.5 * ((P[0] + P[1]) + P[2])) and s["E"].shape == (3, nr)
    path = str(tmp_path / "pspec00007")
    S.write_plane_spectrum(path, s, 7, 0.1 + 0.2)
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head == lines[:len(head)] and len(lines) == len(head) + 3 * nr
    assert head[0] == "# step = 7" and head[2] == "# n = 16 8 3" and "# dir = 2" in head and "# nplanes = 3" in head
    assert head[-1] == "# columns = p coord s k count E Euu Evv Eww Err Ecc"
    assert all(len(l.split()) == 11 for l in lines[len(head):])
    r = S.read_plane_spectrum(path)
    assert (r["step"], r["time"], r["n"], r["L"], r["dir"]) == (7, 0.1 + 0.2, n, L, 2)
    assert r["sum_E"] == math.fsum(s["E"].ravel())
    assert r["count"].dtype == np.int64 and np.array_equal(r["count"], count)
    for key in ("k", "coord", "E", "Euu", "Evv", "Eww", "Err", "Ecc"):
        assert r[key].dtype == np.float64 and r[key].shape == s[key].shape and r[key].tobytes() == s[key].tobytes(), key


# ------------------------------------------------------------------------------------------------------------------ 4. header, library
def test_header_declares_and_library_exports_the_entries():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    tail = (r"int\s+nplanes_cap,\s*int\s+nrings_cap,\s*double\s*\*\s*out,\s*long\s*\*\s*count,\s*int\s*\*\s*nplanes,\s*int\s*\*\s*nrings")
    L = lib.lib()
    for name, args in (("iamrx_plane_spectrum_nq", r"void"),
                       ("iamrx_mf_plane_spectrum", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+ncomp,\s*int\s+dir,\s*" + tail),
                       ("iamrx_mf_plane_cospectrum", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+a,\s*int\s+acomp,\s*iamrx_mf\s+b,\s*int\s+bcomp,\s*int\s+dir,\s*" + tail),
                       ("iamrx_ns_plane_spectrum", r"iamrx_ns\s+ns,\s*int\s+dir,\s*" + tail),
                       ("iamrx_amr_plane_spectrum", r"iamrx_amr\s+a,\s*int\s+dir,\s*" + tail),
                       ("iamrx_plane_spectrum_bench", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+dir,\s*int\s+reps,\s*float\s*\*\s*ms")):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", txt), name
        assert hasattr(L, name), name
    assert L.iamrx_plane_spectrum_nq() == 5
    from iamr_amd.ns import NavierStokes
    from iamr_amd.amr import Amr
    assert callable(NavierStokes.plane_spectrum) and callable(NavierStokes.plane_cospectrum) and callable(Amr.plane_spectrum)
    assert callable(lib.mf_plane_spectrum) and callable(lib.mf_plane_cospectrum)
