"""CPU suite: shell-summed spectra (iamr_amd/spectrum.py, the ns.spectrum_* keys of iamr_amd/inputs.py, the entries of
include/iamrx.h) -- everything about them that needs no device.  The numpy yardstick the GPU tests compare with
(tests/spectrum_numpy.py) is itself checked here: against Parseval, on a single cosine mode whose answer is written out, and its bound
against an independent radix-2 transform."""
import math
import os
import re
import numpy as np
import pytest
import spectrum_numpy as SN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TG16 = os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")


# ------------------------------------------------------------------------------------------------------------------ 1. the yardstick
@pytest.mark.parametrize("n,L", SN.SHAPES)
def test_yardstick_parseval_and_bound(n, L):
    """sum of P over the shells = mean(f^2); count sums to N; the shapes of the GPU tests keep every mode away from a shell boundary; an
    independent radix-2 transform stays far inside the bound (printed)"""
    f = SN.noise(n, 3)[..., 0]
    N = f.size
    P, count = SN.spectrum_reference(f, L)
    s, nbins, dist = SN.shell_index(n, L)
    assert len(P) == len(count) == nbins and int(count.sum()) == N and count[0] == 1
    assert dist > 4e-3
    msq = math.fsum((f * f).ravel()) / N
    assert abs(math.fsum(P) - msq) <= SN.eps_of(N) * msq
    assert abs(P[0] - float(np.mean(f)) ** 2) <= SN.eps_of(N) * P[0]
    P2, c2 = SN.shell_sums(SN.radix2(f), s, nbins)
    worst = float(np.max(np.abs(P2 - P) / SN.bound(P, count, N)))
    print(f"{n} L {L}: {nbins} shells, closest mode to a shell boundary {dist:.2e}, radix-2 against numpy: worst error / bound = {worst:.4f}")
    assert np.array_equal(c2, count) and worst <= 0.006


def test_yardstick_single_cosine_mode():
    """cos(2 pi (3 i + 4 j) / 16) of amplitude 1: |m| = 5, P(5) = 1/2, nothing anywhere else"""
    n, L = (16, 16, 16), (1.0, 1.0, 1.0)
    P, count = SN.spectrum_reference(SN.cosine_mode(n), L)
    eps = SN.eps_of(16 ** 3)
    assert len(P) == 15 and abs(P[5] - 0.5) <= SN.bound(P, count, 16 ** 3)[5]
    assert float(np.delete(P, 5).max()) <= eps * eps * 0.5
    # a non-cubic domain stretches the shell index: L = (1, 1, 2) doubles m_x and m_y, so (3, 4, 0) lies in shell 10
    P2, _ = SN.spectrum_reference(SN.cosine_mode((16, 16, 32)), (1.0, 1.0, 2.0))
    assert int(np.argmax(P2)) == 10 and abs(P2[10] - 0.5) <= 1e-15


def test_yardstick_refuses_a_tie():
    """L = (1, 1, 1.5) at 8^3 gives r_x = 1.5 and puts the mode (1, 0, 0) at kappa = 1.5: either shell would be right, so the yardstick
    refuses the shape"""
    with pytest.raises(AssertionError):
        SN.shell_index((8, 8, 8), (1.0, 1.0, 1.5))


def test_python_shell_count_is_the_yardsticks():
    from iamr_amd import spectrum as S
    for n, L in SN.SHAPES + (((256, 256, 256), (1.0, 1.0, 1.0)), ((128, 64, 32), (2.0, 1.0, 0.5))):
        c = [float(-(v // 2)) * (max(L) / l) for v, l in zip(n, L)]
        assert S.nbins_of(n, L) == int(math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + 0.5) + 1
    assert S.nbins_of((32, 32, 32), (1, 1, 1)) == SN.shell_index((32, 32, 32), (1, 1, 1))[1] == 29
    assert [S.extent_ok(v) for v in (2, 4, 24, 64, 1024, 2048, 0)] == [False, True, False, True, True, False, False]


# ------------------------------------------------------------------------------------------------------------------ 2. inputs
def test_spectrum_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([TG16]).problem()
    assert off["spectrum"] == dict(interval=-1, file="spec")
    on = Inputs([TG16], ["ns.spectrum_interval=5", "ns.spectrum_file=out/Ek"]).problem()
    assert on["spectrum"] == dict(interval=5, file="out/Ek")
    assert on["params"] == off["params"] and not any("spectrum" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "spectrum"} == {k: v for k, v in off.items() if k != "spectrum"}
    # the keys alone change nothing else, and a file that cannot have a spectrum still parses without them or with the interval off
    assert Inputs([LDC]).problem()["spectrum"]["interval"] == -1
    assert Inputs([LDC], ["ns.spectrum_interval=-1", "ns.spectrum_file=x"]).problem()["spectrum"] == dict(interval=-1, file="x")
    assert Inputs([POIS2D], ["ns.spectrum_interval=0"]).problem()["spectrum"]["interval"] == 0


def test_spectrum_refusals_name_the_reason():
    from iamr_amd.inputs import Inputs
    with pytest.raises(ValueError, match="periodic"):                               # walls all round
        Inputs([LDC], ["ns.spectrum_interval=1"]).problem()
    with pytest.raises(ValueError, match=r"n_y = 24"):                              # not a power of two
        Inputs([TG16], ["ns.spectrum_interval=1", "amr.n_cell=16 24 16", "amr.max_level=0"]).problem()
    with pytest.raises(NotImplementedError, match="two-dimensional"):               # a slab file, like ns.avg_interval
        Inputs([POIS2D], ["ns.spectrum_interval=1"]).problem()


# ------------------------------------------------------------------------------------------------------------------ 3. files
def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import spectrum as S
    rng = np.random.default_rng(5)
    nb = S.nbins_of((16, 16, 32), (1.0, 1.0, 2.0))
    P = np.abs(rng.standard_normal((4, nb))) * 10.0 ** rng.integers(-30, 3, size=(4, nb))
    count = rng.integers(1, 10 ** 9, size=nb)
    s = S.as_dict(P, count, (16, 16, 32), (1.0, 1.0, 2.0))
    assert sorted(s) == sorted(["k", "count", "E", "Euu", "Evv", "Eww", "Ecc", "n", "L"])
    assert np.array_equal(s["k"], np.arange(nb) * (2.0 * math.pi / 2.0))
    assert np.array_equal(s["Euu"], 0.5 * P[0]) and np.array_equal(s["Ecc"], 0.5 * P[3])
    assert np.array_equal(s["E"], 0.5 * ((P[0] + P[1]) + P[2]))
    path = str(tmp_path / "spec00007")
    S.write_spectrum(path, s, 7, 0.1 + 0.2)
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head == lines[:len(head)] and len(lines) == len(head) + nb
    assert head[0] == "# step = 7" and head[2] == "# n = 16 16 32" and head[-1] == "# columns = s k count E Euu Evv Eww Ecc"
    assert [l.split()[0] for l in lines[len(head):]] == [str(b) for b in range(nb)] and all(len(l.split()) == 8 for l in lines[len(head):])
    r = S.read_spectrum(path)
    assert (r["step"], r["time"], r["n"], r["L"]) == (7, 0.1 + 0.2, (16, 16, 32), (1.0, 1.0, 2.0))
    assert r["sum_E"] == math.fsum(s["E"])
    assert r["count"].dtype == np.int64 and np.array_equal(r["count"], count)
    for key in ("k", "E", "Euu", "Evv", "Eww", "Ecc"):
        assert r[key].dtype == np.float64 and r[key].tobytes() == s[key].tobytes(), key


# ------------------------------------------------------------------------------------------------------------------ 4. header, library
def test_header_declares_and_library_exports_the_entries():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    tail = r"int\s+nbins_cap,\s*double\s*\*\s*out,\s*long\s*\*\s*count,\s*int\s*\*\s*nbins"
    L = lib.lib()
    for name, args in (("iamrx_spectrum_nq", r"void"),
                       ("iamrx_mf_spectrum", r"const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+ncomp,\s*" + tail),
                       ("iamrx_ns_spectrum", r"iamrx_ns\s+ns,\s*" + tail),
                       ("iamrx_amr_spectrum", r"iamrx_amr\s+a,\s*" + tail)):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", txt), name
        assert hasattr(L, name), name
    assert L.iamrx_spectrum_nq() == 4
    from iamr_amd.ns import ns_params, NavierStokes
    from iamr_amd.amr import Amr
    assert not [f for f, _ in type(ns_params())._fields_ if "spectrum" in f]
    assert callable(NavierStokes.spectrum) and callable(Amr.spectrum) and callable(lib.mf_spectrum)
