"""Host side of the way back from mode space (iamr_amd/spectral.py, include/iamrx.h, tests/specop_numpy.py): the entries are declared
and exported; the yardstick stays inside its own bounds when its transforms are replaced by the independent radix-2 one; the model
spectrum, the table reader, the inputs of prob.probtype = 101 and the statistics of the noise.  No GPU."""
import math
import os
import re
import numpy as np
import pytest
import spectrum_numpy as SN
import specop_numpy as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY = os.path.join(ROOT, "tests", "golden", "inputs.3d.decay16")
UNIT = (1.0, 1.0, 1.0)
SHAPES = [((8, 16, 32), UNIT), ((16, 16, 16), UNIT)]


def test_header_declares_and_library_exports_the_entries():
    from iamr_amd import lib
    from iamr_amd.ns import NavierStokes
    from iamr_amd.amr import Amr
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    L = lib.lib()
    for name in ("iamrx_mf_noise", "iamrx_mf_filter", "iamrx_mf_solenoidal", "iamrx_mf_synthesize", "iamrx_specop_bench", "iamrx_specop_bench_np"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(L, name), name
    assert L.iamrx_specop_bench_np() == 17
    for f in (lib.mf_noise, lib.mf_filter, lib.mf_solenoidal, lib.mf_synthesize, NavierStokes.filtered, Amr.filtered):
        assert callable(f)


@pytest.mark.parametrize("n,L", SHAPES)
def test_yardstick_holds_its_filter_bound(n, L):
    f = SO.noise(n, 5, 1)[..., 0] + 0.25
    for kind, kc in ((0, 1.0), (1, 4.5), (2, 3.0), (3, 3.0)):
        a = SO.filter_reference(f, L, kind, kc)
        b = SO.filter_reference(f, L, kind, kc, SO.r2_fwd, SO.r2_inv)
        err, bd = SO.norm2(a - b), SO.filter_bound(f)
        print(f"{n} kind {kind}: ||numpy - radix2|| = {err:.3e}, bound {bd:.3e}")
        assert err <= bd
    assert SO.norm2(SO.filter_reference(f, L, 0, 1.0) - f) <= SO.filter_bound(f)


@pytest.mark.parametrize("n,L", SHAPES)
def test_yardstick_holds_its_projection_bounds(n, L):
    f = SO.noise(n, 6, 3)
    for wn in (0, 1):
        a = SO.solenoidal_reference(f, L, wn)
        b = SO.solenoidal_reference(f, L, wn, SO.r2_fwd, SO.r2_inv)
        assert SO.norm2(a - b) <= SO.projection_bound(f)
        assert SO.norm2(SO.solenoidal_reference(a, L, wn) - a) <= SO.projection_bound(f)         # idempotent
    c = SO.solenoidal_reference(f, L, 1)
    rms = SO.norm2(SO.centred_divergence(c, L)) / math.sqrt(c[..., 0].size)
    bd = SO.divergence_bound(f, c, L)
    e = SO.solenoidal_reference(f, L, 0)
    rms_e = SO.norm2(SO.centred_divergence(e, L)) / math.sqrt(c[..., 0].size)
    print(f"{n}: centred divergence rms {rms:.3e} (bound {bd:.3e}); of the exact projection {rms_e:.3e}")
    assert rms <= bd and rms_e > 1000.0 * bd
    # what the exact projection still removes from the centred-projected field: the mode-by-mode expression
    removed = SO.norm2(SO.solenoidal_reference(c, L, 0) - c)
    want = SO.cross_removed(c, L, 0)
    assert want > 1e-3 * SO.norm2(c) and abs(removed - want) <= SO.projection_bound(f)


@pytest.mark.parametrize("n,L", SHAPES)
def test_yardstick_holds_its_synthesis_bounds(n, L):
    from iamr_amd.spectral import hit_spectrum
    s, nbins, _ = SN.shell_index(n, L)
    E = hit_spectrum(nbins, L, 3.0, 1.0, n=n)
    N = n[0] * n[1] * n[2]
    a, info = SO.synth_reference(n, L, 42, E, 1)
    b, _ = SO.synth_reference(n, L, 42, E, 1, SO.r2_fwd, SO.r2_inv)
    err, bd = SO.norm2(a - b) / math.sqrt(N), SO.synth_field_bound(E, info, N)
    print(f"{n}: synthesis numpy against radix2 {err:.3e}, bound {bd:.3e}")
    assert err <= bd
    got = 0.5 * sum(SN.spectrum_reference(np.ascontiguousarray(a[..., c]), L)[0] for c in range(3))
    sb = SO.synth_spectrum_bound(E, info, N)
    assert np.all(np.abs(got - E) <= sb) and got[0] <= sb[0]
    c = SO.centred_divergence(a, L)
    assert SO.norm2(c) / math.sqrt(N) <= 1e-9 * math.sqrt(3.0) * max(n)               # solenoidal for the centred difference


def test_yardstick_refuses_an_empty_shell():
    """4^3 cells on a 1 x 1 x 4 box: kappa^2 = 16 m_x^2 + 16 m_y^2 + m_z^2 has no value in [2.5^2, 3.5^2), shell 3 holds no mode"""
    n, L = (4, 4, 4), (1.0, 1.0, 4.0)
    s, nbins, _ = SN.shell_index(n, L)
    count = np.bincount(s.ravel(), minlength=nbins)
    assert count[3] == 0 and count[2] > 0
    E = np.zeros(nbins)
    E[2] = 1.0
    SO.synth_reference(n, L, 1, E, 1)
    E[3] = 1.0
    with pytest.raises(ValueError, match="empty"):
        SO.synth_reference(n, L, 1, E, 1)


def test_hit_spectrum_and_table_reader(tmp_path):
    from iamr_amd.spectral import hit_spectrum, read_spectrum_table, write_spectrum_table
    from iamr_amd.spectrum import nbins_of
    n = (64, 64, 64)
    nb = nbins_of(n, UNIT)
    for k0, urms0 in ((4.0, 1.0), (6.0, 0.5)):
        E = hit_spectrum(nb, UNIT, k0, urms0, n=n)
        want = 1.5 * urms0 * urms0
        assert abs(math.fsum(E) - want) <= 4.0 * 2.0 ** -53 * want
        assert int(np.argmax(E)) == int(k0) and E[0] == 0.0 and not E[33:].any() and E[32] > 0.0
        raw = hit_spectrum(nb, UNIT, k0, urms0, normalize=False)
        assert abs(math.fsum(raw) - want) <= 1e-3 * want                      # the integral of the model, sampled with dk = 1
    E = hit_spectrum(nb, UNIT, 4.0, 1.0, n=n)
    p = tmp_path / "table.txt"
    write_spectrum_table(str(p), E)
    back = read_spectrum_table(str(p), nb)
    assert back.tobytes() == E.tobytes()
    p2 = tmp_path / "coarse.csv"
    p2.write_text("k, E\n0, 5.0\n2, 1.0\n4, 3.0\n")
    assert list(read_spectrum_table(str(p2), 7)) == [0.0, 3.0, 1.0, 2.0, 3.0, 0.0, 0.0]
    p2.write_text("2 1.0\n1 3.0\n")
    with pytest.raises(ValueError, match="increase"):
        read_spectrum_table(str(p2), 7)


def test_inputs_parse_and_refuse():
    from iamr_amd.inputs import Inputs
    pr = Inputs([DECAY]).problem()
    pb = pr["prob"]
    assert pb["probtype"] == 101 and pb["k0"] == 3.0 and pb["urms0"] == 1.0 and pb["seed"] == 42 and pb["wavenumber"] == "centred"
    assert pb["density_ic"] == 1.0 and pb["spectrum_file"] == "" and pr["spectrum"]["interval"] == 1 and tuple(pr["n"]) == (16, 16, 16)
    assert Inputs([DECAY], ["hit.wavenumber=exact", "hit.seed=7"]).problem()["prob"]["wavenumber"] == "exact"
    with pytest.raises(ValueError, match="periodic"):
        Inputs([DECAY], ["geometry.is_periodic=1 0 1", "ns.lo_bc=0 4 0", "ns.hi_bc=0 4 0", "ns.spectrum_interval=-1"]).problem()
    with pytest.raises(ValueError, match="n_y = 12"):
        Inputs([DECAY], ["amr.n_cell=16 12 16", "ns.spectrum_interval=-1"]).problem()
    with pytest.raises(NotImplementedError, match="max_level"):
        Inputs([DECAY], ["amr.max_level=1", "amr.regrid_file=" + os.path.join(ROOT, "tests", "golden", "fixed_grids_3d_tg")]).problem()
    with pytest.raises(ValueError, match="wavenumber"):
        Inputs([DECAY], ["hit.wavenumber=staggered"]).problem()
    with pytest.raises(NotImplementedError, match="101"):
        Inputs([DECAY], ["prob.probtype=3"]).problem()
    with pytest.raises(KeyError, match=r"hit\."):                                  # the keys belong to probtype 101 alone
        Inputs([DECAY], ["prob.probtype=11"]).problem()


def test_inputs_refuse_two_dimensions(tmp_path):
    from iamr_amd.inputs import Inputs
    with pytest.raises(NotImplementedError, match="101.*two-dimensional"):
        Inputs([os.path.join(ROOT, "tests", "golden", "inputs.2d.doubleshearlayer_c3")], ["prob.probtype=101"]).problem()


def test_noise_statistics():
    n = (32, 32, 32)
    N = 32 ** 3
    w = SO.noise(n, 11, 2)
    assert w.min() > -0.5 and w.max() < 0.5
    for c in range(2):
        v = w[..., c].ravel()
        se_mean = math.sqrt(1.0 / 12.0 / N)
        se_var = math.sqrt((1.0 / 80.0 - 1.0 / 144.0) / N)                        # var(x^2) = E x^4 - (E x^2)^2 of the uniform law
        assert abs(v.mean()) <= 5.0 * se_mean and abs(np.mean(v * v) - 1.0 / 12.0) <= 5.0 * se_var
    assert not np.array_equal(w[..., 0], w[..., 1])
    assert not np.array_equal(SO.noise(n, 12, 1)[..., 0], w[..., 0])
    assert np.array_equal(SO.noise(n, 11, 1)[..., 0], w[..., 0])
    # the definition, spelled out for one cell in Python integers: seed 11, c = 1, o = 5 + 32 (6 + 32 * 7)
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    h = mix((mix(11 ^ ((2 * 0x9E3779B97F4A7C15) & M)) + 5 + 32 * (6 + 32 * 7)) & M)
    assert w[5, 6, 7, 1] == ((h >> 12) + 0.5) * 2.0 ** -52 - 0.5
