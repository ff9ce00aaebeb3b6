"""CPU suite: the a-priori LES analysis (iamr_amd/sgs.py, the ns.sgs_* keys of iamr_amd/inputs.py, the entries of include/iamrx.h) --
everything about it that needs no device.  The numpy yardstick the GPU tests compare with (tests/sgs_numpy.py) is itself checked
here: a single sine mode whose subgrid stress is written out for three sharp cut-offs, and Parseval's identity for <k_sgs> under all
four filter kinds."""
import math
import os
import re
import numpy as np
import pytest
import specop_numpy as SO
import sgs_numpy as GN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TG16 = os.path.join(HERE, "golden", "inputs.3d.taylorgreen_amr16")
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")
UNIT = (1.0, 1.0, 1.0)
ENTRIES = ("iamrx_sgs_nstat", "iamrx_mf_sgs", "iamrx_ns_sgs", "iamrx_amr_sgs", "iamrx_sgs_bench")


def header():
    return open(os.path.join(ROOT, "include", "iamrx.h")).read()


# ------------------------------------------------------------------------------------------------------------------ 1. the interface
def test_the_entries_are_declared_and_exported():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    tail = r"iamrx_mf\s+out,\s*int\s+ocomp,\s*int\s+nout,\s*const\s+int\s*\*\s*which,\s*double\s*\*\s*stats,\s*long\s*\*\s*counts\s*\)"
    assert re.search(r"int\s+iamrx_sgs_nstat\s*\(\s*void\s*\)", txt)
    assert re.search(r"int\s+iamrx_mf_sgs\s*\(\s*const\s+iamrx_geom\s*\*\s*g,\s*iamrx_mf\s+vel,\s*int\s+vcomp,\s*int\s+kind,\s*double\s+kc,\s*" + tail, txt)
    assert re.search(r"int\s+iamrx_ns_sgs\s*\(\s*iamrx_ns\s+ns,\s*int\s+kind,\s*double\s+kc,\s*" + tail, txt)
    assert re.search(r"int\s+iamrx_amr_sgs\s*\(\s*iamrx_amr\s+a,\s*int\s+kind,\s*double\s+kc,\s*" + tail, txt)
    assert re.search(r"int\s+iamrx_sgs_bench\s*\(", txt)
    L = lib.lib()
    missing = [s for s in ENTRIES if not hasattr(L, s)]
    assert not missing, missing
    assert L.iamrx_sgs_nstat() == 16


def test_names_agree_with_the_header_comment():
    from iamr_amd import sgs as G
    txt = header()
    a = txt.index(" * sgs statistics:")
    b = txt.index(" * sgs fields:")
    c = txt.index("int iamrx_sgs_nstat(void);")
    row = re.compile(r"^ \*\s+(\d+)\s+(\w+)\b", flags=re.M)
    stats = [(int(q), nm) for q, nm in row.findall(txt[a:b])]
    fields = [(int(q), nm) for q, nm in row.findall(txt[b:c])]
    assert stats == list(enumerate(G.STAT_NAMES)) and len(stats) == 16
    assert fields == list(enumerate(G.FIELD_NAMES)) and len(fields) == 10
    assert G.STAT_NAMES == GN.STAT_NAMES and G.FIELD_NAMES == GN.FIELD_NAMES          # the yardstick speaks of the same columns
    assert G.field_ids(["tau_yz", 7, "smag_flux"]) == [4, 7, 9] and G.field_ids("k_sgs") == [6] and G.field_ids(()) == []
    with pytest.raises(ValueError, match="field 'tau_zx', known are tau_xx"):
        G.field_ids(["tau_zx"])


# ------------------------------------------------------------------------------------------------------------------ 2. the yardstick
def sine_field(n=(8, 16, 8), A=1.5, a=2, phi=0.3):
    """u = (A sin(2 pi a j / n_y + phi), 0, 0) -> (f, theta (n_y,))"""
    theta = 2.0 * math.pi * a * np.arange(n[1]) / n[1] + phi
    f = np.zeros(n + (3,))
    f[..., 0] = (A * np.sin(theta))[None, :, None]
    return f, theta


def test_closed_forms_of_a_sine_mode():
    """u_x = A sin(theta), mode number a = 2 along y; u_x^2 = A^2 / 2 - (A^2 / 2) cos(2 theta) has modes 0 and 4.  Sharp filter:
    kc = 2.5 keeps u and drops the mode 4 of the square: tau_xx = (A^2 / 2) cos(2 theta); kc = 4.5 keeps everything: tau = 0;
    kc = 1.5 drops u and keeps the mean of the square: tau_xx = A^2 / 2, <k_sgs> = A^2 / 4, S = 0."""
    A = 1.5
    f, theta = sine_field(A=A)
    worst = 0.0
    r = GN.analyse(f, UNIT, 1, 2.5, strict=False)
    worst = max(worst, float(np.max(np.abs(r["fields"]["tau_xx"].v - (0.5 * A * A * np.cos(2.0 * theta))[None, :, None]))))
    r = GN.analyse(f, UNIT, 1, 4.5, strict=False)
    worst = max(worst, max(float(np.max(np.abs(r["fields"][nm].v))) for nm in GN.FIELD_NAMES[:7]))
    r = GN.analyse(f, UNIT, 1, 1.5, strict=False)
    worst = max(worst, float(np.max(np.abs(r["fields"]["tau_xx"].v - 0.5 * A * A))), abs(r["stats"][3] - 0.25 * A * A),
                float(np.max(np.abs(r["fields"]["filtered_strain"].v))))
    print(f"sine mode: worst deviation from the closed forms {worst:.3e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("kind,kc", [(0, 1.0), (1, 4.5), (2, 3.0), (3, 3.0)])
def test_subgrid_energy_is_parseval(kind, kc):
    n, L = (8, 16, 32), UNIT
    f = SO.noise(n, 21, 3) * 2.0 + np.array([0.3, -0.2, 0.1])
    r = GN.analyse(f, L, kind, kc)
    want = GN.ksgs_from_modes(f, L, kind, kc)
    print(f"kind {kind} kc {kc}: <k_sgs> = {r['stats'][3]:.6e}, Parseval {want:.6e}, difference {abs(r['stats'][3] - want):.3e}, bound {r['stat_bounds'][3]:.3e}")
    assert abs(r["stats"][3] - want) <= r["stat_bounds"][3]
    assert (kind == 0) == (abs(want) < 1e-12)


# ------------------------------------------------------------------------------------------------------------------ 3. the file
def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import sgs as G
    rng = np.random.default_rng(5)
    path = str(tmp_path / "sgs")
    rows = [(s, 0.1 * s + rng.random() * 1e-3, kc, rng.standard_normal(16) * 10.0 ** rng.integers(-12, 12, 16), (4096, int(rng.integers(0, 4096))))
            for s in (0, 2) for kc in (2.5, 4.5)]
    G.start_file(path)
    for r in rows[:2]:
        G.append_row(path, *r)
    G.start_file(path, append=True)                       # a restarted run keeps the rows
    for r in rows[2:]:
        G.append_row(path, *r)
    got = G.read_sgs(path)
    assert got["step"].tolist() == [0, 0, 2, 2] and got["kc"].tolist() == [2.5, 4.5, 2.5, 4.5]
    assert got["time"].tobytes() == np.array([r[1] for r in rows]).tobytes()
    assert got["stats"].tobytes() == np.array([r[3] for r in rows]).tobytes()
    for q, nm in enumerate(G.STAT_NAMES):
        assert got[nm].tobytes() == np.array([r[3][q] for r in rows]).tobytes()
    assert got["N"].tolist() == [4096] * 4 and got["negative_cells"].tolist() == [r[4][1] for r in rows]
    with open(path) as f:
        assert f.readline().rstrip("\n") == G.header_line() == "# step time kc " + " ".join(G.STAT_NAMES) + " N negative_cells"
    G.start_file(path)                                    # a run from initial data starts the file afresh
    assert len(G.read_sgs(path)["step"]) == 0
    with open(path, "w") as f:
        f.write("# step time kc other\n")
    with pytest.raises(ValueError, match="this run writes"):
        G.start_file(path, append=True)
    with pytest.raises(ValueError, match="does not start with the header line"):
        G.read_sgs(path)


# ------------------------------------------------------------------------------------------------------------------ 4. the inputs keys
def test_sgs_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([TG16]).problem()
    assert off["sgs"] == dict(interval=-1, filter="gaussian", kc=[], file="sgs")
    on = Inputs([TG16], ["ns.sgs_interval=5", "ns.sgs_filter=sharp", "ns.sgs_kc=2.5 4.5", "ns.sgs_file=out/sgs"]).problem()
    assert on["sgs"] == dict(interval=5, filter="sharp", kc=[2.5, 4.5], file="out/sgs")
    assert on["params"] == off["params"] and not any("sgs" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "sgs"} == {k: v for k, v in off.items() if k != "sgs"}
    assert Inputs([LDC], ["ns.sgs_interval=-1", "ns.sgs_filter=whatever"]).problem()["sgs"]["interval"] == -1      # off: nothing is checked
    with pytest.raises(KeyError, match="ns.sgs_intervall"):
        Inputs([TG16], ["ns.sgs_intervall=5"]).problem()


def test_sgs_refusals_name_the_reason():
    from iamr_amd.inputs import Inputs
    with pytest.raises(NotImplementedError, match=r"ns.sgs_interval > 0 in a two-dimensional run"):
        Inputs([POIS2D], ["ns.sgs_interval=1", "ns.sgs_kc=2"]).problem()
    with pytest.raises(ValueError, match=r"ns.sgs_interval > 0 needs a fully periodic domain"):
        Inputs([LDC], ["ns.sgs_interval=1", "ns.sgs_kc=2"]).problem()
    with pytest.raises(ValueError, match=r"ns.sgs_interval > 0 needs extents that are powers of two in 4 .. 1024, amr.n_cell has n_y = 24"):
        Inputs([TG16], ["ns.sgs_interval=1", "ns.sgs_kc=2", "amr.n_cell=16 24 16", "amr.max_level=0"]).problem()
    with pytest.raises(ValueError, match=r"ns.sgs_filter = tophat: one of sharp \| gaussian \| box"):
        Inputs([TG16], ["ns.sgs_interval=1", "ns.sgs_kc=2", "ns.sgs_filter=tophat"]).problem()
    with pytest.raises(ValueError, match=r"ns.sgs_kc = -2: a cut-off must be positive and finite"):
        Inputs([TG16], ["ns.sgs_interval=1", "ns.sgs_kc=2.5 -2"]).problem()
    with pytest.raises(ValueError, match=r"ns.sgs_kc = 0: a cut-off must be positive"):
        Inputs([TG16], ["ns.sgs_interval=1", "ns.sgs_kc=0"]).problem()
    with pytest.raises(ValueError, match=r"needs 1 .. 8 cut-offs in ns.sgs_kc, it holds 0"):
        Inputs([TG16], ["ns.sgs_interval=1"]).problem()
    with pytest.raises(ValueError, match=r"needs 1 .. 8 cut-offs in ns.sgs_kc, it holds 9"):
        Inputs([TG16], ["ns.sgs_interval=1", "ns.sgs_kc=1 2 3 4 5 6 7 8 9"]).problem()


# ------------------------------------------------------------------------------------------------------------------ 5. the ratios
def test_derived_ratios_of_a_hand_made_vector():
    from iamr_amd import sgs as G
    #     Pi   Pi2  Pi_neg k    S2   taud2  P    P2    PiP   MM   LM     P    P2    PiP   MM   LM
    s = [2.0, 13.0, -0.5, 0.7, 9.0, 8.0,  16.0, 292.0, 50.0, 4.0, -1.0,  8.0, 100.0, 7.0, 0.0, 0.0]
    d = G.as_dict(s, (64, 16), 0.125)
    assert d["Pi"] == 2.0 and d["LM_strain"] == -1.0 and d["N"] == 64 and d["negative_cells"] == 16 and d["delta"] == 0.125 and d["fields"] is None
    assert d["backscatter_fraction"] == 0.25
    assert d["backscatter_share"] == 0.5 / 2.5
    m = d["strain"]
    assert m["Cs2_flux"] == 2.0 / 16.0 and m["Cs2_lsq"] == 1.0 / 4.0
    assert m["rho_tensor"] == 2.0 / math.sqrt(8.0 * 8.0)
    assert m["rho_flux"] == (50.0 - 32.0) / math.sqrt((13.0 - 4.0) * (292.0 - 256.0))
    g = d["gradient"]
    assert g["Cs2_flux"] == 0.25
    assert math.isnan(g["Cs2_lsq"]) and math.isnan(g["rho_tensor"])                   # <D^2 |S|^2> = 0: nan, not an exception
    assert g["rho_flux"] == (7.0 - 16.0) / math.sqrt(9.0 * 36.0)
    z = G.derived([0.0] * 16, (0, 0))
    assert all(math.isnan(v) for v in (z["backscatter_fraction"], z["backscatter_share"]))
    assert all(math.isnan(v) for mdl in G.MODELS for v in z[mdl].values())
