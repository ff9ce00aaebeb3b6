"""GPU: the a-priori LES analysis (include/iamrx.h: iamrx_mf_sgs / iamrx_ns_sgs / iamrx_amr_sgs; kernels in iamr_amd/csrc/k_sgs.hip, driver in
k_spectrum.hip) through the C-ABI against the numpy yardstick of tests/sgs_numpy.py on the same data, inside the bounds its docstring
derives.  Every ghost cell of the velocity and of the output holds NaN before a call and must hold it afterwards.  The shapes are the
smallest at which a path can go wrong: unequal extents with rows shorter than a wavefront, a non-cubic domain, two thin shapes whose
periodic wrap lies two cells from itself on two axes, one box against eight.

Ratios error / bound observed on the MI355X are kept in DESIGN.md (the section on the a-priori analysis)."""
import functools
import math
import os
import numpy as np
import pytest
import spectrum_numpy as SN
import specop_numpy as SO
import sgs_numpy as GN
from test_gpu_spectrum import make_mf, geom_of, UNIT
from test_gpu_specop import nan_mf, all_nan, ghosts_nan, valid, vector
from test_cpu_sgs import sine_field

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY = os.path.join(ROOT, "tests", "golden", "inputs.3d.decay16")
AMR16 = os.path.join(ROOT, "tests", "golden", "inputs.3d.taylorgreen_amr16")
LONG = (1.0, 1.0, 2.0)
KIND = {"identity": 0, "sharp": 1, "gaussian": 2, "box": 3}
ALL = tuple(range(10))
TAU_STATS = (0, 1, 2, 3, 5, 8, 10, 13, 15)          # the statistics that vanish with tau


@functools.lru_cache(maxsize=None)
def yardstick(n, L, kind, kc, shift=(0.0, 0.0, 0.0)):
    """computed once per case and shared, never written to"""
    return GN.analyse(vector(n) + np.array(shift), L, KIND[kind], kc)


def report(tag, got, a, names=GN.FIELD_NAMES):
    """fields (n, len(names)) and the dict of mf_sgs against the analysis a: prints and returns the worst error / bound"""
    worst = 0.0
    for q, nm in enumerate(names):
        ref = a["fields"][nm]
        err = SO.norm2(got["F"][..., q] - ref.v)
        print(f"{tag} field {nm}: ||got - yardstick|| = {err:.3e}, bound {ref.e:.3e}, ratio {err / ref.e:.4f}")
        worst = max(worst, err / ref.e)
    for q, nm in enumerate(GN.STAT_NAMES):
        err, bd = abs(got[nm] - a["stats"][q]), a["stat_bounds"][q]
        print(f"{tag} <{nm}> = {got[nm]:.9e}: |got - yardstick| = {err:.3e}, bound {bd:.3e}, ratio {err / bd:.4f}")
        worst = max(worst, err / bd)
    return worst


def call(gpu, n, L, kind, kc, fields=ALL, mgs=None, out_mgs="same", f=None):
    """mf_sgs on vector(n) (or f) with NaN ghosts -> the dict plus "F": the requested fields gathered (n, nfields); checks the ghosts"""
    vel, _ = make_mf(n, vector(n) if f is None else f, mgs)
    lay = None
    if out_mgs != "same":
        lay = gpu.Layout.single(n) if out_mgs is None else gpu.Layout.decompose(tuple(n), out_mgs)
    r = gpu.mf_sgs(geom_of(n, L), vel, kind, kc, fields, layout=lay)
    if r["fields"] is not None:
        r["F"] = valid(r["fields"], n)
        assert not np.isnan(r["F"]).any()
    assert ghosts_nan(vel, vel.layout)
    return r


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("n,L,kind,kc", [((8, 16, 32), UNIT, "sharp", 4.5), ((8, 16, 32), UNIT, "gaussian", 3.0), ((8, 16, 32), UNIT, "box", 3.0),
                                         ((16, 16, 32), LONG, "sharp", 4.5), ((16, 16, 32), LONG, "gaussian", 3.0), ((16, 16, 32), LONG, "box", 3.0),
                                         ((64, 4, 4), UNIT, "gaussian", 1.0), ((4, 4, 64), UNIT, "gaussian", 1.0)])
@pytest.mark.parametrize("mgs", [None, 8])
def test_parity(gpu, n, L, kind, kc, mgs):
    if mgs is not None and min(n) < 8:
        mgs = 4                                       # the thin shapes: boxes of 4^3
    a = yardstick(n, L, kind, kc)
    assert GN.no_tie(a), "a cell of the yardstick has |Pi| below its bound"
    r = call(gpu, n, L, kind, kc, mgs=mgs)
    worst = report(f"{n} {kind} {kc} mgs {mgs}", r, a)
    assert worst <= 1.0
    assert (r["N"], r["negative_cells"]) == a["counts"] and r["N"] == n[0] * n[1] * n[2]
    assert r["delta"] == a["delta"]


# ------------------------------------------------------------------------------------------------------------------ 2. identity
def test_identity_filter_has_no_subgrid_scales(gpu):
    n, L = (8, 16, 32), UNIT
    a = yardstick(n, L, "identity", 1.0)
    r = call(gpu, n, L, "identity", 1.0)
    for q, nm in enumerate(GN.FIELD_NAMES[:8]):                      # tau, k_sgs, Pi: zero; the bound covers either side against the exact 0
        err, bd = SO.norm2(r["F"][..., q]), a["fields"][nm].e
        print(f"identity field {nm}: ||got|| = {err:.3e}, bound {bd:.3e}, ratio {err / bd:.4f}")
        assert err <= bd
    for q in TAU_STATS:
        nm = GN.STAT_NAMES[q]
        print(f"identity <{nm}> = {r[nm]:.3e}, bound {a['stat_bounds'][q]:.3e}")
        assert abs(r[nm]) <= a["stat_bounds"][q]
    for q in set(range(16)) - set(TAU_STATS):                        # the strain and the model fluxes are those of the field itself
        nm = GN.STAT_NAMES[q]
        assert abs(r[nm] - a["stats"][q]) <= a["stat_bounds"][q] and r[nm] > 0.0
    for q in (8, 9):
        ref = a["fields"][GN.FIELD_NAMES[q]]
        assert SO.norm2(r["F"][..., q] - ref.v) <= ref.e


# ------------------------------------------------------------------------------------------------------------------ 3. spectrum
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), LONG)])
def test_subgrid_energy_is_the_tail_of_the_spectrum(gpu, n, L):
    """sharp cut at 4.5: <k_sgs> = sum over the shells s >= 5 of E(s) = (P_u + P_v + P_w) / 2 of mf_spectrum of the same array"""
    a = yardstick(n, L, "sharp", 4.5)
    vel, _ = make_mf(n, vector(n))
    g = geom_of(n, L)
    r = gpu.mf_sgs(g, vel, "sharp", 4.5)
    P, _ = gpu.mf_spectrum(g, vel, 0, 3)
    tail = 0.5 * math.fsum(P[:, 5:].ravel())
    tol = a["stat_bounds"][3]
    for c in range(3):
        Pr, count = SN.spectrum_reference(vector(n)[..., c], L)
        tol += 0.5 * math.fsum(SN.bound(Pr, count, vector(n)[..., c].size)[5:])
    print(f"{n}: <k_sgs> = {r['k_sgs']:.12e}, spectrum tail {tail:.12e}, difference {abs(r['k_sgs'] - tail):.3e}, tolerance {tol:.3e}")
    assert r["fields"] is None and abs(r["k_sgs"] - tail) <= tol


# ------------------------------------------------------------------------------------------------------------------ 4. closed form
def test_closed_forms_of_a_sine_mode(gpu):
    """the cases of tests/test_cpu_sgs.py on the device, within its 1e-14"""
    n, A = (8, 16, 8), 1.5
    f, theta = sine_field(n, A)
    r = call(gpu, n, UNIT, "sharp", 2.5, f=f)
    worst = float(np.max(np.abs(r["F"][..., 0] - (0.5 * A * A * np.cos(2.0 * theta))[None, :, None])))
    r = call(gpu, n, UNIT, "sharp", 4.5, f=f)
    worst = max(worst, float(np.max(np.abs(r["F"][..., :7]))))
    r = call(gpu, n, UNIT, "sharp", 1.5, f=f)
    worst = max(worst, float(np.max(np.abs(r["F"][..., 0] - 0.5 * A * A))), abs(r["k_sgs"] - 0.25 * A * A), float(np.max(np.abs(r["F"][..., 8]))))
    print(f"sine mode on the device: worst deviation from the closed forms {worst:.3e}")
    assert worst <= 1e-14


# ------------------------------------------------------------------------------------------------------------------ 5. Galilean
@pytest.mark.parametrize("n,L", [((8, 16, 32), UNIT), ((16, 16, 32), LONG)])
def test_galilean_invariance(gpu, n, L):
    """tau and Pi of u + (10, -7, 3) are those of u: G(0) = 1 and the filter is linear.  Tolerance: the two calls' bounds added."""
    shift = (10.0, -7.0, 3.0)
    a0, a1 = yardstick(n, L, "gaussian", 3.0), yardstick(n, L, "gaussian", 3.0, shift)
    r0 = call(gpu, n, L, "gaussian", 3.0, fields=range(8))
    r1 = call(gpu, n, L, "gaussian", 3.0, fields=range(8), f=vector(n) + np.array(shift))
    for q, nm in enumerate(GN.FIELD_NAMES[:8]):
        err, bd = SO.norm2(r1["F"][..., q] - r0["F"][..., q]), a0["fields"][nm].e + a1["fields"][nm].e
        print(f"{n} Galilean {nm}: ||shifted - plain|| = {err:.3e} (max {float(np.max(np.abs(r1['F'][..., q] - r0['F'][..., q]))):.3e}), tolerance {bd:.3e}, ratio {err / bd:.4f}")
        assert err <= bd
    for q in (0, 3):
        nm = GN.STAT_NAMES[q]
        assert abs(r1[nm] - r0[nm]) <= a0["stat_bounds"][q] + a1["stat_bounds"][q]


# ------------------------------------------------------------------------------------------------------------------ 6. bits, layouts
def test_bits_and_layouts(gpu):
    n, L = (8, 16, 32), UNIT
    r1 = call(gpu, n, L, "gaussian", 3.0)
    again = call(gpu, n, L, "gaussian", 3.0)
    assert again["F"].tobytes() == r1["F"].tobytes() and again["stats"].tobytes() == r1["stats"].tobytes()        # the same call twice
    r8 = call(gpu, n, L, "gaussian", 3.0, mgs=8)
    assert len(r8["fields"].layout.boxes) == 8
    assert r8["F"].tobytes() == r1["F"].tobytes() and r8["stats"].tobytes() == r1["stats"].tobytes()              # one box against eight
    assert (r8["N"], r8["negative_cells"]) == (r1["N"], r1["negative_cells"])
    so = call(gpu, n, L, "gaussian", 3.0, fields=())
    assert so["fields"] is None and so["stats"].tobytes() == r1["stats"].tobytes() and so["negative_cells"] == r1["negative_cells"]
    pick = ["sgs_flux", 2, "k_sgs", 9, 0]
    sub = call(gpu, n, L, "gaussian", 3.0, fields=pick, mgs=8)
    assert sub["F"].shape[3] == 5 and sub["stats"].tobytes() == r1["stats"].tobytes()
    assert sub["F"].tobytes() == np.ascontiguousarray(r1["F"][..., [7, 2, 6, 9, 0]]).tobytes()                    # a shuffled subset
    x = call(gpu, n, L, "gaussian", 3.0, mgs=8, out_mgs=None)                                                      # eight boxes into one
    y = call(gpu, n, L, "gaussian", 3.0, mgs=None, out_mgs=8)                                                      # one box into eight
    assert len(x["fields"].layout.boxes) == 1 and len(y["fields"].layout.boxes) == 8
    assert x["F"].tobytes() == r1["F"].tobytes() and y["F"].tobytes() == r1["F"].tobytes()


def test_output_ghosts_and_neighbour_components_stay(gpu):
    """fields into components 1 .. 2 of a NaN array of four with a ghost layer, straight through the C entry: nothing else is written"""
    import ctypes as C
    from test_gpu_specop import ghosts_nan_comp
    n = (8, 16, 32)
    vel, _ = make_mf(n, vector(n), 8)
    out, lay = nan_mf(n, 4, 8)
    g = geom_of(n)
    stats, counts, which = np.zeros(16), (C.c_long * 2)(), (C.c_int * 2)(7, 6)
    rc = gpu.lib().iamrx_mf_sgs(C.byref(g), vel.h, 0, 2, C.c_double(3.0), out.h, 1, 2, which, stats.ctypes.data_as(C.POINTER(C.c_double)), counts)
    assert rc == 0 and ghosts_nan_comp(out, lay, 1, 2)
    ref = call(gpu, n, UNIT, "gaussian", 3.0, fields=(7, 6))
    assert valid(out, n)[..., 1:3].tobytes() == ref["F"].tobytes() and stats.tobytes() == ref["stats"].tobytes()
    assert list(counts) == [ref["N"], ref["negative_cells"]]
    rc = gpu.lib().iamrx_mf_sgs(C.byref(g), vel.h, 0, 2, C.c_double(3.0), None, 0, 0, None, stats.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == 0 and stats.tobytes() == ref["stats"].tobytes()                                                   # counts may be null


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_errors_leave_out_untouched(gpu):
    import ctypes as C
    from iamr_amd.lib import IamrxError, check
    n = (8, 16, 32)
    vel, lay = make_mf(n, vector(n))
    out, _ = nan_mf(n, 10)
    g = geom_of(n)
    stats, counts = np.zeros(16), (C.c_long * 2)()
    sp = stats.ctypes.data_as(C.POINTER(C.c_double))

    def raw(gm=g, v=vel, vcomp=0, kind=2, kc=3.0, o=out, ocomp=0, which=(0,), nout=None, st=sp, wnull=False):
        w = (C.c_int * max(len(which), 1))(*which)
        check(gpu.lib().iamrx_mf_sgs(C.byref(gm), v.h, vcomp, kind, C.c_double(kc), o.h if o is not None else None, ocomp,
                                     len(which) if nout is None else nout, None if wnull else w, st, counts))

    raw()                                                             # the defaults are a good call ...
    assert not all_nan(out)
    out, _ = nan_mf(n, 10)                                            # ... and from here on nothing may be written
    nodal = gpu.MultiFab(gpu.Layout.single(n), gpu.NODE, 3, 1)
    for kw in (dict(v=nodal), dict(o=nodal)):
        with pytest.raises(IamrxError, match="cell-centred"):
            raw(**kw)
    for kw in (dict(vcomp=1), dict(vcomp=-1), dict(ocomp=10), dict(ocomp=8, which=(0, 1, 2))):
        with pytest.raises(IamrxError, match="component"):
            raw(**kw)
    with pytest.raises(IamrxError, match="cover"):
        raw(gm=geom_of((8, 16, 64)))
    half, _ = nan_mf((8, 16, 16), 10)
    with pytest.raises(IamrxError, match="cover"):
        raw(o=half)
    assert all_nan(half)
    with pytest.raises(IamrxError, match="periodic"):
        raw(gm=geom_of(n, periodic=(1, 0, 1)))
    m12 = (12, 16, 16)
    v12, _ = make_mf(m12, SN.noise(m12, 1, 3))
    o12, _ = nan_mf(m12, 10)
    with pytest.raises(IamrxError, match=r"n_x = 12"):
        raw(gm=geom_of(m12), v=v12, o=o12)
    assert all_nan(o12)
    for kind in (-1, 4):
        with pytest.raises(IamrxError, match="kind"):
            raw(kind=kind)
    for kc in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(IamrxError, match="kc"):
            raw(kc=kc)
    for which in ((10,), (-1,), (0, 3, 11)):
        with pytest.raises(IamrxError, match=r"field id -?\d+ outside 0 .. 9"):
            raw(which=which)
    with pytest.raises(IamrxError, match="null out or which"):
        raw(o=None)
    with pytest.raises(IamrxError, match="null out or which"):
        raw(wnull=True)
    with pytest.raises(IamrxError, match="out aliases vel"):
        raw(o=vel)
    with pytest.raises(IamrxError, match="null stats"):
        raw(st=None)
    with pytest.raises(ValueError, match="tau_zx"):
        gpu.mf_sgs(g, vel, "gaussian", 3.0, ["tau_zx"])
    with pytest.raises(ValueError, match="tophat"):
        gpu.mf_sgs(g, vel, "tophat", 3.0)
    assert all_nan(out)
    assert valid(vel, n).tobytes() == np.ascontiguousarray(vector(n)).tobytes() and ghosts_nan(vel, lay)


# ------------------------------------------------------------------------------------------------------------------ 8. level entries
def same(a, b, n):
    return (a["stats"].tobytes() == b["stats"].tobytes() and (a["N"], a["negative_cells"]) == (b["N"], b["negative_cells"])
            and valid(a["fields"], n).tobytes() == valid(b["fields"], n).tobytes())


def test_level_and_hierarchy(gpu):
    """NavierStokes.sgs on the 16^3 state of inputs.3d.decay16 is mf_sgs of its velocity to the bit; Amr.sgs is level 0's"""
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    n = (16, 16, 16)
    ns, lay, g, pr = R.build(Inputs([DECAY], ["amr.plot_int=-1", "amr.check_int=-1", "ns.spectrum_interval=-1"]), gpu, N)
    ns.post_init(pr["stop_time"])
    a = ns.sgs("gaussian", 3.0, ("sgs_flux", "tau_xy"))
    b = gpu.mf_sgs(ns.geom, ns.data(ns.S_NEW), "gaussian", 3.0, ("sgs_flux", "tau_xy"), vcomp=0)
    assert same(a, b, n) and a["k_sgs"] > 0.0 and 0 < a["negative_cells"] < a["N"] == 4096
    assert a["strain"]["Cs2_flux"] == a["Pi"] / a["P_strain"] and a["backscatter_fraction"] == a["negative_cells"] / 4096
    pra = Inputs([AMR16]).problem()
    amr, lays, g0 = R.build_amr(pra, gpu, N)
    amr.post_init(pra["stop_time"])
    amr.coarse_step()
    assert amr.nlev > 1
    c = amr.sgs("sharp", 2.5, (6, 7))
    d = gpu.mf_sgs(amr.geom0, amr.levels[0].data(amr.levels[0].S_NEW), "sharp", 2.5, (6, 7))
    assert same(c, d, n) and same(c, amr.levels[0].sgs("sharp", 2.5, (6, 7)), n)


def test_driver_writes_the_time_series(gpu, tmp_path, monkeypatch):
    """python -m iamr_amd.run tests/golden/inputs.3d.decay16 max_step=2 ns.sgs_interval=1 ns.sgs_kc="2.5 4.5", in this process: one row
    per output and cut-off; every row has the bits of a direct call at that moment; without the key no file appears"""
    from iamr_amd import run as R
    from iamr_amd.sgs import read_sgs
    monkeypatch.chdir(tmp_path)
    seen = {}

    def observe(ns, step, dt):
        seen[step] = [ns.sgs("gaussian", kc) for kc in (2.5, 4.5)]

    quiet = ["max_step=2", "amr.plot_int=-1", "amr.check_int=-1", "ns.spectrum_interval=-1"]
    assert R.main([DECAY] + quiet + ["ns.sgs_interval=1", "ns.sgs_kc=2.5 4.5"], observe) == 0
    assert sorted(os.listdir(tmp_path)) == ["sgs"]
    t = read_sgs(str(tmp_path / "sgs"))
    outputs = sorted(seen)
    assert len(outputs) >= 2 and outputs[-1] == 2
    assert t["step"].tolist() == [s for s in outputs for _ in range(2)] and t["kc"].tolist() == [2.5, 4.5] * len(outputs)
    for row, (s, q) in enumerate((s, q) for s in outputs for q in range(2)):
        assert t["stats"][row].tobytes() == seen[s][q]["stats"].tobytes(), (s, q)
        assert (int(t["N"][row]), int(t["negative_cells"][row])) == (seen[s][q]["N"], seen[s][q]["negative_cells"])
    assert np.all(t["k_sgs"][0::2] > t["k_sgs"][1::2]) and np.all(t["k_sgs"] > 0.0)      # a lower cut-off leaves more below the grid
    os.remove(tmp_path / "sgs")
    assert R.main([DECAY] + quiet) == 0 and os.listdir(tmp_path) == []
