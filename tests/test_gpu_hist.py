"""GPU: histograms and PDFs (include/iamrx.h: iamrx_mf_histogram / iamrx_ns_histogram / iamrx_amr_histogram and the joint forms; kernel in
iamr_amd/csrc/k_hist.hip) through the C-ABI against the numpy restatement of tests/hist_numpy.py on the same data.

The counts are integers: every comparison is exact equality, there are no tolerances.  The shapes are the smallest at which each path of
the kernel can go wrong: unequal extents, a row that is no multiple of a wavefront and a row shorter than one, a z extent that is no
multiple of the march, several unequal boxes, more tiles than one, column groups, two and three levels.  All ghost cells hold NaN: a
ghost cell that is read shows in the slot `nan`."""
import os
import numpy as np
import pytest
import hist_numpy as HN
from test_gpu_profile import random_state, put_state, one_level

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
REGRID16 = os.path.join(GOLD, "inputs.3d.tracer_regrid16")
POIS2D = os.path.join(GOLD, "regtest.2d.poiseuille")
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]
NAMES5 = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer"]
# random_state: uniform in mean +- 1; the ranges cut into the data on one side or the other, so that below and above are exercised
RANGES5 = [(-0.5, 1.0), (-1.2, 0.8), (-0.9, 1.1), (0.75, 2.0), (-0.5, 1.6)]


def slots(h):
    """the dict of pdf.as_dict -> the library's (n, nbins + 3) counts"""
    return np.concatenate([h["counts"], h["below"][:, None], h["above"][:, None], h["nan"][:, None]], axis=1)


def reference_one_level(S, boxes, ranges, nbins):
    return HN.hist_reference([S], [boxes], list(S.shape[:3]), [r[0] for r in ranges], [r[1] for r in ranges], nbins)


def put_mf(lay, A, ng=1):
    """a cell MultiFab := A (n, ncomp) on the valid cells of every box, NaN in all ghost cells"""
    from iamr_amd import lib as L
    mf = L.MultiFab(lay, L.CELL, A.shape[-1], ng)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (A.shape[-1],), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = A[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    return mf


# ------------------------------------------------------------------------------------------------------------------ 1. one box
@pytest.mark.parametrize("n", [(20, 12, 6), (4, 8, 8)])
@pytest.mark.parametrize("nbins", [7, 64])
def test_one_box(gpu, n, nbins):
    """unequal extents (an axis mix-up shows), nx neither a multiple nor a divisor of 64, nz no multiple of the march; then a row
    shorter than a wavefront.  Five columns in one pass."""
    S = random_state(n, 5)
    ns, lay = one_level(n, S)
    h = ns.histogram(NAMES5, nbins, RANGES5)
    ref = reference_one_level(S, lay.boxes, RANGES5, nbins)
    assert h["counts"].dtype == np.int64 and np.array_equal(slots(h), ref)
    assert not h["nan"].any()                                                         # no ghost cell was read
    assert h["below"].sum() > 0 and h["above"].sum() > 0                              # (the ranges do cut into the data)
    assert np.array_equal(h["total"], np.full(5, n[0] * n[1] * n[2]))
    for q in range(5):
        assert np.array_equal(h["edges"][q], RANGES5[q][0] + (RANGES5[q][1] - RANGES5[q][0]) * np.arange(nbins + 1) / nbins)
        assert np.array_equal(h["pdf"][q], h["counts"][q] / (h["counts"][q].sum() * ((RANGES5[q][1] - RANGES5[q][0]) / nbins)))
    again = ns.histogram(NAMES5, nbins, RANGES5)
    assert slots(again).tobytes() == slots(h).tobytes()                               # the same bits on every call


# ------------------------------------------------------------------------------------------------------------------ 2. edge values
def test_edge_values(gpu):
    """lo = 0, hi = 1, nbins = 8 (exact edges): lo, hi, their neighbours outward and inward, every interior edge and the double below
    it, -0.0, the infinities and a NaN, each in one cell of u; the other cells hold 0.5"""
    n = (4, 8, 8)
    special = [0.0, 1.0, np.nextafter(0.0, -np.inf), np.nextafter(1.0, np.inf), np.nextafter(0.0, np.inf), np.nextafter(1.0, -np.inf)]
    special += [k / 8 for k in range(1, 8)] + [np.nextafter(k / 8, -np.inf) for k in range(1, 8)]
    special += [-0.0, np.inf, -np.inf, np.nan]
    S = np.full(n + (5,), 0.5)
    rng = np.random.default_rng(8)
    at = rng.permutation(n[0] * n[1] * n[2])[:len(special)]
    S[..., 0].flat[at] = special
    ns, lay = one_level(n, S)
    h = ns.histogram("x_velocity", 8, (0.0, 1.0))
    ref = HN.hist1(S[..., 0], 0.0, 1.0, 8)
    assert np.array_equal(slots(h)[0], ref)
    # ... and written out: what the rule says about each of them
    want = np.zeros(11, dtype=np.int64)
    want[0] += 3                                      # lo, its inward neighbour, -0.0
    want[7] += 2                                      # hi (the last bin), its inward neighbour
    for k in range(1, 8):
        want[k] += 1                                  # an interior edge lies in the upper bin
        want[k - 1] += 1                              # the double below it in the lower one
    want[4] += n[0] * n[1] * n[2] - len(special)      # the cells that hold 0.5
    want[8], want[9], want[10] = 2, 2, 1              # below: nextafter(lo), -inf; above: nextafter(hi), +inf; nan
    assert np.array_equal(slots(h)[0], want)


# ------------------------------------------------------------------------------------------------------------------ 3. constant field
def test_constant_field(gpu):
    """16^3 cells in one bin: every lane of every wavefront holds the same counter (the aggregation path)"""
    n = (16, 16, 16)
    S = np.zeros(n + (5,))
    S[..., 3] = 1.25
    ns, lay = one_level(n, S)
    h = ns.histogram(["density", "x_velocity"], 16, [(1.0, 2.0), (0.0, 1.0)])
    want = np.zeros((2, 19), dtype=np.int64)
    want[0, 4] = want[1, 0] = 4096
    assert np.array_equal(slots(h), want)


# ------------------------------------------------------------------------------------------------------------------ 4. box independence
def test_box_independence(gpu):
    """(20, 12, 6) cut at max_grid_size 8 into several unequal boxes: the same counts as the single box, to the bit"""
    n = (20, 12, 6)
    S = random_state(n, 12)
    many, lay = one_level(n, S, 8)
    assert len(lay.boxes) >= 4 and len({tuple(hi[d] - lo[d] + 1 for d in range(3)) for lo, hi in lay.boxes}) > 1
    one, lay1 = one_level(n, S)
    a, b = many.histogram(NAMES5, 33, RANGES5), one.histogram(NAMES5, 33, RANGES5)
    assert np.array_equal(slots(a), reference_one_level(S, lay.boxes, RANGES5, 33))
    assert slots(a).tobytes() == slots(b).tobytes()
    assert not a["nan"].any()


# ------------------------------------------------------------------------------------------------------------------ 5. bin limits
def test_bin_limits(gpu):
    """nbins = 1; nbins = 4096 with 8 columns on 16^3: three columns' counters fill the LDS, the columns go in three groups"""
    from iamr_amd import lib as L
    n = (16, 16, 16)
    rng = np.random.default_rng(21)
    A = rng.uniform(-1.0, 1.0, size=n + (8,)) * np.arange(1, 9)
    lay = L.Layout.single(n)
    mf = put_mf(lay, A)
    ranges = [(-0.75 * (q + 1), 0.9 * (q + 1)) for q in range(8)]
    for nbins in (1, 4096):
        got = L.mf_histogram(mf, 0, 8, nbins, ranges)
        assert got.dtype == np.int64 and got.shape == (8, nbins + 3)
        assert np.array_equal(got, reference_one_level(A, lay.boxes, ranges, nbins))
        assert not got[:, nbins + 2].any() and np.array_equal(got.sum(axis=1), np.full(8, 4096))
    # a sub-range of the components, a weight, one range for all columns
    got = L.mf_histogram(mf, 2, 3, 4096, (-1.0, 1.0), weight=64)
    assert np.array_equal(got, 64 * reference_one_level(A[..., 2:5], lay.boxes, [(-1.0, 1.0)] * 3, 4096))
    # a coverage array: the cells with cov != 0 are skipped, whatever they hold
    cov = np.zeros(n + (1,))
    cov[3:9, :, 5:7] = 1.0
    B = A.copy()
    B[cov[..., 0] != 0.0] = np.nan
    got = L.mf_histogram(put_mf(lay, B), 0, 8, 64, ranges, cov=put_mf(lay, cov, 0))
    want = np.stack([HN.hist1(A[..., q][cov[..., 0] == 0.0], ranges[q][0], ranges[q][1], 64) for q in range(8)])
    assert np.array_equal(got, want) and not got[:, 66].any()


# ------------------------------------------------------------------------------------------------------------------ 6. hierarchy
def _hierarchy_check(amr, seed):
    """random data on every level, NaN under the finer levels: composite counts, nothing in `nan`, the total"""
    assert amr.nlev >= 2
    n0 = list(amr.geom0.n)
    F = amr.nlev - 1
    boxes = [amr.layouts[l].boxes for l in range(amr.nlev)]
    counted = HN.counted_masks(boxes, n0)
    states = []
    for l in range(amr.nlev):
        S = random_state([v << l for v in n0], seed + l)
        S[HN.box_mask(boxes[l], S.shape[:3]) & ~counted[l]] = np.nan                   # what a finer level covers must reach no slot
        states.append(S)
        put_state(amr.levels[l], amr.layouts[l], S)
    for nbins in (7, 64):
        h = amr.histogram(NAMES5, nbins, RANGES5)
        ref = HN.hist_reference(states, boxes, n0, [r[0] for r in RANGES5], [r[1] for r in RANGES5], nbins)
        assert np.array_equal(slots(h), ref), nbins
        assert not h["nan"].any()
        assert np.array_equal(h["total"], np.full(5, n0[0] * n0[1] * n0[2] * 8 ** F))
    c2, o2 = HN.hist2_reference([S[..., 0] for S in states], [S[..., 3] for S in states], boxes, n0, (RANGES5[0][0], RANGES5[3][0]),
                                (RANGES5[0][1], RANGES5[3][1]), (5, 9))
    h2 = amr.histogram2("x_velocity", "density", (5, 9), (RANGES5[0], RANGES5[3]))
    assert np.array_equal(h2["counts"], c2) and h2["outside"] == o2 and h2["total"] == n0[0] * n0[1] * n0[2] * 8 ** F
    return F


@pytest.mark.parametrize("inputs,seed", [(AMR16, 20), (REGRID16, 30)], ids=["taylorgreen_amr16", "tracer_regrid16"])
def test_hierarchy(gpu, inputs, seed):
    """the fixed grids of inputs.3d.taylorgreen_amr16 and the boxes inputs.3d.tracer_regrid16 tags for its initial data"""
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    amr, lays, g0 = R.build_amr(Inputs([inputs]).problem(), L, N)
    print(f"{os.path.basename(inputs)}: {amr.nlev} levels, boxes per level {[len(l.boxes) for l in amr.layouts]}")
    assert _hierarchy_check(amr, seed) == 2                                            # three levels


# ------------------------------------------------------------------------------------------------------------------ 7. derived names
def _level_field(level, n, name):
    return level.derive(name).gather_valid(n)[..., 0]


def test_derived_names(gpu):
    """mag_vort and energy: the yardstick applied to what derive(name) returns, on one level (several boxes) and on the hierarchy"""
    n = (20, 12, 6)
    ns, lay = one_level(n, random_state(n, 3), 8)
    names = ["mag_vort", "x_velocity", "energy"]
    cols = np.stack([_level_field(ns, n, "mag_vort"), ns.data(ns.S_NEW).gather_valid(n)[..., 0], _level_field(ns, n, "energy")], axis=-1)
    assert np.isfinite(cols).all() and cols[..., 0].max() > 0.0
    ranges = [(0.0, 0.6 * cols[..., 0].max()), (-0.5, 1.0), (0.1, 0.5 * cols[..., 2].max())]
    h = ns.histogram(names, 24, ranges)
    assert np.array_equal(slots(h), reference_one_level(cols, lay.boxes, ranges, 24))
    h2 = ns.histogram2("energy", "mag_vort", (6, 11), (ranges[2], ranges[0]))
    c2, o2 = HN.hist2(cols[..., 2], cols[..., 0], (ranges[2][0], ranges[0][0]), (ranges[2][1], ranges[0][1]), (6, 11))
    assert np.array_equal(h2["counts"], c2) and h2["outside"] == o2 and o2 > 0
    # the hierarchy: initial TaylorGreen data, automatic range
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    amr, lays, g0 = R.build_amr(Inputs([AMR16]).problem(), L, N)
    amr.post_init(-1.0)
    n0 = list(amr.geom0.n)
    boxes = [amr.layouts[l].boxes for l in range(amr.nlev)]
    f = [np.stack([_level_field(amr.levels[l], [v << l for v in n0], nm) for nm in ("mag_vort", "energy")], axis=-1) for l in range(amr.nlev)]
    h = amr.histogram(["mag_vort", "energy"], 32)
    valid = [f[l][HN.box_mask(boxes[l], f[l].shape[:3])] for l in range(amr.nlev)]
    for q in range(2):
        assert h["range"][q][0] == min(v[:, q].min() for v in valid) and h["range"][q][1] == max(v[:, q].max() for v in valid)
    assert np.array_equal(slots(h), HN.hist_reference(f, boxes, n0, h["range"][:, 0], h["range"][:, 1], 32))
    assert not h["below"].any() and not h["above"].any() and not h["nan"].any()


# ------------------------------------------------------------------------------------------------------------------ 8. joint histogram
def test_joint_histogram(gpu):
    n = (20, 12, 6)
    S = random_state(n, 14)
    ns, lay = one_level(n, S)
    # nothing outside: the marginals are the one-dimensional histograms
    rx, ry = (-0.75, 1.35), (0.45, 2.55)
    h2 = ns.histogram2("x_velocity", "density", (5, 9), (rx, ry))
    c, o = HN.hist2(S[..., 0], S[..., 3], (rx[0], ry[0]), (rx[1], ry[1]), (5, 9))
    assert h2["counts"].dtype == np.int64 and np.array_equal(h2["counts"], c) and h2["outside"] == o == 0
    assert h2["total"] == n[0] * n[1] * n[2]
    assert np.array_equal(h2["counts"].sum(axis=1), ns.histogram("x_velocity", 5, rx)["counts"][0])
    assert np.array_equal(h2["counts"].sum(axis=0), ns.histogram("density", 9, ry)["counts"][0])
    assert np.array_equal(h2["xedges"], rx[0] + (rx[1] - rx[0]) * np.arange(6) / 5) and np.array_equal(h2["yedges"], ry[0] + (ry[1] - ry[0]) * np.arange(10) / 9)
    # one value outside on one axis lands in `outside`
    S2 = S.copy()
    S2[7, 5, 3, 3] = 2.6
    put_state(ns, lay, S2)
    h3 = ns.histogram2("x_velocity", "density", (5, 9), (rx, ry))
    c3, o3 = HN.hist2(S2[..., 0], S2[..., 3], (rx[0], ry[0]), (rx[1], ry[1]), (5, 9))
    assert h3["outside"] == o3 == 1 and np.array_equal(h3["counts"], c3) and h3["counts"].sum() == c.sum() - 1
    # ranges that cut into both axes, the largest joint histogram (128 x 128 = 16384 slots), several boxes
    many, lay8 = one_level(n, S, 8)
    h4 = many.histogram2("z_velocity", "density", (128, 128), (RANGES5[2], RANGES5[3]))
    c4, o4 = HN.hist2(S[..., 2], S[..., 3], (RANGES5[2][0], RANGES5[3][0]), (RANGES5[2][1], RANGES5[3][1]), (128, 128))
    assert np.array_equal(h4["counts"], c4) and h4["outside"] == o4 > 0


# ------------------------------------------------------------------------------------------------------------------ 9. automatic range
def test_automatic_range(gpu):
    n = (20, 12, 6)
    S = random_state(n, 17)
    S[..., 4] = 0.375                                                                  # a constant tracer
    ns, lay = one_level(n, S, 8)
    h = ns.histogram(NAMES5, 16)
    for q in range(4):
        assert h["range"][q][0] == S[..., q].min() and h["range"][q][1] == S[..., q].max()
        assert h["counts"][q][15] >= 1 and h["counts"][q][0] >= 1                      # the maximum sits in the last bin
    assert not h["below"].any() and not h["above"].any() and not h["nan"].any()
    assert tuple(h["range"][4]) == (0.375 - 0.5, 0.375 + 0.5)                          # numpy's rule for lo == hi
    assert h["counts"][4][8] == n[0] * n[1] * n[2]
    assert np.array_equal(slots(h), reference_one_level(S, lay.boxes, [tuple(r) for r in h["range"]], 16))


# ------------------------------------------------------------------------------------------------------------------ 10. errors
def test_errors(gpu):
    from iamr_amd import lib as L
    from iamr_amd.lib import IamrxError
    n = (4, 8, 8)
    ns, lay = one_level(n, random_state(n, 1))
    for kw in (dict(range=(1.0, 1.0)), dict(range=(1.0, 0.5)), dict(range=(np.nan, 1.0)), dict(range=(0.0, np.inf)), dict(nbins=0, range=(0.0, 1.0)),
               dict(nbins=4097, range=(0.0, 1.0))):
        with pytest.raises(IamrxError):
            ns.histogram("x_velocity", **kw)
    with pytest.raises(IamrxError, match="mag_vort"):                                  # the message lists the known names
        ns.histogram(["x_velocity", "vorticity"], 8, [(0.0, 1.0), (0.0, 1.0)])
    with pytest.raises(IamrxError):
        ns.histogram("tracer2", 8, (0.0, 1.0))                                         # the run has no second tracer
    with pytest.raises(IamrxError):
        ns.histogram2("x_velocity", "density", (129, 128), ((0.0, 1.0), (0.0, 1.0)))
    with pytest.raises(IamrxError):
        ns.histogram2("x_velocity", "nothing", (4, 4), ((0.0, 1.0), (0.0, 1.0)))
    mf = put_mf(lay, random_state(n, 2))
    other = L.Layout.decompose(n, 4)
    with pytest.raises(IamrxError, match="layout"):                                    # a coverage array on another layout
        L.mf_histogram(mf, 0, 1, 8, (0.0, 1.0), cov=L.MultiFab(other, L.CELL, 1, 0))
    with pytest.raises(IamrxError):
        L.mf_histogram(mf, 3, 3, 8, (0.0, 1.0))                                        # components 3 .. 5 of 5
    assert np.array_equal(L.mf_histogram(mf, 0, 1, 8, (0.0, 1.0)).sum(axis=1), [256])  # ... and the level still works


# ------------------------------------------------------------------------------------------------------------------ 11. driver
def test_driver_writes_the_files(gpu, tmp_path, monkeypatch):
    """inputs.3d.taylorgreen_amr16, two steps with ns.pdf_interval = 1: pdf00000 .. pdf00002 appear in the working directory, the last
    equals Amr.histogram of the final state bit for bit; without the keys no file appears"""
    from iamr_amd import run as R
    from iamr_amd.pdf import read_pdf
    names = ["x_velocity", "mag_vort"]
    seen = {}

    def observe(amr, step, dt):
        if step == 2:
            seen[step] = (amr.time, amr.histogram(names, 64))

    d1 = tmp_path / "on"; d1.mkdir(exist_ok=True)          # (the test may run once per box mode)
    monkeypatch.chdir(d1)
    assert R.main([AMR16, "max_step=2", "ns.pdf_interval=1", 'ns.pdf_vars="x_velocity mag_vort"'] + QUIET, observe) == 0
    assert sorted(os.listdir(d1)) == ["pdf00000", "pdf00001", "pdf00002"]
    time, h = seen[2]
    r = read_pdf(str(d1 / "pdf00002"))
    assert (r["step"], r["time"], r["names"], r["nbins"]) == (2, time, tuple(names), 64)
    for k in ("range", "edges", "counts", "below", "above", "nan", "total", "pdf"):
        assert r[k].dtype == h[k].dtype and r[k].tobytes() == h[k].tobytes(), k
    assert not r["below"].any() and not r["above"].any() and not r["nan"].any() and r["total"][0] == r["total"][1] > 0
    d2 = tmp_path / "off"; d2.mkdir(exist_ok=True)
    monkeypatch.chdir(d2)
    assert R.main([AMR16, "max_step=1"] + QUIET) == 0
    assert os.listdir(d2) == []


def test_driver_two_dimensional(gpu, tmp_path, monkeypatch):
    """a 2-D regtest fixture with the keys: the file's slots sum to the slab's cell total (in finest-level cells)"""
    from iamr_amd import run as R
    from iamr_amd.pdf import read_pdf
    seen = {}

    def observe(run, step, dt):
        g = getattr(run, "geom0", None) or run.geom
        seen[step] = int(np.prod(g.n)) * 8 ** (run.nlev - 1)

    monkeypatch.chdir(tmp_path)
    assert R.main([POIS2D, "max_step=1", "ns.pdf_interval=1", "ns.pdf_vars=x_velocity y_velocity", "ns.pdf_nbins=16"] + QUIET, observe) == 0
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("pdf")) == ["pdf00000", "pdf00001"]
    for step in (0, 1):
        r = read_pdf(str(tmp_path / f"pdf{step:05d}"))
        assert r["names"] == ("x_velocity", "y_velocity") and r["nbins"] == 16
        assert np.array_equal(r["total"], [seen[step]] * 2) and not r["nan"].any()
