"""CPU suite: histograms and PDFs (iamr_amd/pdf.py, the ns.pdf_* keys of iamr_amd/inputs.py, the entries of include/iamrx.h) --
everything about them that needs no device.  The numpy restatement the GPU tests compare with (tests/hist_numpy.py) is itself
checked here against np.histogram / np.histogram2d where the two rules cannot differ, and on the edge cases of the binning rule."""
import os
import re
import numpy as np
import pytest
import hist_numpy as HN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LDC = os.path.join(HERE, "golden", "inputs.3d.lid_driven_cavity16")
POIS2D = os.path.join(HERE, "golden", "regtest.2d.poiseuille")


# ------------------------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("lo,hi,nbins", [(0.0, 1.0, 8), (-0.3, 1.1, 7), (2.5, 1000.0, 64), (-1.0e-3, 1.0e-3, 1)])
def test_restatement_equals_numpy_at_bin_centres(lo, hi, nbins):
    """values at the bin centres, a random number of times each: no rule can put a centre into another bin"""
    rng = np.random.default_rng(nbins)
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    centres = 0.5 * (edges[:-1] + edges[1:])
    v = rng.permutation(np.repeat(centres, rng.integers(0, 9, size=nbins)))
    got = HN.hist1(v, lo, hi, nbins)
    want, _ = np.histogram(v, bins=nbins, range=(lo, hi))
    assert got.dtype == np.int64 and np.array_equal(got[:nbins], want) and not got[nbins:].any()
    assert np.array_equal(HN.hist1(v, lo, hi, nbins, weight=64), 64 * got)


def test_restatement_equals_numpy_2d_at_bin_centres():
    rng = np.random.default_rng(2)
    lo, hi, nb = (-1.0, 0.5), (2.0, 0.75), (5, 9)
    cx = lo[0] + (hi[0] - lo[0]) * (np.arange(nb[0]) + 0.5) / nb[0]
    cy = lo[1] + (hi[1] - lo[1]) * (np.arange(nb[1]) + 0.5) / nb[1]
    x, y = cx[rng.integers(0, nb[0], size=500)], cy[rng.integers(0, nb[1], size=500)]
    got, outside = HN.hist2(x, y, lo, hi, nb)
    want, _, _ = np.histogram2d(x, y, bins=nb, range=((lo[0], hi[0]), (lo[1], hi[1])))
    assert outside == 0 and np.array_equal(got, want.astype(np.int64))
    # the marginals of a joint histogram with nothing outside are the one-dimensional histograms
    assert np.array_equal(got.sum(axis=1), HN.hist1(x, lo[0], hi[0], nb[0])[:nb[0]])
    assert np.array_equal(got.sum(axis=0), HN.hist1(y, lo[1], hi[1], nb[1])[:nb[1]])
    # one value outside on one axis only
    x2 = np.concatenate([x, [cx[0]]]); y2 = np.concatenate([y, [np.nextafter(hi[1], np.inf)]])
    got2, outside2 = HN.hist2(x2, y2, lo, hi, nb)
    assert outside2 == 1 and np.array_equal(got2, got)


def test_restatement_edge_cases():
    """lo = 0, hi = 1, nbins = 8: the edges k / 8 are exact"""
    lo, hi, nb = 0.0, 1.0, 8
    slot = lambda v: int(HN.slots_of(np.array([v]), lo, hi, nb)[0])
    BELOW, ABOVE, NAN = nb, nb + 1, nb + 2
    assert slot(lo) == 0 and slot(hi) == nb - 1                                       # v == hi lies in the last bin
    assert slot(np.nextafter(lo, -np.inf)) == BELOW and slot(np.nextafter(hi, np.inf)) == ABOVE
    assert slot(np.nextafter(lo, np.inf)) == 0 and slot(np.nextafter(hi, -np.inf)) == nb - 1
    for k in range(1, nb):
        assert slot(k / 8) == k and slot(np.nextafter(k / 8, -np.inf)) == k - 1        # an interior edge lies in the upper bin
    assert slot(-0.0) == 0
    assert slot(-np.inf) == BELOW and slot(np.inf) == ABOVE and slot(np.nan) == NAN
    h = HN.hist1(np.array([0.0, 1.0, -0.0, np.nan, np.inf, -np.inf, 0.5, 0.5]), lo, hi, nb)
    assert list(h) == [2, 0, 0, 0, 2, 0, 0, 1, 1, 1, 1] and h.sum() == 8
    # nbins = 1: everything inside is bin 0
    assert list(HN.hist1(np.array([0.0, 0.3, 1.0, 2.0]), lo, hi, 1)) == [3, 0, 1, 0]


def test_restatement_composite_weights():
    """a coarse row of 4 cells with a fine patch over the coarse cells 1 and 2 (NaN there: never read): weights 8 and 1, total 4 * 8"""
    f0 = np.array([0.1, np.nan, np.nan, 0.9]).reshape(4, 1, 1, 1)
    f1 = np.full((8, 2, 2, 1), np.nan)
    f1[2:6, :, :, 0] = 0.6
    boxes = [[((0, 0, 0), (3, 0, 0))], [((2, 0, 0), (5, 1, 1))]]
    c = HN.hist_reference([f0, f1], boxes, [4, 1, 1], [0.0], [1.0], 2)
    assert c.shape == (1, 5) and list(c[0]) == [8, 8 + 16, 0, 0, 0] and c.sum() == 4 * 8
    c2, o2 = HN.hist2_reference([f0[..., 0], f1[..., 0]], [f0[..., 0], f1[..., 0]], boxes, [4, 1, 1], (0.0, 0.0), (1.0, 1.0), (2, 2))
    assert c2.tolist() == [[8, 0], [0, 24]] and o2 == 0


# ------------------------------------------------------------------------------------------------------------------ 2. header, library
def test_header_declares_and_library_exports_the_entries():
    from iamr_amd import lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iamrx.h")).read(), flags=re.S)
    L = lib.lib()
    rng1 = r"const\s+double\s*\*\s*lo,\s*const\s+double\s*\*\s*hi,\s*int\s+nbins"
    rng2 = r"const\s+double\s+lo\[2\],\s*const\s+double\s+hi\[2\],\s*const\s+int\s+nbins\[2\]"
    out = r",\s*long\s+long\s*\*\s*counts"
    nm1, nm2 = r"int\s+nnames,\s*const\s+char\s*\*\s*const\s*\*\s*names,\s*", r"const\s+char\s*\*\s*namex,\s*const\s+char\s*\*\s*namey,\s*"
    for name, args in (("iamrx_mf_histogram", r"iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+ncomp,\s*iamrx_mf\s+cov\s*,\s*" + rng1 + r",\s*long\s+long\s+weight" + out),
                       ("iamrx_mf_histogram2", r"iamrx_mf\s+mf,\s*int\s+compx,\s*int\s+compy,\s*iamrx_mf\s+cov\s*,\s*" + rng2 + r",\s*long\s+long\s+weight" + out),
                       ("iamrx_ns_histogram", r"iamrx_ns\s+\w+,\s*" + nm1 + rng1 + out),
                       ("iamrx_amr_histogram", r"iamrx_amr\s+\w+,\s*" + nm1 + rng1 + out),
                       ("iamrx_ns_histogram2", r"iamrx_ns\s+\w+,\s*" + nm2 + rng2 + out),
                       ("iamrx_amr_histogram2", r"iamrx_amr\s+\w+,\s*" + nm2 + rng2 + out),
                       ("iamrx_hist_bench", r"iamrx_mf\s+mf,\s*int\s+comp,\s*int\s+ncomp,\s*iamrx_mf\s+cov\s*,\s*" + rng1 + r",\s*int\s+nby,\s*int\s+reps,\s*float\s*\*\s*ms")):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", txt), name
        assert hasattr(L, name), name
    # the struct the parameters travel in is untouched: the keys live outside it
    from iamr_amd.ns import ns_params
    assert not [f for f, _ in type(ns_params())._fields_ if "pdf" in f or "hist" in f]


# ------------------------------------------------------------------------------------------------------------------ 3. inputs
def test_pdf_keys_of_the_inputs_file():
    from iamr_amd.inputs import Inputs
    off = Inputs([LDC]).problem()
    assert off["pdf"] == dict(interval=-1, vars=[], nbins=64, range=None, file="pdf")
    on = Inputs([LDC], ["ns.pdf_interval=10", "ns.pdf_vars=x_velocity mag_vort density", "ns.pdf_nbins=128",
                        "ns.pdf_range=-1 1 0 50.5 0.5 2", "ns.pdf_file=out/pdf_"]).problem()
    assert on["pdf"] == dict(interval=10, vars=["x_velocity", "mag_vort", "density"], nbins=128,
                             range=[(-1.0, 1.0), (0.0, 50.5), (0.5, 2.0)], file="out/pdf_")
    # quotes group the names into one value; it is split all the same
    assert Inputs([LDC], ['ns.pdf_interval=1', 'ns.pdf_vars="x_velocity mag_vort"']).problem()["pdf"]["vars"] == ["x_velocity", "mag_vort"]
    # a file without the keys parses exactly as before: nothing but the "pdf" entry knows of them
    assert on["params"] == off["params"] and not any("pdf" in k for k in on["params"])
    assert {k: v for k, v in on.items() if k != "pdf"} == {k: v for k, v in off.items() if k != "pdf"}
    with pytest.raises(ValueError, match="pdf_vars"):
        Inputs([LDC], ["ns.pdf_interval=5"]).problem()
    with pytest.raises(ValueError, match="vorticity_x"):
        Inputs([LDC], ["ns.pdf_interval=5", "ns.pdf_vars=x_velocity vorticity_x"]).problem()
    with pytest.raises(ValueError, match="tracer2"):                                  # the run has no second tracer
        Inputs([LDC], ["ns.pdf_vars=tracer2"]).problem()
    with pytest.raises(ValueError, match="pdf_range"):
        Inputs([LDC], ["ns.pdf_interval=5", "ns.pdf_vars=x_velocity density", "ns.pdf_range=0 1 2"]).problem()
    with pytest.raises(ValueError, match="pdf_range"):
        Inputs([LDC], ["ns.pdf_interval=5", "ns.pdf_vars=x_velocity", "ns.pdf_range=1 1"]).problem()
    for nb in (0, 4097):
        with pytest.raises(ValueError, match="pdf_nbins"):
            Inputs([LDC], ["ns.pdf_interval=5", "ns.pdf_vars=x_velocity", f"ns.pdf_nbins={nb}"]).problem()
    # two-dimensional inputs are accepted
    p2 = Inputs([POIS2D], ["ns.pdf_interval=1", "ns.pdf_vars=x_velocity y_velocity"]).problem()
    assert p2["slab"] and p2["pdf"]["vars"] == ["x_velocity", "y_velocity"]


# ------------------------------------------------------------------------------------------------------------------ 4. dict and files
def _made_up(seed=3, nbins=7):
    from iamr_amd import pdf as P
    rng = np.random.default_rng(seed)
    names = ("x_velocity", "mag_vort", "density")
    counts = rng.integers(0, 2 ** 52, size=(3, nbins + 3), dtype=np.int64)
    counts[2, :nbins] = 0                                                             # a column without a counted cell
    lo = rng.standard_normal(3) * 10.0 ** rng.integers(-8, 8, size=3)
    hi = lo + np.abs(rng.standard_normal(3)) * 10.0 ** rng.integers(-8, 8, size=3) + 1.0e-30
    return P.as_dict(names, counts, lo, hi), counts, lo, hi


def test_dict_of_a_histogram():
    h, counts, lo, hi = _made_up()
    nb = 7
    assert h["names"] == ("x_velocity", "mag_vort", "density") and h["nbins"] == nb
    for q in range(3):
        assert np.array_equal(h["edges"][q], lo[q] + (hi[q] - lo[q]) * np.arange(nb + 1) / nb)
        assert np.array_equal(h["range"][q], [lo[q], hi[q]])
    assert h["counts"].dtype == np.int64 and np.array_equal(h["counts"], counts[:, :nb])
    assert np.array_equal(h["below"], counts[:, nb]) and np.array_equal(h["above"], counts[:, nb + 1]) and np.array_equal(h["nan"], counts[:, nb + 2])
    assert np.array_equal(h["total"], counts.sum(axis=1))
    for q in range(2):
        assert np.array_equal(h["pdf"][q], counts[q, :nb] / (counts[q, :nb].sum() * ((hi[q] - lo[q]) / nb)))
        assert abs(float(np.sum(h["pdf"][q]) * (hi[q] - lo[q]) / nb) - 1.0) < 1e-12        # the PDF integrates to one
    assert not h["pdf"][2].any()
    from iamr_amd.pdf import widen
    assert widen(2.5, 2.5) == (2.0, 3.0) and widen(-1.0, 3.0) == (-1.0, 3.0)


def test_file_round_trip_is_bit_for_bit(tmp_path):
    from iamr_amd import pdf as P
    h, counts, lo, hi = _made_up(5)
    path = str(tmp_path / "pdf00010")
    P.write_pdf(path, h, 10, 0.1 + 0.2)
    lines = open(path).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert head == lines[:len(head)] and len(lines) == len(head) + 7
    assert all(len(l.split()) == 1 + 4 * 3 for l in lines[len(head):])
    assert re.fullmatch(r"\d+", lines[len(head)].split()[3])                            # an integer is written as an integer
    r = P.read_pdf(path)
    assert (r["step"], r["time"], r["names"], r["nbins"]) == (10, 0.1 + 0.2, h["names"], 7)
    for k in ("range", "edges", "counts", "below", "above", "nan", "total", "pdf"):
        assert r[k].dtype == h[k].dtype and r[k].shape == h[k].shape and r[k].tobytes() == h[k].tobytes(), k
