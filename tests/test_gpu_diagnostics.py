"""GPU: the host side of the diagnostics (iamr_amd/csrc/diagnostics.hip): the field table, the resolver from names to (array, component)
and the one loop over levels behind histogram, histogram2, integrate, plane_profile and sum_integrated.

Everything here is an exact comparison: the counts are integers, and a per-name result must not depend on which other names stand in the
list (k_sum_comps finishes every component on its own in a fixed tile order; the velocity-gradient kernel forms every quantity on its
own).  Two fixtures: a single periodic level of four unequal boxes whose largest holds a 32 x 8 tile (the marching form of the
velocity-gradient kernel), and the three levels of inputs.3d.taylorgreen_amr16 with random data (boxes of 16 cells and less: the plain
form, and two masked levels).  tests/golden/diagnostics_parent.json holds what the commit before the diagnostics moved into one
translation unit gave for both (tools/record_diagnostics_golden.py wrote it)."""
import itertools
import json
import os
import numpy as np
import pytest
import hist_numpy as HN
from test_gpu_profile import random_state, put_state, as_array

pytestmark = [pytest.mark.gpu, pytest.mark.both_box_modes]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
GOLDEN_FILE = os.path.join(GOLD, "diagnostics_parent.json")
MU = 0.01
N1, MGS1 = (44, 12, 6), (32, 8, 8)
# state, velocity-gradient and pointwise names interleaved
MIXED = ["enstrophy", "density", "dissipation", "energy", "x_velocity", "q_criterion", "avg_pressure", "tracer"]
# fixed ranges that cut into the data of both fixtures (the gradients of the random data grow with the level: the fine levels fill `above`)
RANGES = {"enstrophy": (0.0, 4000.0), "density": (0.75, 2.0), "dissipation": (0.0, 60.0), "energy": (0.1, 2.0), "x_velocity": (-0.5, 1.0),
          "q_criterion": (-2000.0, 2000.0), "avg_pressure": (-0.4, 0.3), "tracer": (-0.5, 1.6), "mag_vort": (0.0, 80.0)}
PERMS = [[3, 7, 0, 5, 1, 6, 2, 4], [5, 2, 0, 4, 7, 1, 3, 6]]
STATE = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer"]
POINTWISE = ["energy", "mag_vort", "avg_pressure"]
VELGRAD = ["diveru", "vort_x", "vort_y", "vort_z", "enstrophy", "strain_rate", "dissipation", "q_criterion", "r_invariant", "helicity"]


def put_pressure(level, lay, n, seed):
    """the new-time pressure of a level := random values that depend on the node alone (a node two boxes share holds one value)"""
    from iamr_amd import lib as L
    P = np.random.default_rng(seed).uniform(-1.0, 1.0, size=tuple(v + 3 for v in n))
    mf = L.MultiFab(lay, L.NODE, 1, 1)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        a = P[tuple(slice(glo[d] + 1, ghi[d] + 2) for d in range(3))]
        mf.from_numpy(np.asfortranarray(a[..., None]), li)
    level.set_data(level.P_NEW, mf)


def fill_level(level, lay, n, seed):
    level.init_rest(1.0)
    put_state(level, lay, random_state(n, seed))
    put_pressure(level, lay, n, seed + 100)


def single_level(**params):
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    lay = L.Layout.decompose(N1, MGS1)
    assert len({tuple(hi[d] - lo[d] + 1 for d in range(3)) for lo, hi in lay.boxes}) == 4
    ns = N.NavierStokes(L.Geom.make(list(N1), periodic=(1, 1, 1)), lay, N.ns_params(visc_coef=MU, **params))
    fill_level(ns, lay, N1, 41)
    return ns


def hierarchy_of_one():
    """the boxes and data of single_level as an Amr with max_level = 0"""
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd.amr import Amr
    lay = L.Layout.decompose(N1, MGS1)
    amr = Amr(L.Geom.make(list(N1), periodic=(1, 1, 1)), [lay], N.ns_params(visc_coef=MU))
    fill_level(amr.levels[0], lay, N1, 41)
    return amr


def hierarchy():
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    amr, lays, g0 = R.build_amr(Inputs([AMR16], [f"ns.vel_visc_coef={MU}"]).problem(), L, N)
    assert amr.nlev == 3
    for l in range(amr.nlev):
        fill_level(amr.levels[l], amr.layouts[l], [v << l for v in amr.geom0.n], 20 + l)
    return amr


def box_mode():
    """the suite runs every test here with the level objects' boxes merged and with the callers' boxes kept (conftest.py)"""
    return "kept" if os.environ.get("IAMRX_COALESCE") == "0" else "merged"


_BUILT = {}


def fixture_of(which):
    """the single level or the hierarchy, built once per box mode and never modified"""
    key = (which, box_mode())
    if key not in _BUILT:
        _BUILT[key] = single_level() if which == "level" else hierarchy()
    return _BUILT[key]


def slots(h):
    return np.concatenate([h["counts"], h["below"][:, None], h["above"][:, None], h["nan"][:, None]], axis=1)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def hist_of(run, names):
    return slots(run.histogram(names, 16, [RANGES[nm] for nm in names]))


def fields_of(run, names):
    """derive_fields of every level: a list of arrays (boxes in order, valid cells) per level"""
    out = []
    for lev in run.levels:
        mf = lev.derive_fields(names)
        out.append([mf.to_numpy(li)[0].copy() for li in range(mf.nlocal())])
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. grouping
@pytest.mark.parametrize("which", ["level", "hierarchy"])
def test_independence_of_grouping(gpu, which):
    """integrate, histogram and derive_fields of the mixed list: the same bits name by name and in two other orders"""
    run = fixture_of(which)
    I, H, F = run.integrate(MIXED), hist_of(run, MIXED), fields_of(run, MIXED)
    assert np.isfinite(I).all() and not H[:, 18].any() and (H[:, :16].sum(axis=1) > 0).all()
    for q, nm in enumerate(MIXED):
        assert np.array_equal(bits(run.integrate([nm])), bits(I[q:q + 1])), nm
        assert np.array_equal(hist_of(run, [nm])[0], H[q]), nm
        for one, full in zip(fields_of(run, [nm]), F):
            for a, b in zip(one, full):
                assert np.array_equal(bits(a[..., 0]), bits(b[..., q])), nm
    for perm in PERMS:
        names = [MIXED[q] for q in perm]
        assert np.array_equal(bits(run.integrate(names)), bits(I[perm])), names
        assert np.array_equal(hist_of(run, names), H[perm]), names
        for lp, lf in zip(fields_of(run, names), F):
            for a, b in zip(lp, lf):
                assert np.array_equal(bits(a), bits(b[..., perm])), names


@pytest.mark.parametrize("namex,namey", [("x_velocity", "density"), ("tracer", "enstrophy"), ("q_criterion", "dissipation"), ("energy", "enstrophy")],
                         ids=["state-state", "state-velgrad", "velgrad-velgrad", "pointwise-velgrad"])
def test_joint_histogram_pairings(gpu, namex, namey):
    """histogram2 against numpy's binning rule applied to what derive_fields gives for the pair, level by level"""
    nb, rx, ry = (5, 9), RANGES[namex], RANGES[namey]
    for run in (fixture_of("level"), fixture_of("hierarchy")):
        nlev = len(run.levels)
        n0 = list(run.levels[0].geom.n)
        boxes = [lev.layout.boxes for lev in run.levels]
        f = [lev.derive_fields([namex, namey]).gather_valid([v << l for v in n0]) for l, lev in enumerate(run.levels)]
        c, o = HN.hist2_reference([a[..., 0] for a in f], [a[..., 1] for a in f], boxes, n0, (rx[0], ry[0]), (rx[1], ry[1]), nb)
        h = run.histogram2(namex, namey, nb, (rx, ry))
        assert np.array_equal(h["counts"], c) and h["outside"] == o and h["total"] == n0[0] * n0[1] * n0[2] * 8 ** (nlev - 1)
        assert c.sum() > 0


# ------------------------------------------------------------------------------------------------------------------ 2. a hierarchy of one
def all_five(run):
    r = dict(integrate=bits(run.integrate(MIXED)), sum_integrated=bits(run.sum_integrated()), histogram=hist_of(run, MIXED))
    h2 = run.histogram2("energy", "enstrophy", (5, 9), (RANGES["energy"], RANGES["enstrophy"]))
    r["histogram2"] = np.append(h2["counts"].ravel(), h2["outside"])
    for d in range(3):
        r[f"plane_profile{d}"] = bits(as_array(run.plane_profile(d)))
    return r


def test_level_equals_hierarchy_of_one(gpu):
    a, b = all_five(fixture_of("level")), all_five(hierarchy_of_one())
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------------------------ 3. acceptance
# Which entry point takes which name, read from the code before the field table existed (NavierStokes::derive's chain of name tests,
# hist_field, and derive_fields' "state name, else derive()").  derive forms no state component; only derive knows the six-component
# velocity_average, and only with averaging on; the particle counts exist only in a run with particles bound (there is none here).
ABSENT = ["tracer2", "temp", "particle_count", "total_particle_count", "vorticity"]
ENTRIES = ["derive", "derive_fields", "integrate", "histogram", "histogram2"]


def accepted(entry, name, averaging):
    if name in POINTWISE or name in VELGRAD:
        return True
    if name in STATE:
        return entry != "derive"
    if name == "velocity_average":
        return entry == "derive" and averaging
    return False


def calls(run, entry, name):
    """the calls that hand `name` to an entry point, one per slot that takes a name"""
    return [lambda slot=slot: call(run, entry, name, slot) for slot in ((0, 1) if entry == "histogram2" else (0,))]


def call(run, entry, name, slot=0):
    if entry == "derive":
        run.derive(name)
    elif entry == "derive_fields":
        run.derive_fields([name])
    elif entry == "integrate":
        run.integrate([name])
    elif entry == "histogram":
        run.histogram([name], 8, (0.0, 1.0))
    else:
        run.histogram2(*((name, "density") if slot == 0 else ("density", name)), (4, 4), ((0.0, 1.0), (0.0, 1.0)))


@pytest.mark.parametrize("averaging", [False, True], ids=["plain", "averaging"])
def test_acceptance_matrix(gpu, averaging):
    from iamr_amd.lib import IamrxError
    from iamr_amd.amr import Amr
    ns = single_level(avg_interval=1) if averaging else single_level()
    amr = Amr(ns.geom, [ns.layout], ns.params)
    fill_level(amr.levels[0], ns.layout, N1, 41)
    for entry, name in itertools.product(ENTRIES, STATE + POINTWISE + VELGRAD + ["velocity_average"] + ABSENT):
        for run in (ns, amr) if entry in ("integrate", "histogram", "histogram2") else (ns,):
            for one in calls(run, entry, name):
                if accepted(entry, name, averaging):
                    one()
                else:
                    with pytest.raises(IamrxError):
                        one()
    if averaging:
        assert ns.derive("velocity_average").ncomp == 6
    for entry in ("derive", "histogram"):                          # the messages list the known names
        for word in ("mag_vort", "q_criterion"):
            with pytest.raises(IamrxError, match=word):
                call(ns, entry, "vorticity")


# ------------------------------------------------------------------------------------------------------------------ 4. the parent commit
def record(run, bin_levels):
    """what the golden file holds for one fixture: floats as hex strings, counts as integers"""
    hexes = lambda a: [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]
    r = dict(integrate=hexes(run.integrate(MIXED)), histogram=hist_of(run, MIXED).tolist(), sum_integrated=hexes(run.sum_integrated()))
    for b in bin_levels:
        r[f"plane_profile_dir0_bin_level{b}"] = hexes(as_array(run.plane_profile(0, b)))
    return r


def record_all():
    """both fixtures in the box mode of the moment"""
    return dict(level=record(fixture_of("level"), [0]), hierarchy=record(fixture_of("hierarchy"), [0, 1]))


@pytest.mark.parametrize("which", ["level", "hierarchy"])
def test_against_the_parent_commit(gpu, which):
    with open(GOLDEN_FILE) as f:
        gold = json.load(f)
    assert gold["names"] == MIXED and gold["nbins"] == 16 and gold["ranges"] == [list(RANGES[nm]) for nm in MIXED]
    got, want = record_all()[which], gold[box_mode()][which]
    assert sorted(got) == sorted(want)
    for key in got:
        assert got[key] == want[key], key
    assert len(got["plane_profile_dir0_bin_level0"]) == 14 * (N1[0] if which == "level" else 16)
