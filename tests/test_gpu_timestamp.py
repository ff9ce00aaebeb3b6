"""GPU: state sampled at the tracer particles (k_part_sample, iamr_amd/csrc/k_particles.hip) and the timestamp files.
1. the kernel against the numpy yardstick tests/timestamp_numpy.py on a two-box level, periodic and with two wall directions;
2. the records of one coarse step of a sub-cycled two-level hierarchy in uniform flow;
3. no basename set: the same bits and no file;
4. the driver on the reference's two-dimensional particle regression inputs with particles.do_timestamps = 1, and a restart; a single
   level with walls;
5. two ranks against one.

The container's arithmetic belongs to AMReX, which is not in the reference tree: nothing here is pinned against it (DESIGN.md section 7
row f8).

Bound of 1: 32 2^-53 max|f| over the array grown by its first ghost layer.  Derived, not measured: indices and weights are identical on
both sides (division and subtraction are correctly rounded); each of the three nested stages a + w (b - a) commits at most 3 roundings on
operands no larger than 2 max|f|, which gives about 15 2^-53 max|f| when the device contracts the stage into a fused multiply-add and
numpy does not; the factor 2 is margin.  A uniform field must come out exact.
Bound of 2 (sampled x-velocity against U): the interpolant is a convex combination of cell values, so it lies within the largest
deviation of the levels' new velocity from U (read from the state) -- to which the existing uniform-flow test's own measure, the largest
deviation of u_mac from U, is added -- plus 64 2^-53 max(1, |U|) of rounding and 1e-10 |U| for the ten printed digits."""
import os
import pathlib
import tempfile
import numpy as np
import pytest

import timestamp_numpy as tn
from test_gpu_particles import N0, PLO, PHI, DX0, BOXES0, UVEL, PATCH_A, _uniform_hierarchy, _around_patch, _umac_deviation

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
EPS = 2.0 ** -53
NG = 2


def _fresh(tmp_path):
    """a directory of this call's own: the suite may run a test twice, once per box mode (tests/conftest.py), and the records are appended"""
    return pathlib.Path(tempfile.mkdtemp(dir=tmp_path))


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------
def _field(rng, per, ncomp=5):
    """cell array over indices -NG .. n + NG - 1: smooth random Fourier modes, periodic images exact in the periodic directions; beyond a
    wall the first ghost layer holds distinct finite values of its own (what a boundary fill would leave); the second ghost layer 1e30"""
    idx = [np.arange(-NG, N0[e] + NG) for e in range(3)]
    ph = []
    for e in range(3):
        pos = idx[e] + 0.5
        if per[e]:
            pos = np.mod(pos, N0[e])
        ph.append(2.0 * np.pi * pos / N0[e])
    X, Y, Z = np.meshgrid(*ph, indexing="ij")
    f = np.zeros(X.shape + (ncomp,))
    for c in range(ncomp):
        for _ in range(4):
            k = rng.integers(0, 3, size=3)
            a, p0 = rng.uniform(-0.4, 0.4), rng.uniform(0, 2 * np.pi)
            f[..., c] += a * np.cos(k[0] * X + k[1] * Y + k[2] * Z + p0)
        f[..., c] += rng.uniform(-0.3, 0.3) + c
    for e in range(3):
        if not per[e]:
            for side in (NG - 1, N0[e] + NG):            # first ghost layer beyond either wall
                sl = [slice(None)] * 3
                sl[e] = side
                f[tuple(sl)] += 10.0 + rng.uniform(0.0, 1.0, f[tuple(sl)].shape)
    return f


def _box_junk(a):
    """the outermost ghost layer of one box's array -> 1e30 (in place)"""
    for e in range(3):
        for side in (0, -1):
            sl = [slice(None)] * 4
            sl[e] = side
            a[tuple(sl)] = 1.0e30


def _positions(rng, per):
    """about 300: random ones; within 1e-12 and at distance 0 of the box interface, of every domain face and of cell centres"""
    span = np.array(PHI) - np.array(PLO)
    x = [rng.uniform(0.0, 1.0, size=(150, 3)) * span + np.array(PLO)]
    planes = [(0, 1.0)] + [(e, c) for e in range(3) for c in (PLO[e], PHI[e])]
    planes += [(e, PLO[e] + (i + 0.5) * DX0[e]) for e in range(3) for i in (0, 3, N0[e] - 1)]
    for e, c in planes:
        for s in (-1e-12, 1e-12, 0.0):
            q = rng.uniform(0.0, 1.0, size=(3, 3)) * span + np.array(PLO)
            q[:, e] = c + s
            x.append(q)
    x = np.concatenate(x)
    # what lies outside a wall would be removed by the placement: keep those inside (a periodic direction wraps them)
    inside = np.all([(x[:, e] >= PLO[e]) & (x[:, e] < PHI[e]) | bool(per[e]) for e in range(3)], axis=0)
    return x[inside]


@pytest.fixture(scope="module")
def sampled(gpu):
    """both geometries once: the container, the filled array, the particles and the yardstick's values for all five components"""
    from iamr_amd.particles import Particles
    lib = gpu
    out = {}
    for name, per in (("periodic", (1, 1, 1)), ("walls", (1, 0, 0))):
        rng = np.random.default_rng(21)
        g = lib.Geom.make(N0, PLO, PHI, per)
        lay = lib.Layout(BOXES0)
        F = _field(rng, per)
        mf = lib.MultiFab(lay, lib.CELL, 5, NG)
        fabs = []
        for li in range(mf.nlocal()):
            lo, hi = mf.fab_box(li)
            a = F[tuple(slice(lo[e] + NG, hi[e] + NG + 1) for e in range(3))].copy()
            _box_junk(a)
            mf.from_numpy(a, li)
            fabs.append((a, lo))
        x0 = _positions(rng, per)
        ids = np.arange(1, len(x0) + 1, dtype=np.int32)
        ids[5] = 0                                      # an invalid particle: dropped by the placement, in no result
        pc = Particles([g], [lay], 1)
        pc.add(x0, ids=ids)
        s = pc.read()
        assert len(s["id"]) == len(x0) - 1 >= 250 and set(s["box"]) == {0, 1} and 0 not in s["id"]
        ref = np.zeros((len(s["id"]), 5))
        for b, (a, lo) in enumerate(fabs):
            sel = s["box"] == b
            ref[sel] = tn.sample(a, lo, s["xyz"][sel], PLO, DX0, (0, 0, 0), [0, 1, 2, 3, 4])
        # max |f| over the array grown by the first ghost layer
        fmax = np.abs(F[NG - 1:-(NG - 1), NG - 1:-(NG - 1), NG - 1:-(NG - 1)]).max()
        out[name] = dict(pc=pc, mf=mf, state=s, ref=ref, fmax=fmax, F=F, keep=(g, lay))
    return out


@pytest.mark.parametrize("comps", [[3], [4, 0, 2]])
@pytest.mark.parametrize("geometry", ["periodic", "walls"])
def test_sample_against_the_yardstick(gpu, sampled, geometry, comps):
    d = sampled[geometry]
    got = d["pc"].sample(0, d["mf"], comps)
    assert np.array_equal(got["id"], d["state"]["id"]) and np.array_equal(got["cpu"], d["state"]["cpu"])
    ref = d["ref"][:, comps]
    assert np.abs(ref).max() < 1e3                       # the 1e30 layer was not read by the yardstick ...
    worst = np.abs(got["values"] - ref).max()
    bound = 32.0 * EPS * d["fmax"]
    print(f"sample {geometry} comps={comps}: worst |gpu - numpy| = {worst:.3e}, bound {bound:.3e} (max|f| = {d['fmax']:.3f})")
    assert worst <= bound                                # ... nor by the kernel
    if geometry == "walls":                              # the first ghost layer beyond a wall (values above 10) shows up in the result
        x = d["state"]["xyz"]
        # component c is c + at most 1.9 in the cells; the layer beyond a wall is 10 to 11 above that.  Within 0.05 dx of a wall the
        # ghost cell weighs at least 0.45: the value is above c + 2; a cell or more away from every wall it is within 1.9 of c
        near = (x[:, 1] < PLO[1] + 0.05 * DX0[1]) | (x[:, 2] > PHI[2] - 0.05 * DX0[2])
        far = (x[:, 1] > PLO[1] + DX0[1]) & (x[:, 1] < PHI[1] - DX0[1]) & (x[:, 2] > PLO[2] + DX0[2]) & (x[:, 2] < PHI[2] - DX0[2])
        assert near.sum() >= 5 and far.sum() >= 50
        assert np.all(got["values"][near, 0] > comps[0] + 2.0) and np.all(np.abs(got["values"][far, 0] - comps[0]) < 2.0)


def test_sample_uniform_field_exact_and_invalid_particle(gpu):
    from iamr_amd.particles import Particles
    lib = gpu
    g = lib.Geom.make(N0, PLO, PHI, (1, 1, 1))
    lay = lib.Layout(BOXES0)
    mf = lib.MultiFab(lay, lib.CELL, 2, 1)
    for li in range(mf.nlocal()):
        lo, hi = mf.fab_box(li)
        a = np.zeros(tuple(hi[e] - lo[e] + 1 for e in range(3)) + (2,))
        a[..., 0], a[..., 1] = 0.1, -3.7e5
        mf.from_numpy(a, li)
    rng = np.random.default_rng(4)
    x0 = _positions(rng, (1, 1, 1))
    pc = Particles([g], [lay], 1)
    pc.add(x0)
    v = pc.sample(0, mf, [1, 0, 1])
    assert np.all(v["values"][:, 0] == -3.7e5) and np.all(v["values"][:, 1] == 0.1) and np.all(v["values"][:, 2] == -3.7e5)
    # positions that are not numbers or far outside: the stencil is clamped to the array, nothing outside it is read
    s = pc.read()
    s["xyz"][3] = (np.nan, 1e300, -1e300)
    pc.set_positions(s["xyz"])
    w = pc.sample(0, mf, [0])
    assert w["values"].shape == (len(x0), 1) and np.all(np.delete(w["values"][:, 0], 3) == 0.1) and w["values"][3, 0] == 0.1
    ids = np.arange(1, 11, dtype=np.int32)
    ids[5] = 0
    pc2 = Particles([g], [lay], 1)
    pc2.add(x0[:10], ids=ids)
    assert pc2.count() == 9 and 0 not in pc2.sample(0, mf, [0])["id"]
    with pytest.raises(lib.IamrxError, match="component"):
        pc.sample(0, mf, [2])
    with pytest.raises(lib.IamrxError, match="components"):
        pc.sample(0, mf, [0] * 17)


# ---- 2. / 3. records of a sub-cycled hierarchy -----------------------------------------------------------------------------------------------
def _state_deviation(amr, N):
    dev = 0.0
    for lev in amr.levels:
        m = lev.data(N.NavierStokes.S_NEW)
        for li in range(m.nlocal()):
            a, lo = m.to_numpy(li)
            blo, bhi, _ = m.layout.local_box(li)
            v = a[tuple(slice(blo[e] - lo[e], bhi[e] - lo[e] + 1) for e in range(3))]
            dev = max(dev, float(np.abs(v[..., 0] - UVEL[0]).max()))
    return dev


def _one_coarse_step(lib, basename):
    from iamr_amd.particles import Particles
    amr, N = _uniform_hierarchy(lib, PATCH_A)
    pc = Particles.for_hierarchy(amr)
    amr.set_particles(pc)
    x0 = _around_patch(PATCH_A, np.random.default_rng(11))
    pc.add(x0)
    before = pc.read_sorted()
    if basename:
        pc.set_timestamp(basename, [0, 3])
    t0 = amr.time
    dt = amr.coarse_step()
    after = pc.read_sorted()
    state = []
    for lev in amr.levels:
        m = lev.data(N.NavierStokes.S_NEW)
        for li in range(m.nlocal()):
            a, lo = m.to_numpy(li)
            blo, bhi, _ = m.layout.local_box(li)
            state.append(a[tuple(slice(blo[e] - lo[e], bhi[e] - lo[e] + 1) for e in range(3))].copy())
    return dict(amr=amr, N=N, pc=pc, before=before, after=after, t0=t0, dt=dt, state=state)


@pytest.fixture(scope="module")
def stepped(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("timestamp_step")
    return _one_coarse_step(gpu, str(d / "Timestamp")), d


def test_records_of_a_subcycled_hierarchy(gpu, stepped):
    """post_timestep_particle (NavierStokesBase.cpp:3866-3951) on two levels, n_cycle = 2: after the first fine sub-step the particles of
    level 1 are written at the fine level's time; after the coarse step's redistribution every particle is written at the coarse time"""
    run, d = stepped
    files = sorted(os.listdir(d))
    assert files == ["Timestamp_00"]
    raw = open(d / "Timestamp_00").read()
    assert raw.endswith("\n") and "  " not in raw and "\t" not in raw
    rows = tn.parse_file(str(d / "Timestamp_00"))
    b, a = run["before"], run["after"]
    n1, ntot = int((b["level"] == 1).sum()), len(b["id"])
    assert n1 > 100 and ntot - n1 > 100
    assert rows.shape == (ntot + n1, 11)                                   # level 1 twice, level 0 once: not more
    t_half, t_full = run["t0"] + 0.5 * run["dt"], run["t0"] + run["dt"]
    first, rest = rows[:n1], rows[n1:]
    assert np.allclose(first[:, 5], t_half, rtol=1e-9, atol=0) and np.allclose(rest[:, 5], t_full, rtol=1e-9, atol=0)
    assert np.array_equal(first[:, 0], b["id"][b["level"] == 1])            # sorted by id: the particles level 1 held
    # the coarse time: one call per level, level 0 first, each sorted by id
    n0_after = int((a["level"] == 0).sum())
    assert np.array_equal(rest[:n0_after, 0], a["id"][a["level"] == 0]) and np.array_equal(rest[n0_after:, 0], a["id"][a["level"] == 1])
    assert np.all(rows[:, 1] == 0)
    o = np.argsort(rest[:, 0], kind="stable")
    final = rest[o]
    assert np.array_equal(final[:, 0], a["id"])
    rel = lambda got, ref: np.abs(got - ref).max() <= 1e-10 * max(1e-300, np.abs(ref).max())
    assert rel(final[:, 2:5], a["xyz"]) and rel(final[:, 6:9], a["r"])       # columns 7-9 are the container's r
    dev = max(_umac_deviation(run["amr"], run["N"]), 0.0) + _state_deviation(run["amr"], run["N"])
    bound = dev + 64.0 * EPS * max(1.0, abs(UVEL[0])) + 1e-10 * abs(UVEL[0])
    worst = np.abs(rows[:, 9] - UVEL[0]).max()
    print(f"records: {len(rows)} lines, worst |sampled u - U| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert np.abs(rows[:, 10] - 1.0).max() <= 1e-10                         # the initial density
    # the first line, character by character, from the yardstick's formatter
    q = int(np.nonzero(b["level"] == 1)[0][0])
    assert raw.split("\n")[0].split(" ")[:2] == [str(int(b["id"][q])), "0"]
    assert all(len(t) == 16 + (t[0] == "-") for t in raw.split("\n")[0].split(" ")[2:])     # d.dddddddddde+dd


def test_off_means_off(gpu, stepped, tmp_path):
    """the same step without set_timestamp: state and particle arrays identical to the bit, and no file anywhere near"""
    run, d = stepped
    tmp_path = _fresh(tmp_path)
    off = _one_coarse_step(gpu, None)
    for k in ("xyz", "r", "id", "cpu", "level", "box"):
        assert np.array_equal(run["after"][k], off["after"][k]), k
    assert off["dt"] == run["dt"] and all(np.array_equal(x, y) for x, y in zip(run["state"], off["state"]))
    assert sorted(os.listdir(d)) == ["Timestamp_00"] and not os.listdir(tmp_path)
    with pytest.raises(gpu.IamrxError, match="basename"):
        off["pc"].timestamp(0, None, 0.0)
    # set and cleared again: off
    off["pc"].set_timestamp(str(tmp_path / "T"), [0])
    off["pc"].set_timestamp(None)
    off["amr"].coarse_step()
    assert not os.listdir(tmp_path)


def test_timestamp_without_values_and_append(gpu, tmp_path):
    """the direct call: mf None ends the line after r2; a second call appends"""
    tmp_path = _fresh(tmp_path)
    from iamr_amd.particles import Particles
    lib = gpu
    g = lib.Geom.make(N0, PLO, PHI, (1, 1, 1))
    pc = Particles([g], [lib.Layout(BOXES0)], 1)
    x = np.array([[1.5, 0.5, 0.25], [0.5, 1.0, 0.75], [0.25, 0.25, 0.5]])
    pc.add(x, ids=[7, 3, 5], r=[[1.0, 2.0, 3.0], [-1.0, 0.0, 0.5], [0.0, 0.0, 0.0]], cpus=[0, 2, 1])
    pc.set_timestamp(str(tmp_path / "Timestamp"), [])
    pc.timestamp(0, None, 0.125)
    expect = (tn.format_line(3, 2, x[1], 0.125, (-1.0, 0.0, 0.5)) + tn.format_line(5, 1, x[2], 0.125, (0.0, 0.0, 0.0))
              + tn.format_line(7, 0, x[0], 0.125, (1.0, 2.0, 3.0)))
    assert open(tmp_path / "Timestamp_00").read() == expect
    pc.set_fixed_dir(1)
    pc.timestamp(0, None, 0.25)
    more = "".join(tn.format_line(i, c, x[q], 0.25, r, fixed_dir=1) for i, c, q, r in ((3, 2, 1, (-1.0, 0.0, 0.5)), (5, 1, 2, (0.0, 0.0, 0.0)), (7, 0, 0, (1.0, 2.0, 3.0))))
    assert open(tmp_path / "Timestamp_00").read() == expect + more


# ---- 4. the driver ---------------------------------------------------------------------------------------------------------------------------
def test_front_end_records_and_restart(gpu, tmp_path, capsys, monkeypatch):
    tmp_path = _fresh(tmp_path)
    from iamr_amd import run as R
    inp = os.path.join(GOLD, "run_2d_particles", "regtest.inputs")
    common = [inp, "amr.n_cell=32 32", "max_step=4", "amr.plot_int=-1", "particles.particles_in_plotfile=0"]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    a.mkdir(), b.mkdir(), c.mkdir()
    assert R.main(common + ["particles.do_timestamps=1", f"particles.timestamp_dir={a}/ts", f"amr.check_file={a}/chk", "amr.check_int=2"]) == 0
    out = capsys.readouterr().out
    steps = [l.split() for l in out.splitlines() if l.startswith("STEP =")]
    times = [float(l[l.index("TIME") + 2]) for l in steps]
    assert len(times) == 4 and "timestamp records" in out
    ignored = [l for l in out.splitlines() if l.startswith("inputs: ignored")]
    assert not any("particles.timestamp" in l for l in ignored)
    path = a / "ts" / "Timestamp_00"
    assert os.path.isfile(path) and os.listdir(a / "ts") == ["Timestamp_00"]
    raw = open(path).read()
    lines = raw.split("\n")[:-1]
    assert all(len(l.split(" ")) == 8 for l in lines)                      # id cpu x y time u v value
    rows = tn.parse_file(str(path))
    assert set(rows[:, 0].astype(int)) == set(range(1, 31))
    # the times: every step time (level 0's records, and the finer level's at the coarse time), and between two of them the fine
    # level's sub-step time for the particles it holds
    allowed = times + [0.5 * (t0 + t1) for t0, t1 in zip([0.0] + times[:-1], times)]
    near = lambda t, ts: min(abs(t - u) for u in ts) <= 1e-9 * max(1.0, abs(t))
    assert all(near(t, allowed) for t in rows[:, 4])
    for t in times:
        at = rows[np.abs(rows[:, 4] - t) <= 1e-9 * max(1.0, abs(t))]
        assert sorted(at[:, 0].astype(int)) == list(range(1, 31))          # all 30 particles once at every step time
    assert np.all(np.diff(rows[:, 4]) >= 0)                                # appended in time order
    # restart from step 2 into the directory as it stood at step 2 (the records are only ever appended: a prefix of the file)
    n2 = int((rows[:, 4] <= times[1] * (1 + 1e-9)).sum())
    os.makedirs(b / "ts")
    with open(b / "ts" / "Timestamp_00", "w") as f:
        f.write("".join(l + "\n" for l in lines[:n2]))
    assert R.main(common + ["particles.do_timestamps=1", f"particles.timestamp_dir={b}/ts", f"amr.check_file={b}/chk", f"amr.restart={a}/chk00002"]) == 0
    capsys.readouterr()
    assert open(b / "ts" / "Timestamp_00").read() == raw
    # without the new key: no directory, here or in the working directory (the file's relative `particle_dir`)
    monkeypatch.chdir(c)
    assert R.main(common[:2] + ["max_step=1", "amr.plot_int=-1", "amr.check_int=-1", "particles.particles_in_plotfile=0"]) == 0
    assert "particles.timestamp_dir" in capsys.readouterr().out
    assert os.listdir(c) == []


def test_single_level_with_walls(gpu, tmp_path, capsys):
    """the single-level step (the l = 0, ngrow = 0 case) in the lid-driven cavity: the sampled array is FillPatched, so next to a wall
    the stencil reads the ghost cell, which holds the wall's value (the moving lid's 1, a no-slip wall's 0) -- it is not clamped to the
    domain.  0.1 dx under the lid the ghost cell weighs 0.4: u = 0.4 + 0.6 u_top with 0 <= u_top <= 1 up to a small undershoot; 0.1 dx
    above the floor u = 0.6 u_bottom, and the fluid there is still nearly at rest after two steps"""
    tmp_path = _fresh(tmp_path)
    from iamr_amd import run as R
    dx = 1.0 / 16
    x0 = np.array([[0.5, 0.5, 1.0 - 0.1 * dx], [0.5, 0.5, 0.1 * dx], [0.3, 0.6, 0.5], [0.1 * dx, 0.4, 0.7]])
    with open(tmp_path / "p.txt", "w") as f:
        f.write("4\n" + "".join("%.17g %.17g %.17g\n" % tuple(q) for q in x0))
    assert R.main([os.path.join(GOLD, "inputs.3d.lid_driven_cavity16"), f"particles.particle_init_file={tmp_path}/p.txt", "max_step=2", "amr.plot_int=-1",
                   "amr.check_int=-1", "particles.do_timestamps=1", f"particles.timestamp_dir={tmp_path}/ts", "particles.timestamp_indices=0 3 4 2"]) == 0
    out = capsys.readouterr().out
    times = [float(l.split()[l.split().index("TIME") + 2]) for l in out.splitlines() if l.startswith("STEP =")]
    rows = tn.parse_file(f"{tmp_path}/ts/Timestamp_00")
    assert rows.shape == (8, 13) and len(times) == 2
    assert np.array_equal(rows[:, 0], [1, 2, 3, 4, 1, 2, 3, 4])
    assert np.allclose(rows[:4, 5], times[0], rtol=1e-9, atol=0) and np.allclose(rows[4:, 5], times[1], rtol=1e-9, atol=0)
    print("lid-driven cavity: sampled u", rows[:, 9], "w", rows[:, 12])
    assert np.all(np.abs(rows[:, 10] - 1.0) <= 1e-10) and np.all(np.isfinite(rows))
    top, bottom = rows[rows[:, 0] == 1], rows[rows[:, 0] == 2]
    assert np.all(np.abs(top[:, 4] - x0[0, 2]) < 0.05 * dx) and np.all(np.abs(bottom[:, 4] - x0[1, 2]) < 0.05 * dx)     # they stayed where the weights are known
    assert np.all(top[:, 9] >= 0.35) and np.all(top[:, 9] <= 1.0)
    assert np.all(np.abs(bottom[:, 9]) < 0.05)
    assert np.all(np.abs(rows[:, 12]) <= 1.0)


# ---- 5. two ranks ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.boxes_kept
def test_two_ranks_write_the_records_of_one(tmp_path):
    """taylorgreen_amr16 (three levels, sub-cycling), 64 particles, one coarse step: the lines of the two rank files together are the
    one-rank file's -- the same (time, id) keys, positions (modulo the period) and values within the 1e-8 that
    tests/test_gpu_particles_multirank.py allows between rank counts"""
    try:
        from test_gpu_particles_multirank import run_group, _particle_file, TOL_RUN
    except Exception as e:                                                 # pragma: no cover
        pytest.skip(f"THE TWO-RANK TIMESTAMP TEST DID NOT RUN: the spawning helper of tests/test_gpu_particles_multirank.py cannot be reused ({e})")
    d = str(tmp_path)
    _particle_file(os.path.join(d, "p64.txt"), 4, 6)

    def job(tag):
        return [os.path.join(GOLD, "inputs.3d.taylorgreen_amr16"), f"particles.particle_init_file={d}/p64.txt", "max_step=1", "amr.plot_int=-1", "amr.check_int=-1",
                "particles.do_timestamps=1", f"particles.timestamp_dir={d}/ts{tag}", "particles.timestamp_indices=0 3"]
    run_group(2, [job(2)], d, "ts_two", with_container=False)
    run_group(1, [job(1)], d, "ts_one", with_container=False)
    assert sorted(os.listdir(f"{d}/ts1")) == ["Timestamp_00"] and sorted(os.listdir(f"{d}/ts2")) == ["Timestamp_00", "Timestamp_01"]
    one = tn.parse_file(f"{d}/ts1/Timestamp_00")
    parts = [tn.parse_file(f"{d}/ts2/Timestamp_0{r}") for r in (0, 1)]
    assert all(len(p) > 0 for p in parts)
    two = np.concatenate(parts)
    assert one.shape[1] == two.shape[1] == 11 and len(one) == len(two) >= 64

    def by_key(rows):
        tq = np.round(rows[:, 5] / (1e-9 * max(1.0, rows[:, 5].max())))    # the printed time, as a key
        return rows[np.lexsort((rows[:, 0], tq))]
    one, two = by_key(one), by_key(two)
    assert np.array_equal(one[:, 0], two[:, 0]) and np.allclose(one[:, 5], two[:, 5], rtol=1e-9, atol=0)
    assert len(set(zip(one[:, 5], one[:, 0]))) == len(one)                 # a (time, id) key appears once
    dx = np.abs(one[:, 2:5] - two[:, 2:5])
    dx = np.minimum(dx, np.abs(1.0 - dx))
    dv = np.abs(one[:, 6:] - two[:, 6:]).max()
    print(f"two ranks against one: {len(one)} lines, largest position difference {dx.max():.3e}, value difference {dv:.3e} (bound {TOL_RUN:.0e})")
    assert dx.max() <= TOL_RUN and dv <= TOL_RUN
