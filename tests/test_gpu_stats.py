"""GPU: on-the-fly velocity statistics (ns.avg_interval / ns.compute_fluctuations) and integrated quantities (ns.sum_interval).

The yardstick is numpy on snapshots the test takes through the C-ABI from INSIDE the driver's own loop (iamr_amd.run.main's `observe`):
the accumulation of NavierStokesBase::time_average (NS_average.cpp:19-69)

    dt_avg += dt;   every avg_interval-th level-0 step:   A += dt_avg * u;   vp = u - A / (time_avg + dt_avg);   R += dt_avg * vp * vp;
                                                          time_avg += dt_avg;   time_avg_fluct += dt_avg (or = 0);   dt_avg = 0

is restated below with the same IEEE operations in the same order (the library is built with FMA contraction off), so accumulators and
scalars are compared with np.array_equal / ==.  der_vel_avg (NS_derive.cpp:11-45): A / time_avg and sqrt(R / time_avg_fluct), a zero
divisor counting as 1.  Integrated quantities (NavierStokes.cpp:1046-1079, amrex volumeWeightedSum): composite sums over the cells no
finer level covers, weight = cell volume; tolerance N 2^-53 sum |term| (N cells summed): the worst-case rounding of ANY summation order
of N terms (each partial sum is off by at most 2^-53 of its magnitude, N - 1 additions), plus one rounding for the volume factor."""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STATS16 = os.path.join(GOLD, "inputs.3d.taylorgreen_stats16")
AMR16 = os.path.join(GOLD, "inputs.3d.taylorgreen_amr16")
REGRID16 = os.path.join(GOLD, "inputs.3d.tracer_regrid16")
SIX = ["x_vel_average", "y_vel_average", "z_vel_average", "x_vel_rms", "y_vel_rms", "z_vel_rms"]
QUIET = ["amr.plot_int=-1", "amr.check_int=-1"]


class Accumulate:
    """numpy restatement of NS_average.cpp:19-69 for one level"""

    def __init__(self, shape, interval, fluct):
        self.A = np.zeros(tuple(shape) + (6,))
        self.interval, self.fluct = interval, fluct
        self.time_avg = self.time_avg_fluct = self.dt_avg = 0.0

    def sample(self, u, dt_level, level0_steps):
        self.dt_avg = self.dt_avg + dt_level                                          # :23
        if level0_steps % self.interval != 0:                                        # :25
            return
        A, R, da = self.A[..., :3], self.A[..., 3:], self.dt_avg
        A[...] = A + da * u                                                           # :45
        if self.fluct:
            vp = u - A / (self.time_avg + da)                                         # :49, the updated A
            R[...] = R + da * vp * vp                                                 # :50
        self.time_avg = self.time_avg + da                                            # :59
        self.time_avg_fluct = self.time_avg_fluct + da if self.fluct else 0.0         # :60-64
        self.dt_avg = 0.0                                                             # :66

    @property
    def state(self):
        return (self.time_avg, self.time_avg_fluct, self.dt_avg)


def der_vel_avg(A, time_avg, time_avg_fluct):
    """NS_derive.cpp:27-43 with the divisions written as divisions"""
    out = np.empty_like(A)
    out[..., :3] = A[..., :3] / (time_avg if time_avg != 0.0 else 1.0)
    out[..., 3:] = np.sqrt(A[..., 3:] / (time_avg_fluct if time_avg_fluct != 0.0 else 1.0))
    return out


def _covered(boxes, n):
    m = np.zeros(tuple(n), dtype=bool)
    for lo, hi in boxes:
        m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    return m


def composite_sums(states, masks, dxs):
    """(sums, rounding bound) of density, tracer and rho |u|^2 / 2 over the cells of every level where masks[l] (counted) is set"""
    tot, mag, ncell = np.zeros(3), np.zeros(3), 0
    for S, m, dx in zip(states, masks, dxs):
        vol = dx[0] * dx[1] * dx[2]
        u, v, w, r, q = (S[..., c][m] for c in range(5))
        terms = [r * vol, q * vol, 0.5 * r * (u * u + v * v + w * w) * vol]
        ncell += int(m.sum())
        for c, t in enumerate(terms):
            tot[c] += float(np.sum(t))
            mag[c] += float(np.sum(np.abs(t)))
    return tot, (ncell + 1) * 2.0 ** -53 * mag          # + 1: the product with the cell volume rounds once more


def _hier_snapshot(amr):
    n0 = list(amr.geom0.n)
    ns = [[v * 2 ** l for v in n0] for l in range(amr.nlev)]
    S = [amr.levels[l].data(0).gather_valid(ns[l]) for l in range(amr.nlev)]
    have = [_covered(amr.layouts[l].boxes, ns[l]) for l in range(amr.nlev)]
    counted = []
    for l in range(amr.nlev):
        m = have[l].copy()
        if l + 1 < amr.nlev:
            m &= ~have[l + 1][::2, ::2, ::2]
        counted.append(m)
    dxs = [[(amr.geom0.prob_hi[d] - amr.geom0.prob_lo[d]) / ns[l][d] for d in range(3)] for l in range(amr.nlev)]
    return ns, S, have, counted, dxs


# ------------------------------------------------------------------------------------------------------------------ single level
@pytest.mark.parametrize("fluct", [0, 1])
@pytest.mark.parametrize("interval", [1, 3])
def test_accumulators_equal_numpy_to_the_bit(gpu, interval, fluct):
    """TaylorGreen 16^3, viscous, 7 steps through the driver's loop: after post_init and after every step the accumulators equal the numpy
    accumulation of the velocities read at those moments with the dt values the run reports, and the three scalars are the same doubles;
    derive("velocity_average") equals A / T and sqrt(R / Tf) exactly.  Mean-only runs leave components 3..5 zero."""
    from iamr_amd import run as R
    n = [16, 16, 16]
    ref = Accumulate(n, interval, fluct)
    seen = []

    def observe(ns, step, dt):
        u = ns.data(ns.S_NEW).gather_valid(n)[..., :3]
        ref.sample(u, ns.dt if dt is None else dt, step)
        A = ns.data(ns.AVERAGE).gather_valid(n)
        assert A.shape == (16, 16, 16, 6)
        worst = float(np.abs(A - ref.A).max())
        print(f"step {step}: max |A - numpy| = {worst:.3e}, scalars {ns.average_state} vs {ref.state}")
        assert np.array_equal(A, ref.A), (step, worst)
        assert ns.average_state == ref.state, (step, ns.average_state, ref.state)
        D = ns.derive("velocity_average").gather_valid(n)
        assert np.array_equal(D, der_vel_avg(ref.A, ref.time_avg, ref.time_avg_fluct)), step
        seen.append(step)

    assert R.main([STATS16, f"ns.avg_interval={interval}", f"ns.compute_fluctuations={fluct}", "ns.sum_interval=-1", "max_step=7"] + QUIET, observe) == 0
    assert seen == list(range(8))
    assert float(np.abs(ref.A[..., :3]).max()) > 1e-3 and ref.time_avg > 0.0            # something was accumulated
    if fluct:
        assert float(ref.A[..., 3:].max()) > 0.0 and ref.time_avg_fluct == ref.time_avg
    else:
        assert not ref.A[..., 3:].any() and ref.time_avg_fluct == 0.0


def test_derive_before_the_first_sample_and_refusal_without_averages(gpu):
    """both divisors zero: velocity_average returns A and sqrt(R) (der_vel_avg's factor 1); a level without averages knows neither the
    derived quantity nor the accumulator array nor the scalars"""
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd.lib import IamrxError
    n = [16, 16, 16]
    g = L.Geom.make(n, periodic=(1, 1, 1))
    lay = L.Layout.decompose(tuple(n), 8)
    ns = N.NavierStokes(g, lay, N.ns_params(avg_interval=2, compute_fluctuations=1))
    ns.init_taylorgreen(1.0, 1.0, 1.0, 0.0, 1.0)
    assert ns.average_state == (0.0, 0.0, 0.0) and not ns.data(ns.AVERAGE).gather_valid(n).any()      # zero at initialisation
    rng = np.random.default_rng(7)
    G = rng.uniform(0.1, 2.0, size=(16, 16, 16, 6))
    G[..., :3] -= 1.0
    mf = L.MultiFab(lay, L.CELL, 6, 0)
    mf.set_from_global(G, (0, 0, 0))
    ns.set_data(ns.AVERAGE, mf)
    assert np.array_equal(ns.data(ns.AVERAGE).gather_valid(n), G)
    D = ns.derive("velocity_average").gather_valid(n)
    assert np.array_equal(D[..., :3], G[..., :3]) and np.array_equal(D[..., 3:], np.sqrt(G[..., 3:]))
    ns.average_state = (0.75, 0.5, 0.125)
    assert ns.average_state == (0.75, 0.5, 0.125)
    assert np.array_equal(ns.derive("velocity_average").gather_valid(n), der_vel_avg(G, 0.75, 0.5))
    # an odd level0_steps with avg_interval = 2: only dt_avg moves
    ns.time_average(0.25, 1)
    assert ns.average_state == (0.75, 0.5, 0.375) and np.array_equal(ns.data(ns.AVERAGE).gather_valid(n), G)
    plain = N.NavierStokes(g, lay, N.ns_params())
    plain.init_taylorgreen(1.0, 1.0, 1.0, 0.0, 1.0)
    plain.time_average(0.1, 0)                        # a no-op
    for call in (lambda: plain.derive("velocity_average"), lambda: plain.data(plain.AVERAGE), lambda: plain.average_state):
        with pytest.raises(IamrxError):
            call()


def test_uniform_flow_keeps_its_mean_and_no_fluctuation(gpu):
    """a uniform inviscid flow stays uniform to round-off (the pin of tests/test_cpu_oracle_amr.py), so mean = u and rms = 0 to 1e-13 |u|"""
    from iamr_amd import run as R
    n = [16, 16, 16]
    u0 = np.array([1.0, 0.2, 0.0])
    tol = 1e-13 * float(np.abs(u0).max())
    last = {}

    def observe(ns, step, dt):
        last["D"] = ns.derive("velocity_average").gather_valid(n)
        last["T"] = ns.average_state

    assert R.main([REGRID16, "amr.max_level=0", "ns.vel_visc_coef=0.0", "ns.avg_interval=1", "ns.compute_fluctuations=1", "max_step=5"] + QUIET, observe) == 0
    D = last["D"]
    em, er = float(np.abs(D[..., :3] - u0).max()), float(np.abs(D[..., 3:]).max())
    print(f"uniform flow: max |mean - u| = {em:.3e}, max rms = {er:.3e} (bound {tol:.1e}); T = {last['T']}")
    assert last["T"][0] > 0.0 and em <= tol and er <= tol


def test_sums_of_one_level(gpu, capsys):
    """the fused reduction against numpy on the gathered state (rounding bound of the module docstring); the same call twice gives the same
    bits; the three printed lines carry the returned numbers with 12 significant digits"""
    from iamr_amd import run as R
    n = [16, 16, 16]
    got = []

    def observe(ns, step, dt):
        S = ns.data(ns.S_NEW).gather_valid(n)
        a, b = ns.sum_integrated(), ns.sum_integrated()
        assert a == b
        ref, bound = composite_sums([S], [np.ones(n, dtype=bool)], [[1.0 / 16] * 3])
        print(f"step {step}: sums {a}, |diff| {np.abs(np.array(a) - ref)}, bound {bound}")
        assert np.all(np.abs(np.array(a) - ref) <= bound), (a, ref, bound)
        got.append((ns.time, a))

    assert R.main([STATS16, "max_step=3"] + QUIET, observe) == 0
    out = capsys.readouterr().out
    assert got[0][1][0] > 0.9 and got[0][1][2] > 0.01                        # density 1 on the unit cube; a flow
    for name, c in (("MASS", 0), ("TRAC", 1), ("KINETIC ENERGY", 2)):
        lines = [l for l in out.splitlines() if l.startswith("TIME= ") and f" {name}= " in l]
        assert len(lines) == 4, (name, lines)                                # after post_init and after each of the 3 steps
        for l, (t, sums) in zip(lines, got):
            assert l == f"TIME= {t:.12g} {name}= {sums[c]:.12g}"
            assert abs(float(l.rsplit("= ", 1)[1]) - sums[c]) <= 5e-12 * abs(sums[c]) + 1e-300


def test_nan_reaches_the_sums(gpu):
    """a NaN in a counted cell gives NaN, never a clean number"""
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    n = [16, 16, 16]
    g = L.Geom.make(n, periodic=(1, 1, 1))
    lay = L.Layout.decompose(tuple(n), 8)
    ns = N.NavierStokes(g, lay, N.ns_params())
    ns.init_taylorgreen(1.0, 1.0, 1.0, 0.0, 1.0)
    assert all(np.isfinite(v) for v in ns.sum_integrated())
    S = ns.data(ns.S_NEW)
    for li in range(S.nlocal()):
        a, lo = S.to_numpy(li)
        if li == S.nlocal() - 1:
            a[3, 4, 5, 3] = np.nan                                           # the density of one valid cell (the fab has one ghost layer)
        S.from_numpy(a, li)
    ns.set_data(ns.S_NEW, S)
    m, t, e = ns.sum_integrated()
    assert np.isnan(m) and np.isfinite(t) and np.isnan(e)


# ------------------------------------------------------------------------------------------------------------------ hierarchy
def test_two_level_hierarchy(gpu, capsys):
    """fixed two-level grids (inputs.3d.taylorgreen_amr16 with amr.max_level = 1), 3 coarse steps: level 0's accumulators equal the numpy
    accumulation of level-0 snapshots taken after every coarse step (level 0's post_timestep ends the step) to the bit; time_avg is the same
    double on both levels and equals dt_level0(init) + sum of the coarse dt to 4 ulp; the composite sums equal numpy's within the rounding
    bound, twice the same bits, and the mass stays constant within the 1e-12 tests/test_gpu_amr_step.py allows the same property"""
    from iamr_amd import run as R
    ref = Accumulate([16, 16, 16], 1, 1)
    rec = dict(dts=[], mass=[], sums=[])

    def observe(amr, step, dt):
        assert amr.nlev == 2
        ns_, S, have, counted, dxs = _hier_snapshot(amr)
        w = amr.dts()[0] if dt is None else dt
        rec["dts"].append(w)
        ref.sample(S[0][..., :3], w, step)
        A0 = amr.levels[0].data(12).gather_valid(ns_[0])
        assert np.array_equal(A0, ref.A), (step, float(np.abs(A0 - ref.A).max()))
        st = [amr.levels[l].average_state for l in range(2)]
        assert st[0] == ref.state and st[1] == st[0], (step, st, ref.state)
        a, b = amr.sum_integrated(), amr.sum_integrated()
        assert a == b
        want, bound = composite_sums(S, counted, dxs)
        print(f"step {step}: sums {a}, |diff| {np.abs(np.array(a) - want)}, bound {bound}")
        assert np.all(np.abs(np.array(a) - want) <= bound), (a, want, bound)
        assert amr.last_sum() == (step, amr.time, a)                          # what level 0's post_timestep computed by itself
        rec["mass"].append(a[0]); rec["sums"].append((amr.time, a))

    argv = [AMR16, "amr.max_level=1", "ns.avg_interval=1", "ns.compute_fluctuations=1", "ns.sum_interval=1", "max_step=3"] + QUIET
    assert R.main(argv, observe) == 0
    out = capsys.readouterr().out
    closed = float(np.sum(np.array(rec["dts"])))
    assert abs(ref.time_avg - closed) <= 4 * np.spacing(closed), (ref.time_avg, closed)
    assert max(abs(m - rec["mass"][0]) for m in rec["mass"]) <= 1e-12, rec["mass"]
    lines = [l for l in out.splitlines() if l.startswith("TIME= ") and " MASS= " in l]
    assert lines == [f"TIME= {t:.12g} MASS= {s[0]:.12g}" for t, s in rec["sums"]]


def test_uniform_flow_on_the_fine_level(gpu):
    """fine sub-steps cannot be snapshotted from outside; on a uniform flow every sample is u, so A / T == u on the fine level to 1e-13"""
    from iamr_amd import run as R
    u0 = np.array([1.0, 0.2, 0.0])
    last = {}

    def observe(amr, step, dt):
        ns_, S, have, counted, dxs = _hier_snapshot(amr)
        last["D"] = amr.levels[1].derive("velocity_average").gather_valid(ns_[1])[have[1]]
        last["T"] = [amr.levels[l].average_state for l in range(2)]

    # the uniform flow of inputs.3d.tracer_regrid16 under one refined level that keeps its initial grids (no regrid within the run)
    argv = [REGRID16, "amr.max_level=1", "amr.regrid_int=1000", "ns.avg_interval=1", "ns.compute_fluctuations=1", "max_step=3"] + QUIET
    assert R.main(argv, observe) == 0
    D = last["D"]
    em, er = float(np.abs(D[:, :3] - u0).max()), float(np.abs(D[:, 3:]).max())
    print(f"fine level: max |mean - u| = {em:.3e}, max rms = {er:.3e}; T = {last['T']}")
    assert D.shape[0] > 0 and last["T"][0] == last["T"][1] and last["T"][0][0] > 0.0
    assert em <= 1e-13 and er <= 1e-13


def test_regrid_carries_the_averages(gpu):
    """inputs.3d.tracer_regrid16 (a uniform flow carrying the tracer blob the grids follow), 6 coarse steps with regrids that create and
    move fine boxes: in every cell of every refined level A / T == u to 1e-13 and the rms is zero, and the three scalars equal level 0's.
    A new level whose accumulators were left unfilled fails this."""
    from iamr_amd import run as R
    u0 = np.array([1.0, 0.2, 0.0])
    grids, worst = [], [0.0, 0.0]

    def observe(amr, step, dt):
        ns_, S, have, counted, dxs = _hier_snapshot(amr)
        grids.append([list(amr.layouts[l].boxes) for l in range(1, amr.nlev)])
        t0 = amr.levels[0].average_state
        assert t0[0] > 0.0
        for l in range(amr.nlev):
            assert amr.levels[l].average_state == t0, (step, l, amr.levels[l].average_state, t0)
            D = amr.levels[l].derive("velocity_average").gather_valid(ns_[l])[have[l]]
            em, er = float(np.abs(D[:, :3] - u0).max()), float(np.abs(D[:, 3:]).max())
            worst[0], worst[1] = max(worst[0], em), max(worst[1], er)
            uni = float(np.abs(S[l][..., :3][have[l]] - u0).max())
            print(f"step {step} level {l}: max |mean - u| = {em:.3e}, max rms = {er:.3e}, flow itself off uniform by {uni:.3e}")
            assert em <= 1e-13 and er <= 1e-13, (step, l, em, er)

    assert R.main([REGRID16, "ns.avg_interval=1", "ns.compute_fluctuations=1", "max_step=6"] + QUIET, observe) == 0
    print(f"regrid run: max |mean - u| = {worst[0]:.3e}, max rms = {worst[1]:.3e}; level counts {[len(g) + 1 for g in grids]}")
    assert max(len(g) for g in grids) == 2                                     # three levels existed
    assert any(a != b for a, b in zip(grids, grids[1:])), "no regrid changed the fine boxes: the run tested nothing"


# ------------------------------------------------------------------------------------------------------------------ plotfile, checkpoint
def test_plotfile_holds_velocity_average(gpu, tmp_path):
    """the fixture run: the plotfile's variables end with the six names and energy, and its data equal derive()"""
    from iamr_amd import run as R
    from iamr_amd.plotfile import PlotFile, state_names
    n = [16, 16, 16]
    last = {}

    def observe(ns, step, dt):
        last["va"] = ns.derive("velocity_average").gather_valid(n)
        last["en"] = ns.derive("energy").gather_valid(n)

    root = str(tmp_path / "plt")
    assert R.main([STATS16, f"amr.plot_file={root}", "amr.check_int=-1"], observe) == 0
    pf = PlotFile.read(root + "00004")
    assert pf.names == state_names() + SIX + ["energy"]
    lv = pf.levels[0]
    assert len(lv.boxes) == 8
    for (lo, hi), a in zip(lv.boxes, lv.data):
        sl = tuple(slice(lo[d], hi[d] + 1) for d in range(3))
        assert np.array_equal(a[..., 5:11], last["va"][sl]) and np.array_equal(a[..., 11], last["en"][sl][..., 0])
    assert float(np.abs(last["va"][..., :2]).max()) > 0.1 and float(last["va"][..., 3:5].max()) > 0.0


def _chk_arrays(path, name, level=0):
    from iamr_amd import checkpoint
    return checkpoint._read_vismf(os.path.join(path, f"Level_{level}"), name)


def test_checkpoint_and_restart(gpu, tmp_path):
    """4 steps with a checkpoint every 2; restarted from chk00002 and continued to step 4: accumulators, scalars and state are bit for bit
    those of the uninterrupted run.  With ns.avg_in_checkpoint = 0 the accumulators restart from zero and time_avg is the time of the two
    continued steps.  A checkpoint without the averages read with avg_in_checkpoint = 1 raises."""
    from iamr_amd import run as R
    from iamr_amd import checkpoint
    n = [16, 16, 16]
    d = str(tmp_path)
    assert R.main([STATS16, "amr.plot_int=-1", "amr.check_int=2", f"amr.check_file={d}/chkA_"]) == 0
    hd = checkpoint.read_header(f"{d}/chkA_00002")
    assert hd["level_steps"] == [2]
    assert sorted(f for f in os.listdir(f"{d}/chkA_00002/Level_0") if f.startswith("SD_3")) == ["SD_3_New_MF_D_00000", "SD_3_New_MF_H"]
    assert open(f"{d}/chkA_00002/TimeAverage").readline() == "Writing time_average to checkpoint\n"
    assert R.main([STATS16, "amr.plot_int=-1", "amr.check_int=2", f"amr.check_file={d}/chkB_", f"amr.restart={d}/chkA_00002"]) == 0
    for name in ("SD_0_New_MF", "SD_0_Old_MF", "SD_1_New_MF", "SD_2_New_MF", "SD_3_New_MF"):
        for x, y in zip(_chk_arrays(f"{d}/chkA_00004", name), _chk_arrays(f"{d}/chkB_00004", name)):
            assert np.array_equal(x, y), (name, float(np.abs(x - y).max()))
    assert open(f"{d}/chkA_00004/TimeAverage").read() == open(f"{d}/chkB_00004/TimeAverage").read()
    ta, tf = checkpoint.read_time_average(f"{d}/chkA_00004")
    assert ta > 0.0 and tf == ta and float(np.abs(_chk_arrays(f"{d}/chkA_00004", "SD_3_New_MF")[0]).max()) > 0.0

    # averaging switched on at the restart: zero accumulators, the weights of the two continued steps
    ref = Accumulate(n, 1, 1)
    got = {}

    def observe(ns, step, dt):
        ref.sample(ns.data(ns.S_NEW).gather_valid(n)[..., :3], dt, step)
        got["A"], got["T"] = ns.data(ns.AVERAGE).gather_valid(n), ns.average_state

    assert R.main([STATS16, "ns.avg_in_checkpoint=0"] + QUIET + [f"amr.restart={d}/chkA_00002"], observe) == 0
    assert np.array_equal(got["A"], ref.A) and got["T"] == ref.state and ref.time_avg < ta

    # a checkpoint of a run without averages: the layout every earlier checkpoint had, and no averages to restart from
    assert R.main([STATS16, "ns.avg_interval=0", "amr.derive_plot_vars=NONE", "amr.plot_int=-1", "amr.check_int=2", "max_step=2", f"amr.check_file={d}/chkP_"]) == 0
    per_mf = lambda nm: [nm + "_D_00000", nm + "_H"]
    want = sorted(sum([per_mf(f"SD_{t}_{tag}_MF") for t in range(3) for tag in ("New", "Old")] + [per_mf(f"MacPhiHist_{q}") for q in range(2)], []))
    assert sorted(os.listdir(f"{d}/chkP_00002/Level_0")) == want
    assert sorted(os.listdir(f"{d}/chkP_00002")) == ["Header", "Level_0", "iamrx_restart.json"]
    H = open(f"{d}/chkP_00002/Header").read().split("\n")
    q = H.index(")")                                                          # end of level 0's BoxArray: the number of state types follows
    assert H[q + 1] == "3" and "SD_3" not in "\n".join(H)
    HA = open(f"{d}/chkA_00002/Header").read().split("\n")
    assert HA[HA.index(")") + 1] == "4" and HA[-3:] == ["1", "Level_0/SD_3_New_MF", ""]
    with pytest.raises(RuntimeError, match="avg_in_checkpoint"):
        R.main([STATS16] + QUIET + [f"amr.restart={d}/chkP_00002"])
