"""GPU: plotfiles, checkpoints and restart of runs on several ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py).  Two kinds of comparison: what was WRITTEN against what the ranks HELD is exact (I/O moves doubles);
an N-rank run against a 1-rank run uses the constants tests/test_gpu_dist.py asserts (state within 1e-9 on a single level, 1e-8 for a
hierarchy or a regridded run, dts at rtol 1e-10) on the state variables only.

One spawn serves several checks: the runs through iamr_amd.run.main are grouped by world size into a few spawned process groups whose
ranks call R.main several times (a fresh rendezvous port per call); the module-scoped fixtures below hold their output directories."""
import json
import os
import numpy as np
import pytest
import ranks
from ranks import free_port

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_LEVEL, TOL_HIER, RTOL_DT = 1e-9, 1e-8, 1e-10        # tests/test_gpu_dist.py :301, :264 / :283, :259
NSTATE = 5                                               # u v w density tracer: the variables compared across rank counts


# ---------------------------------------------------------------------------------------------------------------- rank processes
def main_ranks(rank, world, ports, jobs, log_dir, group):
    """every rank: R.main once per job, the way `python -m iamr_amd.run` under torchrun calls it; stdout of every call is kept"""
    ranks.rank_env(rank, world)
    ranks.run_jobs(rank, ports, jobs, log_dir, group)


def plot_ranks(rank, world, port, out_dir, owners, merge):
    """case 1: TaylorGreen 16^3 in four 16 x 8 x 8 boxes, viscous, two steps; every rank dumps what level_arrays gives for its boxes, then
    all write the plotfile together.  owners None: run.build deals the boxes (Layout.decompose); a list: that deal, same construction."""
    lib = ranks.start_rank(rank, world, port, merge)
    from iamr_amd import ns as N
    from iamr_amd import run as R
    from iamr_amd.inputs import Inputs
    from iamr_amd.plotfile import DERIVE_NAMES
    inp = Inputs([os.path.join(GOLD, "inputs.3d.taylorgreen")], ["amr.n_cell=16 16 16", "amr.derive_plot_vars=ALL", "ns.vel_visc_coef=0.01"])
    pr = inp.problem()
    pr["max_grid_size"] = (16, 8, 8)
    if owners is None:
        ns, lay, g, pr = R.build(inp, lib, N, world, pr)
    else:
        boxes = lib.Layout.decompose(tuple(pr["n"]), pr["max_grid_size"], 1).boxes
        lay = lib.Layout(boxes, owners)
        g = lib.Geom.make(pr["n"], prob_lo=pr["prob_lo"], prob_hi=pr["prob_hi"], periodic=pr["periodic"])
        ns = N.NavierStokes(g, lay, N.ns_params(**pr["params"]), lib.mg_opts())
        R.init_level(ns, lay, lib, N, pr, pr["n"])
    ns.post_init(pr["stop_time"])
    for _ in range(2):
        ns.step()
    boxes, arrs = R.level_arrays(ns, lay, N, derived=DERIVE_NAMES)
    idx = R.local_indices(lay)
    assert [lay.boxes[q] for q in idx] == boxes and [lay.owners[q] for q in idx] == [rank] * len(idx)
    np.savez(os.path.join(out_dir, f"held_r{rank}.npz"), idx=np.array(idx, dtype=np.int64), boxes=np.array(lay.boxes).reshape(-1, 6),
             owners=np.array(lay.owners), **{f"box{q}": a for q, a in zip(idx, arrs)})
    path = R.write_plot(ns, lay, pr, N, 2, os.path.join(out_dir, "plt"))
    assert path == os.path.join(out_dir, "plt00002")
    ranks.stop_rank()


def allreduce_ranks(rank, world, port, out_dir):
    lib = ranks.start_rank(rank, world, port)
    v = np.array([1.0 + rank, 10.0 * (rank + 1), -3.0 * rank, 7.0, float(rank % 2)])
    if world == 1:
        res = [lib.comm_allreduce(v.copy(), op) for op in (0, 1, 2)]
        lib.comm_barrier()
    else:
        assert lib.comm_rank() == (rank, world)
        res = [lib.comm_allreduce(v.copy(), op) for op in (0, 1, 2)]
        big = lib.comm_allreduce(np.full((40, 11), float(rank + 1)), 0)          # two-dimensional, larger than any solver reduction
        res.append(big.ravel())
        lib.comm_barrier()
        try:
            lib.comm_allreduce(np.zeros(3, dtype=np.float32))
            raise AssertionError("a float32 array was accepted")
        except TypeError:
            pass
    ranks.stop_rank()
    np.savez(os.path.join(out_dir, f"ar_w{world}_r{rank}.npz"), v=v, **{f"op{q}": r for q, r in enumerate(res)})


# ---------------------------------------------------------------------------------------------------------------- reading back
def _log(d, group, job, rank=0):
    return open(os.path.join(d, f"{group}_job{job}_r{rank}.txt")).read()


def _dts(txt):
    return np.array([float(l.split("DT =")[1].split()[0]) for l in txt.splitlines() if l.startswith("STEP =")])


def _only_rank_zero_reports(d, group, world, job, words):
    out0 = _log(d, group, job)
    for w in words:
        assert w in out0, (w, out0[-500:])
    for r in range(1, world):
        o = _log(d, group, job, r)
        assert not [w for w in ("PLOTFILE:", "CHECKPOINT:", "RESTART from", "STEP =") if w in o], (r, o[-500:])


def _state_close(a, b, tol):
    """same grids and names; state variables within tol; returns the largest difference"""
    from iamr_amd.plotfile import PlotFile
    A, B = PlotFile.read(a), PlotFile.read(b)
    assert A.names == B.names and len(A.levels) == len(B.levels) and A.names[:NSTATE] == ["x_velocity", "y_velocity", "z_velocity", "density", "tracer"]
    worst = 0.0
    for l, (la, lb) in enumerate(zip(A.levels, B.levels)):
        assert la.boxes == lb.boxes and la.step == lb.step, l
        for q, (x, y) in enumerate(zip(la.data, lb.data)):
            worst = max(worst, float(np.abs(x[..., :NSTATE] - y[..., :NSTATE]).max()))
    print(f"{os.path.basename(a)} vs {os.path.basename(b)}: max state difference {worst:.3e} (bound {tol:.0e})")
    assert abs(A.time - B.time) <= RTOL_DT * abs(B.time)
    assert worst <= tol, worst
    return worst


def _same_plotfiles(a, b):
    from iamr_amd.plotfile import PlotFile
    A, B = PlotFile.read(a), PlotFile.read(b)
    assert A.names == B.names and len(A.levels) == len(B.levels) and A.time == B.time
    for la, lb in zip(A.levels, B.levels):
        assert la.boxes == lb.boxes and la.step == lb.step
        assert [fn for fn, _ in la.fab_files] == [fn for fn, _ in lb.fab_files]
        for x, y in zip(la.data, lb.data):
            assert np.array_equal(x, y), float(np.abs(x - y).max())


def _data_files(path, level=0):
    return sorted(f for f in os.listdir(os.path.join(path, f"Level_{level}")) if f.startswith("Cell_D_"))


# ---------------------------------------------------------------------------------------------------------------- the grouped runs
HIER = [os.path.join(GOLD, "inputs.3d.tracer_regrid16"), "max_step=6", "amr.plot_int=6"]
TG = [os.path.join(GOLD, "inputs.3d.taylorgreen"), "amr.n_cell=16 16 16", "amr.max_grid_size=8", "max_step=2", "amr.plot_int=2", "amr.derive_plot_vars=ALL",
      "amr.check_int=-1"]


def _full(d, tag):
    return HIER + [f"amr.plot_file={d}/plt{tag}_", f"amr.check_file={d}/chk{tag}_", "amr.check_int=3"]


def _rst(d, tag, frm):
    return HIER + [f"amr.plot_file={d}/plt{tag}_", "amr.check_int=-1", f"amr.restart={d}/chk{frm}_00003"]


def _run_group(d, group, world, jobs):
    ranks.spawn(main_ranks, world, [free_port() for _ in jobs], jobs, d, group)


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("multirank_io"))


@pytest.fixture(scope="module")
def one_rank(out_dir):
    """1 rank: the uninterrupted hierarchy run with its checkpoint (reference of cases 3 to 5), the single-level run (case 2)"""
    _run_group(out_dir, "one", 1, [_full(out_dir, "A"), TG + [f"amr.plot_file={out_dir}/tgA_"]])
    return out_dir


@pytest.fixture(scope="module")
def three_ranks(out_dir):
    _run_group(out_dir, "three", 3, [_full(out_dir, "B")])
    return out_dir


@pytest.fixture(scope="module")
def two_ranks(one_rank):
    """2 ranks: the full run with checkpoints, its restart on 2 ranks, the restart of the 1-rank checkpoint, the single-level run"""
    d = one_rank
    _run_group(d, "two", 2, [_full(d, "C"), _rst(d, "D", "C"), _rst(d, "G", "A"), TG + [f"amr.plot_file={d}/tgI_"]])
    return d


@pytest.fixture(scope="module")
def other_worlds(two_ranks):
    """the 2-rank checkpoint restarted on 3 ranks and on 1 rank"""
    d = two_ranks
    _run_group(d, "rst3", 3, [_rst(d, "F", "C")])
    _run_group(d, "rst1", 1, [_rst(d, "E", "C")])
    return d


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_comm_allreduce(tmp_path):
    """case 6: sum / max / min of rank-dependent vectors on 3 ranks equal numpy's (small integers as doubles: exact); one rank: untouched"""
    d = str(tmp_path)
    ranks.spawn(allreduce_ranks, 3, free_port(), d)
    Z = [np.load(os.path.join(d, f"ar_w3_r{r}.npz")) for r in range(3)]
    V = np.stack([z["v"] for z in Z])
    for z in Z:
        assert np.array_equal(z["op0"], V.sum(axis=0)) and np.array_equal(z["op1"], V.max(axis=0)) and np.array_equal(z["op2"], V.min(axis=0))
        assert np.array_equal(z["op3"], np.full(440, 6.0))
    ranks.spawn(allreduce_ranks, 1, free_port(), d)
    z = np.load(os.path.join(d, "ar_w1_r0.npz"))
    for q in range(3):
        assert np.array_equal(z[f"op{q}"], z["v"])


@pytest.mark.parametrize("world,owners,merge", [(2, None, False), (3, [0, 1, 0, 2], False), (3, None, False), (2, None, True)],
                         ids=["2ranks", "3ranks-2-1-1", "3ranks-one-idle", "2ranks+merge"])
def test_plotfile_equals_what_the_ranks_held(tmp_path, world, owners, merge):
    """case 1 (exact): the plotfile written by all ranks holds, box by box, the arrays the owning rank got from level_arrays -- state and
    derived components -- one Cell_D file per rank that owns boxes, the layout's box list.  "+merge": the library's default box mode
    (two boxes per rank merged inside the level): box list, owners and data still speak the caller's four boxes."""
    from iamr_amd.plotfile import PlotFile, DERIVE_NAMES, state_names
    d = str(tmp_path)
    ranks.spawn(plot_ranks, world, free_port(), d, owners, merge)
    held = [np.load(os.path.join(d, f"held_r{r}.npz")) for r in range(world)]
    own = [int(o) for o in held[0]["owners"]]
    assert own == ([0, 0, 1, 1] if owners is None else owners)
    pf = PlotFile.read(os.path.join(d, "plt00002"))
    assert pf.names == state_names() + DERIVE_NAMES
    lv = pf.levels[0]
    assert _data_files(os.path.join(d, "plt00002")) == [f"Cell_D_{r:05d}" for r in sorted(set(own))]
    assert len(lv.boxes) == 4 and np.array_equal(np.array(lv.boxes).reshape(-1, 6), held[0]["boxes"])
    assert [fn for fn, _ in lv.fab_files] == [f"Cell_D_{o:05d}" for o in own]
    seen = []
    for r in range(world):
        assert np.array_equal(held[r]["boxes"], held[0]["boxes"]) and np.array_equal(held[r]["owners"], held[0]["owners"])
        assert [int(q) for q in held[r]["idx"]] == [q for q, o in enumerate(own) if o == r]
        for q in held[r]["idx"]:
            a = held[r][f"box{q}"]
            assert a.shape == (16, 8, 8, 8) and np.array_equal(lv.data[q], a), (r, int(q))
            seen.append(int(q))
    assert sorted(seen) == [0, 1, 2, 3]
    assert float(np.abs(lv.data[0][..., 0]).max()) > 0.1 and float(np.abs(lv.data[0][..., 6]).max()) > 0.1          # a flow and its vorticity, not zeros


def test_hierarchy_with_regrids_on_three_ranks(one_rank, three_ranks):
    """case 3: tracer_regrid16 (three levels, regrids above level 0), six coarse steps through R.main on 1 and on 3 ranks: same grids on
    every level, state within the hierarchy constant; the owners recorded in the 3-rank checkpoint are the regrid's real ones"""
    from iamr_amd import checkpoint
    d = one_rank
    _only_rank_zero_reports(d, "one", 1, 0, ["PLOTFILE: ", "CHECKPOINT: "])
    _only_rank_zero_reports(d, "three", 3, 0, ["PLOTFILE: " + f"{d}/pltB_00006", "CHECKPOINT: " + f"{d}/chkB_00003"])
    dA, dB = _dts(_log(d, "one", 0)), _dts(_log(d, "three", 0))
    assert len(dA) == len(dB) == 6 and np.allclose(dB, dA, rtol=RTOL_DT, atol=0)
    _state_close(f"{d}/pltB_00006", f"{d}/pltA_00006", TOL_HIER)
    assert _data_files(f"{d}/pltA_00006") == ["Cell_D_00000"]
    hdA, hdB = checkpoint.read_header(f"{d}/chkA_00003"), checkpoint.read_header(f"{d}/chkB_00003")
    assert hdA["boxes"] == hdB["boxes"] and hdB["finest_level"] == 2
    ex = json.load(open(f"{d}/chkB_00003/iamrx_restart.json"))
    assert ex["world"] == 3 and "world" not in json.load(open(f"{d}/chkA_00003/iamrx_restart.json"))
    for l in range(3):
        own = ex["levels"][l]["owners"]
        assert len(own) == len(hdB["boxes"][l]) and all(0 <= o < 3 for o in own)
        names = sorted(f for f in os.listdir(f"{d}/chkB_00003/Level_{l}") if f.startswith("SD_0_New_MF_D_"))
        assert names == [f"SD_0_New_MF_D_{r:05d}" for r in sorted(set(own))]
    assert any(o != 0 for l in (1, 2) for o in ex["levels"][l]["owners"]), [ex["levels"][l]["owners"] for l in range(3)]


def test_run_main_single_level_on_two_ranks(one_rank, two_ranks):
    """case 2: TaylorGreen 16^3 in eight boxes through R.main (IAMRX_RUN_TRANSPORT=gloo) on 1 and on 2 ranks: both write their plotfile,
    same box list and names, state within the single-level constant"""
    from iamr_amd.plotfile import PlotFile, DERIVE_NAMES, state_names
    d = two_ranks
    _only_rank_zero_reports(d, "two", 2, 3, ["PLOTFILE: " + f"{d}/tgI_00002"])
    A, B = PlotFile.read(f"{d}/tgA_00002"), PlotFile.read(f"{d}/tgI_00002")
    assert A.names == B.names == state_names() + DERIVE_NAMES and len(B.levels[0].boxes) == 8 and A.levels[0].boxes == B.levels[0].boxes
    assert _data_files(f"{d}/tgA_00002") == ["Cell_D_00000"] and _data_files(f"{d}/tgI_00002") == ["Cell_D_00000", "Cell_D_00001"]
    assert os.path.exists(f"{d}/tgA_00000/Header") and os.path.exists(f"{d}/tgI_00000/Header")      # the initial plotfile as well
    dA, dI = _dts(_log(d, "one", 1)), _dts(_log(d, "two", 3))
    assert len(dA) == len(dI) == 2 and np.allclose(dI, dA, rtol=RTOL_DT, atol=0)
    _state_close(f"{d}/tgI_00002", f"{d}/tgA_00002", TOL_LEVEL)


def test_checkpoint_and_restart_on_two_ranks(two_ranks):
    """case 4: six steps on 2 ranks with a checkpoint at step 3, restart from it on 2 ranks: the final plotfiles are equal to the bit
    (the promise tests/test_gpu_restart.py holds one rank to), every box back on its recorded owner"""
    d = two_ranks
    _only_rank_zero_reports(d, "two", 2, 1, ["RESTART from", "PLOTFILE: " + f"{d}/pltD_00006"])
    assert len(_dts(_log(d, "two", 0))) == 6 and len(_dts(_log(d, "two", 1))) == 3
    assert json.load(open(f"{d}/chkC_00003/iamrx_restart.json"))["world"] == 2
    _same_plotfiles(f"{d}/pltD_00006", f"{d}/pltC_00006")
    _state_close(f"{d}/pltC_00006", f"{d}/pltA_00006", TOL_HIER)


def test_restart_on_another_number_of_ranks(other_worlds):
    """case 5: the 2-rank checkpoint restarted on 1 and on 3 ranks, the 1-rank checkpoint restarted on 2 ranks; level 1 regrids level 2
    after the restart, so the redeal of restart() is followed by the library's knapsack.  Step 6 within the hierarchy constant of the
    uninterrupted 1-rank run."""
    d = other_worlds
    for group, job, tag in (("rst1", 0, "E"), ("rst3", 0, "F"), ("two", 2, "G")):
        log = _log(d, group, job)
        assert "RESTART from" in log and len(_dts(log)) == 3, (tag, log[-500:])
        _state_close(f"{d}/plt{tag}_00006", f"{d}/pltA_00006", TOL_HIER)
