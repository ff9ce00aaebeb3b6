"""GPU: velocity statistics and integrated quantities of runs on several ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py).  An N-rank run against the 1-rank run uses that file's constants (single level: 1e-9;
a checkpoint restarted on another number of ranks: 1e-8); the integrated quantities, summed over the ranks through the communicator's
host all-reduce, are also held to the rounding bound of tests/test_gpu_stats.py against numpy on the state the checkpoint holds."""
import json
import os
import numpy as np
import pytest
import ranks
from ranks import free_port
from test_gpu_multirank_io import _log, _dts, TOL_LEVEL, TOL_HIER, RTOL_DT
from test_gpu_stats import composite_sums

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS16 = os.path.join(ROOT, "tests", "golden", "inputs.3d.taylorgreen_stats16")
N16 = [16, 16, 16]


def stats_ranks(rank, world, ports, jobs, log_dir, group):
    """every rank: R.main once per job with an observer that records the integrated quantities (full doubles) and the three scalars"""
    ranks.rank_env(rank, world)
    rec = []

    def observe(ns, step, dt):
        rec.append(dict(step=step, time=ns.time, sums=list(ns.sum_integrated()), avg=list(ns.average_state)))      # collective

    def after(q):
        with open(os.path.join(log_dir, f"{group}_job{q}_r{rank}.json"), "w") as f:
            json.dump(rec, f)
        rec.clear()

    ranks.run_jobs(rank, ports, jobs, log_dir, group, observe, after)


def _job(d, tag, *more):
    return [STATS16, "amr.plot_int=-1", "amr.check_int=2", f"amr.check_file={d}/chk{tag}_"] + list(more)


def _rec(d, group, job, rank=0):
    return json.load(open(os.path.join(d, f"{group}_job{job}_r{rank}.json")))


def _gathered(path, name, typ_ng=0):
    """a checkpointed cell MultiFab of level 0 as one array over the domain (valid cells)"""
    from iamr_amd import checkpoint
    hd = checkpoint.read_header(path)
    fabs = checkpoint._read_vismf(os.path.join(path, "Level_0"), name)
    G = np.zeros(tuple(N16) + (fabs[0].shape[-1],))
    for (lo, hi), a in zip(hd["boxes"][0], fabs):
        ng = typ_ng
        v = a[ng:a.shape[0] - ng, ng:a.shape[1] - ng, ng:a.shape[2] - ng] if ng else a
        G[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = v
    return G


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stats_multirank"))
    # four spawns in one fixture (measured 2.4, 2.9, 2.5 and 3.2 s): four times the helper's 120 s would pass the 420 s after which pytest-timeout
    # takes the whole test, so each gets 100 s -- the helper fires first, and ends its ranks
    lim = 100.0
    one = [_job(d, "A")]
    two = [_job(d, "B")]
    ranks.spawn(stats_ranks, 1, [free_port() for _ in one], one, d, "one", limit=lim)
    ranks.spawn(stats_ranks, 2, [free_port() for _ in two], two, d, "two", limit=lim)
    rst = [_job(d, "C", f"amr.restart={d}/chkB_00002")]
    ranks.spawn(stats_ranks, 1, [free_port()], rst, d, "rst1", limit=lim)
    rst3 = [_job(d, "D", f"amr.restart={d}/chkB_00002")]
    ranks.spawn(stats_ranks, 3, [free_port()], rst3, d, "rst3", limit=lim)
    return d


def test_two_ranks_against_one(runs):
    """eight 8^3 boxes on 2 ranks vs 1 rank, 4 steps: state and accumulators within the single-level constant, the scalars at the dts'
    relative tolerance, the sums within the constant and -- every rank holding the same doubles -- within the rounding bound of numpy on
    the checkpointed state; only rank 0 prints the three lines"""
    d = runs
    assert json.load(open(f"{d}/chkB_00004/iamrx_restart.json"))["world"] == 2
    assert sorted(f for f in os.listdir(f"{d}/chkB_00004/Level_0") if f.startswith("SD_3")) == ["SD_3_New_MF_D_00000", "SD_3_New_MF_D_00001", "SD_3_New_MF_H"]
    dA, dB = _dts(_log(d, "one", 0)), _dts(_log(d, "two", 0))
    assert len(dA) == len(dB) == 4 and np.allclose(dB, dA, rtol=RTOL_DT, atol=0)
    SA, SB = _gathered(f"{d}/chkA_00004", "SD_0_New_MF", 1), _gathered(f"{d}/chkB_00004", "SD_0_New_MF", 1)
    AA, AB = _gathered(f"{d}/chkA_00004", "SD_3_New_MF"), _gathered(f"{d}/chkB_00004", "SD_3_New_MF")
    es, ea = float(np.abs(SA - SB).max()), float(np.abs(AA - AB).max())
    print(f"2 ranks vs 1: state {es:.3e}, accumulators {ea:.3e} (bound {TOL_LEVEL:.0e})")
    assert float(np.abs(AA).max()) > 1e-3 and es <= TOL_LEVEL and ea <= TOL_LEVEL
    rA, rB0, rB1 = _rec(d, "one", 0), _rec(d, "two", 0, 0), _rec(d, "two", 0, 1)
    assert [r["step"] for r in rA] == [r["step"] for r in rB0] == [0, 1, 2, 3, 4]
    assert rB0 == rB1                                                         # the all-reduce leaves the same doubles on every rank
    for a, b in zip(rA, rB0):
        assert np.allclose(b["avg"], a["avg"], rtol=RTOL_DT, atol=0)
        assert float(np.abs(np.array(a["sums"]) - np.array(b["sums"])).max()) <= TOL_LEVEL
    want, bound = composite_sums([SB], [np.ones(N16, dtype=bool)], [[1.0 / 16] * 3])
    got = np.array(rB0[-1]["sums"])
    print(f"2-rank sums {got}, |diff to numpy| {np.abs(got - want)}, bound {bound}")
    assert np.all(np.abs(got - want) <= bound)
    assert _log(d, "two", 0, 0).count(" MASS= ") == 5 and "TIME= " not in _log(d, "two", 0, 1)


@pytest.mark.parametrize("group,tag", [("rst1", "C"), ("rst3", "D")])
def test_restart_on_another_number_of_ranks(runs, group, tag):
    """the 2-rank checkpoint of step 2 restarted on 1 and on 3 ranks and continued to step 4: accumulators, state and scalars within the
    other-world constant of the uninterrupted 1-rank run"""
    from iamr_amd import checkpoint
    d = runs
    log = _log(d, group, 0)
    assert "RESTART from" in log and len(_dts(log)) == 2
    ref, got = f"{d}/chkA_00004", f"{d}/chk{tag}_00004"
    es = float(np.abs(_gathered(ref, "SD_0_New_MF", 1) - _gathered(got, "SD_0_New_MF", 1)).max())
    ea = float(np.abs(_gathered(ref, "SD_3_New_MF") - _gathered(got, "SD_3_New_MF")).max())
    print(f"{group}: state {es:.3e}, accumulators {ea:.3e} (bound {TOL_HIER:.0e})")
    assert es <= TOL_HIER and ea <= TOL_HIER
    assert np.allclose(checkpoint.read_time_average(got), checkpoint.read_time_average(ref), rtol=RTOL_DT, atol=0)
    if group == "rst3":
        assert json.load(open(f"{got}/iamrx_restart.json"))["world"] == 3
