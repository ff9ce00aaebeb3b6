"""GPU: histograms on two and three ranks (ranks sharing the one GPU over the gloo callback transport, the harness of
tests/test_gpu_profile_multirank.py): every rank counts its own boxes, one all-reduce of the slots follows (doubles that hold integers
below 2^53: exact), every rank receives the result.  The histogram of (24, 16, 20) cut at 16 into four unequal boxes equals the 1-rank
result to the bit, on every rank.  The ranks are fresh child processes under a time limit of their own."""
import os
import time
import numpy as np
import pytest
from test_gpu_dist import free_port
from test_gpu_multirank_io import _env
import hist_numpy as HN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N2 = (24, 16, 20)
LIMIT = 120.0          # seconds for the ranks of one run
NAMES = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer", "energy"]
RANGES = [(-0.5, 1.0), (-1.2, 0.8), (-0.9, 1.1), (0.75, 2.0), (-0.5, 1.6), (0.05, 2.0)]
NBINS = 48
JOINT = dict(nbins=(7, 12), range=((-0.5, 1.0), (0.75, 2.0)))


def results(ns):
    from test_gpu_hist import slots
    h = ns.histogram(NAMES, NBINS, RANGES)
    h2 = ns.histogram2("x_velocity", "density", **JOINT)
    auto = ns.histogram(["tracer", "energy"], 16)
    return dict(slots=slots(h), joint=h2["counts"], outside=np.int64(h2["outside"]), auto=slots(auto), auto_range=auto["range"])


def hist_ranks(rank, world, port, out_dir):
    _env(rank, world)
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import comm
    from test_gpu_profile import random_state, put_state
    import torch.distributed as dist
    L.init(0)
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm.init_gloo_callback(dist)
    S = random_state(N2, 9)
    g = L.Geom.make(list(N2), periodic=(1, 1, 1))
    boxes = L.Layout.decompose(N2, 16).boxes
    lay = L.Layout(boxes, [q % world for q in range(len(boxes))])          # four boxes: every rank owns at least one
    assert sorted(set(lay.owners)) == list(range(world))
    ns = N.NavierStokes(g, lay, N.ns_params())
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    np.savez(os.path.join(out_dir, f"hist_w{world}_r{rank}.npz"), **results(ns))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, *args):
    import torch.multiprocessing as mp
    ctx = mp.spawn(hist_ranks, args=(world,) + args, nprocs=world, join=False)
    end = time.monotonic() + LIMIT
    while not ctx.join(timeout=1.0):
        if time.monotonic() > end:
            for p in ctx.processes:
                p.kill()
            raise AssertionError(f"{world} rank(s) did not finish within {LIMIT:.0f} s")


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_against_one(gpu, tmp_path, world):
    """the 1-rank histogram is taken in this process (the same four boxes, kept as boxes), the others by fresh child processes"""
    from test_gpu_profile import random_state, one_level
    d = str(tmp_path)
    _spawn(world, free_port(), d)
    got = [np.load(os.path.join(d, f"hist_w{world}_r{r}.npz")) for r in range(world)]
    S = random_state(N2, 9)
    ns, lay = one_level(N2, S, 16)
    assert len(lay.boxes) == 4
    one = results(ns)
    ref = HN.hist_reference([S], [lay.boxes], list(N2), [r[0] for r in RANGES[:5]], [r[1] for r in RANGES[:5]], NBINS)
    assert np.array_equal(one["slots"][:5], ref) and one["slots"][5].sum() == N2[0] * N2[1] * N2[2]
    for r in range(world):
        for k, v in one.items():
            a = got[r][k]
            assert a.dtype == np.asarray(v).dtype and a.tobytes() == np.asarray(v).tobytes(), (r, k)
