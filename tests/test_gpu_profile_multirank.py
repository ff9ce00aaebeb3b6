"""GPU: plane-averaged profiles on two ranks (ranks sharing the one GPU over the gloo callback transport, the harness of
tests/test_gpu_multirank_io.py): every rank reduces its own boxes, one all-reduce of the bins follows, every rank receives the result.
The 2-rank profile of the four unequal boxes of tests/test_gpu_profile.py equals the 1-rank profile within the bound of
tests/profile_numpy.py, on every rank.  The two ranks are fresh child processes under a time limit of their own."""
import os
import time
import numpy as np
import pytest
from test_gpu_dist import free_port
from test_gpu_multirank_io import _env
import profile_numpy as PN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N2 = (24, 16, 20)
LIMIT = 120.0          # seconds for the two ranks


def profile_ranks(rank, world, port, out_dir):
    _env(rank, world)
    from iamr_amd import lib as L
    from iamr_amd import ns as N
    from iamr_amd import comm
    from test_gpu_profile import random_state, put_state, as_array
    import torch.distributed as dist
    L.init(0)
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm.init_gloo_callback(dist)
    S = random_state(N2, 9)
    g = L.Geom.make(list(N2), periodic=(1, 1, 1))
    lay = L.Layout.decompose(N2, 16, world)
    assert sorted(set(lay.owners)) == list(range(world))
    ns = N.NavierStokes(g, lay, N.ns_params())
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    np.savez(os.path.join(out_dir, f"prof_w{world}_r{rank}.npz"), **{f"d{d}": as_array(ns.plane_profile(d)) for d in range(3)})
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, *args):
    import torch.multiprocessing as mp
    ctx = mp.spawn(profile_ranks, args=(world,) + args, nprocs=world, join=False)
    end = time.monotonic() + LIMIT
    while not ctx.join(timeout=1.0):
        if time.monotonic() > end:
            for p in ctx.processes:
                p.kill()
            raise AssertionError(f"{world} rank(s) did not finish within {LIMIT:.0f} s")


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank profile is taken in this process (the same four boxes, kept as boxes), the 2-rank one by two child processes"""
    from test_gpu_profile import random_state, one_level, as_array
    d = str(tmp_path)
    _spawn(2, free_port(), d)
    two = [np.load(os.path.join(d, f"prof_w2_r{r}.npz")) for r in range(2)]
    S = random_state(N2, 9)
    ns, lay = one_level(N2, S, 16)
    assert len(lay.boxes) == 4
    for q in range(3):
        mean, N, meanabs = PN.profile_reference([S], [lay.boxes], list(N2), q, 0)
        bd = PN.bound(N, meanabs)
        a = as_array(ns.plane_profile(q))
        assert np.all(np.abs(a - mean) <= bd)
        assert two[0][f"d{q}"].tobytes() == two[1][f"d{q}"].tobytes()            # every rank receives the same doubles
        for r in range(2):
            e1, e2 = np.abs(two[r][f"d{q}"] - a), np.abs(two[r][f"d{q}"] - mean)
            print(f"dir {q} rank {r}: max |2 ranks - 1 rank| / bound = {float(np.max(e1 / bd)):.3f}, |2 ranks - fsum| / bound = {float(np.max(e2 / bd)):.3f}")
            assert np.all(e1 <= bd) and np.all(e2 <= bd)
