"""GPU: plane-averaged profiles on two ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py): every rank reduces its own boxes, one all-reduce of the bins follows, every rank receives the result.
The 2-rank profile of the four unequal boxes of tests/test_gpu_profile.py equals the 1-rank profile within the bound of
tests/profile_numpy.py, on every rank.  The two ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import profile_numpy as PN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N2 = (24, 16, 20)


def profile_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    from iamr_amd import ns as N
    from test_gpu_profile import random_state, put_state, as_array
    S = random_state(N2, 9)
    g = L.Geom.make(list(N2), periodic=(1, 1, 1))
    lay = L.Layout.decompose(N2, 16, world)
    assert sorted(set(lay.owners)) == list(range(world))
    ns = N.NavierStokes(g, lay, N.ns_params())
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    np.savez(os.path.join(out_dir, f"prof_w{world}_r{rank}.npz"), **{f"d{d}": as_array(ns.plane_profile(d)) for d in range(3)})
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank profile is taken in this process (the same four boxes, kept as boxes), the 2-rank one by two child processes"""
    from test_gpu_profile import random_state, one_level, as_array
    d = str(tmp_path)
    ranks.spawn(profile_ranks, 2, ranks.free_port(), d)
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
