"""GPU: histograms on two and three ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py): every rank counts its own boxes, one all-reduce of the slots follows (doubles that hold integers
below 2^53: exact), every rank receives the result.  The histogram of (24, 16, 20) cut at 16 into four unequal boxes equals the 1-rank
result to the bit, on every rank.  The ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import hist_numpy as HN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N2 = (24, 16, 20)
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
    L = ranks.start_rank(rank, world, port)
    from iamr_amd import ns as N
    from test_gpu_profile import random_state, put_state
    S = random_state(N2, 9)
    g = L.Geom.make(list(N2), periodic=(1, 1, 1))
    boxes = L.Layout.decompose(N2, 16).boxes
    lay = L.Layout(boxes, [q % world for q in range(len(boxes))])          # four boxes: every rank owns at least one
    assert sorted(set(lay.owners)) == list(range(world))
    ns = N.NavierStokes(g, lay, N.ns_params())
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    np.savez(os.path.join(out_dir, f"hist_w{world}_r{rank}.npz"), **results(ns))
    ranks.stop_rank()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_against_one(gpu, tmp_path, world):
    """the 1-rank histogram is taken in this process (the same four boxes, kept as boxes), the others by fresh child processes"""
    from test_gpu_profile import random_state, one_level
    d = str(tmp_path)
    ranks.spawn(hist_ranks, world, ranks.free_port(), d)
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
