"""GPU: a co-spectrum and the spectral budget on two ranks (ranks sharing the one GPU over the gloo callback transport: tests/ranks.py).
Every rank writes the cells of its own boxes of both fields into zeroed arrays, the arrays are summed (exact: a cell has one owner)
and interleaved, every rank transforms the whole pair.  Both ranks return identical bytes, and those bytes are the one-rank result to the
bit.  The two ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import spectrum_numpy as SN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N3 = (16, 16, 16)
COLS = ("E", "T", "Pi", "D", "F", "count")


def level_of(L, lay, S):
    from iamr_amd import ns as N
    from test_gpu_profile import put_state
    ns = N.NavierStokes(L.Geom.make(list(N3), periodic=(1, 1, 1)), lay, N.ns_params(visc_coef=0.01))
    ns.init_rest(1.0)
    put_state(ns, lay, S)
    return ns


def pair_mf(L, lay, f):
    mf = L.MultiFab(lay, L.CELL, 2, 1)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (2,), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    return mf


def budget_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    from test_gpu_profile import random_state
    lay = L.Layout.decompose(N3, 8, world)
    assert sorted(set(lay.owners)) == list(range(world)) and lay.nlocal() == 8 // world
    mf = pair_mf(L, lay, SN.noise(N3, 7, 2))
    Cab, Pa, Pb, count = L.mf_cospectrum(L.Geom.make(list(N3), periodic=(1, 1, 1)), mf, mf, 0, 1)
    s = level_of(L, lay, random_state(N3, 12)).spectral_budget()
    np.savez(os.path.join(out_dir, f"bud_w{world}_r{rank}.npz"), Cab=Cab, Pa=Pa, Pb=Pb, cnt=count, **{c: s[c] for c in COLS})
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank results are taken in this process (the same eight boxes), the 2-rank ones by two child processes"""
    from test_gpu_profile import random_state
    d = str(tmp_path)
    ranks.spawn(budget_ranks, 2, ranks.free_port(), d)
    two = [np.load(os.path.join(d, f"bud_w2_r{r}.npz")) for r in range(2)]
    lay = gpu.Layout.decompose(N3, 8)
    assert len(lay.boxes) == 8
    mf = pair_mf(gpu, lay, SN.noise(N3, 7, 2))
    Cab, Pa, Pb, count = gpu.mf_cospectrum(gpu.Geom.make(list(N3), periodic=(1, 1, 1)), mf, mf, 0, 1)
    s = level_of(gpu, lay, random_state(N3, 12)).spectral_budget()
    one = dict(Cab=Cab, Pa=Pa, Pb=Pb, cnt=count, **{c: s[c] for c in COLS})
    assert Cab.any() and s["T"].any() and s["D"].any()
    for k, v in one.items():
        assert two[0][k].tobytes() == two[1][k].tobytes(), k          # every rank: the same bytes
        assert two[0][k].tobytes() == v.tobytes(), k                   # ... and the one-rank bytes
