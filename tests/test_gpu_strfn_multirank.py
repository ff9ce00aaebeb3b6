"""GPU: structure functions on two ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py): every rank writes the cells of its own boxes into a zeroed array, the arrays are summed (exact:
a cell has one owner), every rank runs the pair launches on the whole field.  Both ranks return identical bytes, and those bytes are
the one-rank result to the bit.  The two ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import strfn_numpy as SF

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N3 = (32, 32, 32)


def strfn_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    f = SF.noise(N3, 7, 2)
    g = L.Geom.make(list(N3), periodic=(1, 1, 1))
    lay = L.Layout.decompose(N3, 16, world)
    assert sorted(set(lay.owners)) == list(range(world)) and lay.nlocal() == 8 // world
    mf = L.MultiFab(lay, L.CELL, 2, 1)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (2,), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    s = L.mf_structure(g, mf, 0, 2)
    np.savez(os.path.join(out_dir, f"sf_w{world}_r{rank}.npz"), avg=s["avg"], count=s["count"], mean=s["mean"])
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank result is taken in this process (the same eight boxes), the 2-rank one by two child processes"""
    from test_gpu_spectrum import make_mf, geom_of
    from test_gpu_strfn import reference, check, PER
    d = str(tmp_path)
    ranks.spawn(strfn_ranks, 2, ranks.free_port(), d)
    two = [np.load(os.path.join(d, f"sf_w2_r{r}.npz")) for r in range(2)]
    f, refs = reference(N3, PER, 4, (-1, -1, -1), 7, 2)
    mf, lay = make_mf(N3, f, 16)
    assert len(lay.boxes) == 8
    s = gpu.mf_structure(geom_of(N3), mf, 0, 2)
    for q in range(2):
        check(s, refs[q], q, f"one rank, component {q}", f[..., q])
    for k in ("avg", "count", "mean"):
        assert two[0][k].tobytes() == two[1][k].tobytes(), k          # every rank: the same bytes
        assert two[0][k].tobytes() == s[k].tobytes(), k               # ... and the one-rank bytes
