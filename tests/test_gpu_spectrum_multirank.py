"""GPU: shell-summed spectra on two ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py): every rank writes the cells of its own boxes into a zeroed array, the arrays are summed (exact:
a cell has one owner), every rank transforms the whole field.  Both ranks return identical bytes, and those bytes are the one-rank
result to the bit.  The two ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import spectrum_numpy as SN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N3 = (32, 32, 32)


def spectrum_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    f = SN.noise(N3, 7, 2)
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
    P, count = L.mf_spectrum(g, mf, 0, 2)
    np.savez(os.path.join(out_dir, f"spec_w{world}_r{rank}.npz"), P=P, count=count)
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank spectrum is taken in this process (the same eight boxes), the 2-rank one by two child processes"""
    from test_gpu_spectrum import make_mf, geom_of, check
    d = str(tmp_path)
    ranks.spawn(spectrum_ranks, 2, ranks.free_port(), d)
    two = [np.load(os.path.join(d, f"spec_w2_r{r}.npz")) for r in range(2)]
    f = SN.noise(N3, 7, 2)
    mf, lay = make_mf(N3, f, 16)
    assert len(lay.boxes) == 8
    P, count = gpu.mf_spectrum(geom_of(N3), mf, 0, 2)
    for q in range(2):
        check(P[q], SN.spectrum_reference(f[..., q], (1.0, 1.0, 1.0)), f[..., q].size, f"one rank, component {q}")
    assert two[0]["P"].tobytes() == two[1]["P"].tobytes() and np.array_equal(two[0]["count"], two[1]["count"])      # every rank: the same bytes
    assert two[0]["P"].tobytes() == P.tobytes() and np.array_equal(two[0]["count"], count)                           # ... and the one-rank bytes
