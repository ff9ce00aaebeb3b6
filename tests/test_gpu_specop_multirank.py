"""GPU: a filter and a synthesis on two ranks (ranks sharing the one GPU over the gloo callback transport: tests/ranks.py).  The source
field is gathered as the spectra gather it, every rank transforms the whole field and unpacks into its own boxes; the noise of the
synthesis needs no gather at all.  The field assembled from the two ranks has the bits of the one-rank call.  The two ranks are fresh
child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import spectrum_numpy as SN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N3 = (16, 16, 16)


def fields(L, lay):
    """(filtered noise (n, 2), synthesised velocity (n, 3)): the valid cells of THIS rank's boxes, zero elsewhere"""
    from test_gpu_budget_multirank import pair_mf
    from iamr_amd.spectral import hit_spectrum
    from iamr_amd.spectrum import nbins_of
    g = L.Geom.make(list(N3), periodic=(1, 1, 1))
    src = pair_mf(L, lay, SN.noise(N3, 7, 2))
    dst = pair_mf(L, lay, np.full(N3 + (2,), np.nan))
    L.mf_filter(g, dst, src, "gaussian", 3.0, ncomp=2)
    vel = L.MultiFab(lay, L.CELL, 3, 1)
    L.mf_synthesize(g, vel, hit_spectrum(nbins_of(N3, (1.0, 1.0, 1.0)), (1.0, 1.0, 1.0), 3.0, 1.0, n=N3), seed=42, wavenumber="centred")
    return dst.gather_valid(N3), vel.gather_valid(N3)


def specop_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    lay = L.Layout.decompose(N3, 8, world)
    assert sorted(set(lay.owners)) == list(range(world)) and lay.nlocal() == 8 // world
    filt, vel = fields(L, lay)
    np.savez(os.path.join(out_dir, f"specop_w{world}_r{rank}.npz"), filt=filt, vel=vel)
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank fields are made in this process (the same eight boxes), the 2-rank ones by two child processes; a cell has one owner,
    so the sum of the two ranks' arrays (zero outside their boxes) assembles the field exactly"""
    d = str(tmp_path)
    ranks.spawn(specop_ranks, 2, ranks.free_port(), d)
    two = [np.load(os.path.join(d, f"specop_w2_r{r}.npz")) for r in range(2)]
    lay = gpu.Layout.decompose(N3, 8)
    assert len(lay.boxes) == 8
    one = dict(zip(("filt", "vel"), fields(gpu, lay)))
    for k, v in one.items():
        a, b = two[0][k], two[1][k]
        assert a.any() and b.any() and not np.any((a != 0.0) & (b != 0.0)), k         # both ranks own cells, no cell twice
        assert not np.isnan(v).any() and (a + b).tobytes() == v.tobytes(), k
