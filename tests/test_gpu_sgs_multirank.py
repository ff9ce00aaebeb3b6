"""GPU: the a-priori LES analysis on two ranks (ranks sharing the one GPU over the gloo callback transport: tests/ranks.py).  The velocity
and the six products are gathered as the spectra gather a field -- zeroed image, pack, exact all-reduce -- every rank filters the whole
images and unpacks into its own boxes.  Both ranks return the statistics of the one-rank call to the bit, and the fields assembled from
the two ranks have its bits.  The two ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import specop_numpy as SO

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N3 = (8, 16, 32)
FIELDS = ("tau_xy", "k_sgs", "sgs_flux", "filtered_strain", "smag_flux")


def analysis(L, lay):
    """(statistics (16,), counts (2,), the fields on the valid cells of THIS rank's boxes, zero elsewhere)"""
    f = SO.noise(N3, 21, 3) * 2.0 + np.array([0.3, -0.2, 0.1])
    vel = L.MultiFab(lay, L.CELL, 3, 1)
    for li in range(vel.nlocal()):
        glo, ghi = vel.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (3,), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        vel.from_numpy(a, li)
    r = L.mf_sgs(L.Geom.make(list(N3), periodic=(1, 1, 1)), vel, "gaussian", 3.0, FIELDS)
    return r["stats"], np.array([r["N"], r["negative_cells"]], dtype=np.int64), r["fields"].gather_valid(N3)


def sgs_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    lay = L.Layout.decompose(N3, 8, world)
    assert sorted(set(lay.owners)) == list(range(world)) and lay.nlocal() == 8 // world
    stats, counts, F = analysis(L, lay)
    np.savez(os.path.join(out_dir, f"sgs_w{world}_r{rank}.npz"), stats=stats, counts=counts, F=F)
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank result is made in this process (the same eight boxes), the 2-rank ones by two child processes; a cell has one owner, so
    the sum of the two ranks' field arrays (zero outside their boxes) assembles the fields exactly"""
    d = str(tmp_path)
    ranks.spawn(sgs_ranks, 2, ranks.free_port(), d)
    two = [np.load(os.path.join(d, f"sgs_w2_r{r}.npz")) for r in range(2)]
    lay = gpu.Layout.decompose(N3, 8)
    assert len(lay.boxes) == 8
    stats, counts, F = analysis(gpu, lay)
    assert np.all(np.isfinite(stats)) and stats[3] > 0.0 and 0 < counts[1] < counts[0] == 8 * 16 * 32
    for r in range(2):
        assert two[r]["stats"].tobytes() == stats.tobytes(), r
        assert two[r]["counts"].tolist() == counts.tolist(), r
    a, b = two[0]["F"], two[1]["F"]
    assert a.any() and b.any() and not np.any((a != 0.0) & (b != 0.0))          # both ranks own cells, no cell twice
    assert not np.isnan(F).any() and (a + b).tobytes() == F.tobytes()
