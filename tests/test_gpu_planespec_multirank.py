"""GPU: plane spectra on two ranks (ranks sharing the one GPU over the gloo callback transport: tests/ranks.py).  The boxes of one shape
per direction are split between the ranks; every rank packs its own boxes, the arrays are summed (exact: a cell has one owner) and every
rank transforms the whole field: both ranks return the bytes of the one-rank call, with SPECTRUM_DIST = 1 as without it (these calls
stay on the gather).  The two ranks are fresh child processes under a time limit of their own."""
import os
import numpy as np
import pytest
import ranks
import planespec_numpy as PS

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
SHAPES = (((8, 16, 6), PS.U3, 2), ((8, 6, 16), PS.U3, 1), ((6, 8, 16), PS.U3, 0))


def plane_ranks(rank, world, port, out_dir):
    from test_gpu_planespec import unequal_boxes
    L = ranks.start_rank(rank, world, port)
    res = {}
    for dist in (0, 1):
        L.tuning_set("SPECTRUM_DIST", dist)
        for n, Ls, dir in SHAPES:
            f = PS.noise(n, 7, 2)
            g = L.Geom.make(list(n), prob_hi=Ls, periodic=(1, 1, 1))
            boxes = unequal_boxes(n)
            lay = L.Layout(boxes, [q % world for q in range(len(boxes))])
            assert lay.nlocal() == len(boxes) // world
            mf = L.MultiFab(lay, L.CELL, 2, 1)
            for li in range(mf.nlocal()):
                glo, ghi = mf.fab_box(li)
                lo, hi, _ = lay.local_box(li)
                a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (2,), np.nan, order="F")
                a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
                mf.from_numpy(a, li)
            P, count = L.mf_plane_spectrum(g, mf, dir, 0, 2)
            Cab = L.mf_plane_cospectrum(g, mf, mf, dir, 0, 1)[0]
            res[f"P{dir}_{dist}"], res[f"c{dir}_{dist}"], res[f"C{dir}_{dist}"] = P, count, Cab
    L.tuning_set("SPECTRUM_DIST", 0)
    np.savez(os.path.join(out_dir, f"pspec_w{world}_r{rank}.npz"), **res)
    ranks.stop_rank()


def test_two_ranks_against_one(gpu, tmp_path):
    """the 1-rank plane spectra are taken in this process (the same boxes), the 2-rank ones by two child processes"""
    from test_gpu_planespec import make_mf, geom_of, check, unequal_boxes, plane_count
    d = str(tmp_path)
    ranks.spawn(plane_ranks, 2, ranks.free_port(), d)
    two = [np.load(os.path.join(d, f"pspec_w2_r{r}.npz")) for r in range(2)]
    for n, Ls, dir in SHAPES:
        f = PS.noise(n, 7, 2)
        mf, lay = make_mf(n, f, unequal_boxes(n))
        g = geom_of(n, Ls)
        P, count = gpu.mf_plane_spectrum(g, mf, dir, 0, 2)
        Cab = gpu.mf_plane_cospectrum(g, mf, mf, dir, 0, 1)[0]
        for q in range(2):
            check(P[q], PS.plane_spectrum_reference(f[..., q], Ls, dir), plane_count(n, dir), f"one rank, dir {dir}, component {q}")
        for dist in (0, 1):
            for r in range(2):
                assert two[r][f"P{dir}_{dist}"].tobytes() == P.tobytes(), (dir, dist, r)
                assert np.array_equal(two[r][f"c{dir}_{dist}"], count) and two[r][f"C{dir}_{dist}"].tobytes() == Cab.tobytes(), (dir, dist, r)
