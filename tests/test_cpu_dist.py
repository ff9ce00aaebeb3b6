"""CPU suite: the N > 1 path on gloo (world size 2, and 8 for the layout of bench.py --gpus 8).

The boxes of a level are split over two ranks; every ghost exchange is driven by the PRODUCT's host-side
planner (iamrx_host_fill_plan: local copies + packed peer messages) with torch.distributed(gloo) as the
transport, while the oracle supplies the per-box arithmetic (red-black Gauss-Seidel).  The distributed result
must be bit-identical to the single-box, single-rank sweep: this checks partitioning, message
matching/ordering and periodic images exactly as the RCCL path uses them."""
import ctypes as C
import os
import sys
import numpy as np
import pytest
import ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (16, 8, 8)
BOXES = [((i0, 0, 0), (i0 + 3, 7, 7)) for i0 in (0, 4, 8, 12)]
OWNERS = [0, 0, 1, 1]
NSWEEP = 3


def bench_layout(world, n=8):
    """the layout bench.py builds for `world` GPUs (proc_grid: rows never cut, y and z split), one n^3 box per rank"""
    sys.path.insert(0, ROOT)
    import bench
    pg = bench.proc_grid(world)
    boxes = []
    for r in range(world):
        ix, iy, iz = r % pg[0], (r // pg[0]) % pg[1], r // (pg[0] * pg[1])
        boxes.append(((n * ix, n * iy, n * iz), (n * ix + n - 1, n * iy + n - 1, n * iz + n - 1)))
    return tuple(n * pg[d] for d in range(3)), boxes, list(range(world))


def layout(case):
    """(domain, boxes, owners): "x4" = four slabs in x on two ranks; "bench8" = bench.py's 8-GPU layout, one box per rank"""
    return bench_layout(8) if case == "bench8" else (N, BOXES, OWNERS)


def global_fields(N=N):
    rng = np.random.default_rng(42)
    phi = rng.standard_normal(N)
    rhs = rng.standard_normal(N)
    b = []
    for d in range(3):
        shp = list(N)
        shp[d] += 1
        f = 1.0 + 0.5 * rng.random(shp)
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[d] = N[d]
        lo[d] = 0
        f[tuple(hi)] = f[tuple(lo)]        # periodic duplicate face
        b.append(f)
    return phi, rhs, b


def reference_single_box(orc, N=N):
    L = orc.lib()
    g = orc.geom(N)
    phi0, rhs0, b0 = global_fields(N)
    b = []
    for d in range(3):
        f = orc.Fab(N, orc.face(d), 0, 1)
        f.a[..., 0] = b0[d]
        b.append(f)
    lev = orc.abec_level(g, b)
    phi = orc.Fab(N, orc.CELL, 1, 1)
    phi.valid(N)[..., 0] = phi0
    rhs = orc.Fab(N, orc.CELL, 0, 1)
    rhs.a[..., 0] = rhs0
    z = orc.i3([0, 0, 0])
    for _ in range(NSWEEP):
        for rb in (0, 1):
            L.orc_fill_periodic(phi.ref(), C.byref(g), orc.i3(orc.CELL))
            L.orc_abec_gsrb(C.byref(lev), phi.ref(), rhs.ref(), rb, C.c_double(1.15), z, z, 3)
    return phi.valid(N)[..., 0].copy()


def worker(rank, world, port, out_dir, case="x4"):
    ranks.rank_env(rank, world, port)
    import torch
    import torch.distributed as dist
    import orc
    from iamr_amd import lib
    from test_cpu_abi import host_plan
    dist.init_process_group("gloo", rank=rank, world_size=world)
    L = orc.lib()
    N, BOXES, OWNERS = layout(case)
    geom = lib.Geom.make(N)
    desc = host_plan(lib, BOXES, OWNERS, rank, (0, 0, 0), 1, geom)
    phi0, rhs0, b0 = global_fields(N)
    mine = [i for i, o in enumerate(OWNERS) if o == rank]
    fabs, levs, keep = {}, {}, []
    for bi in mine:
        lo, hi = BOXES[bi]
        bn = tuple(hi[d] - lo[d] + 1 for d in range(3))
        bg = orc.geom(bn, periodic=(0, 0, 0))
        bg.dx = (C.c_double * 3)(*[1.0 / N[d] for d in range(3)])
        bf = []
        for d in range(3):
            f = orc.Fab(bn, orc.face(d), 0, 1)
            sl = tuple(slice(lo[q], hi[q] + 1 + (1 if q == d else 0)) for q in range(3))
            f.a[..., 0] = b0[d][sl]
            bf.append(f)
        phi = orc.Fab(bn, orc.CELL, 1, 1)
        sl = tuple(slice(lo[q], hi[q] + 1) for q in range(3))
        phi.valid(bn)[..., 0] = phi0[sl]
        rhs = orc.Fab(bn, orc.CELL, 0, 1)
        rhs.a[..., 0] = rhs0[sl]
        fabs[bi] = (phi, rhs, bn, lo)
        levs[bi] = (orc.abec_level(bg, bf), bg)
        keep.append(bf)

    def region_view(bi, lo_, hi_, shift=(0, 0, 0)):
        phi, _, bn, blo = fabs[bi]
        # fab array origin (global index) = blo - 1
        return tuple(slice(lo_[q] + shift[q] - (blo[q] - 1), hi_[q] + shift[q] - (blo[q] - 1) + 1) for q in range(3))

    def exchange():
        # pack + send / recv + unpack, then local copies (product order: execute_plan)
        peers = sorted(set(int(d[1]) for d in desc if d[0] != 0))
        reqs, recvbufs = [], {}
        for p in peers:
            pk = [d for d in desc if d[0] == 1 and d[1] == p]
            up = [d for d in desc if d[0] == 2 and d[1] == p]
            if pk:
                buf = np.concatenate([fabs[int(d[2])][0].a[region_view(int(d[2]), d[4:7], d[7:10], d[10:13])][..., 0].ravel(order="F") for d in pk])
                reqs.append(dist.isend(torch.from_numpy(buf.copy()), p))
            if up:
                npts = sum(int(np.prod(d[7:10] - d[4:7] + 1)) for d in up)
                t = torch.empty(npts, dtype=torch.float64)
                recvbufs[p] = (t, up)
                reqs.append(dist.irecv(t, p))
        for d in desc:
            if d[0] == 0:
                s, t = int(d[2]), int(d[3])
                fabs[t][0].a[region_view(t, d[4:7], d[7:10])] = fabs[s][0].a[region_view(s, d[4:7], d[7:10], d[10:13])]
        for r in reqs:
            r.wait()
        for p, (t, up) in recvbufs.items():
            a = t.numpy()
            for d in up:
                shp = tuple(int(x) for x in (d[7:10] - d[4:7] + 1))
                off = int(d[13])
                fabs[int(d[3])][0].a[region_view(int(d[3]), d[4:7], d[7:10])][..., 0] = a[off:off + int(np.prod(shp))].reshape(shp, order="F")

    z = orc.i3([0, 0, 0])
    for _ in range(NSWEEP):
        for rb in (0, 1):
            exchange()
            for bi in mine:
                phi, rhs, bn, lo = fabs[bi]
                lev, bg = levs[bi]
                # box origins are multiples of 4, so local and global colour parity coincide
                L.orc_abec_gsrb(C.byref(lev), phi.ref(), rhs.ref(), rb, C.c_double(1.15), z, z, 3)
    # a scalar all-reduce as used for norms / dt (ParallelDescriptor::ReduceRealMax role)
    loc = max(np.abs(fabs[bi][0].valid(fabs[bi][2])).max() for bi in mine)
    t = torch.tensor([loc], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), gmax=t.item(),
             **{f"box{bi}": fabs[bi][0].valid(fabs[bi][2])[..., 0] for bi in mine})
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_halo_exchange_matches_single_rank(orc, tmp_path):
    ref = reference_single_box(orc)
    ranks.spawn(worker, 2, ranks.free_port(), str(tmp_path))
    got = np.zeros(N)
    gmax = []
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        gmax.append(float(z["gmax"]))
        for bi, (lo, hi) in enumerate(BOXES):
            if OWNERS[bi] == r:
                got[tuple(slice(lo[q], hi[q] + 1) for q in range(3))] = z[f"box{bi}"]
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    assert gmax[0] == gmax[1] == np.abs(ref).max()


def test_eight_rank_gloo_halo_exchange_of_the_bench_layout(orc, tmp_path):
    """the layout of bench.py --gpus 8 (1 x 2 x 4 boxes of 8^3, every rank owns one box, every face of a box towards another rank or its
    periodic image) on an 8-member gloo world: the product's plans, message matching and the all-reduce give the single-box sweep bit
    for bit.  No device is opened: the eight-rank world of the GPU path is bounded by the processes a test may run on the GPU."""
    n, boxes, owners = layout("bench8")
    assert len(set(owners)) == 8 and n == (8, 16, 32)
    ref = reference_single_box(orc, n)
    ranks.spawn(worker, 8, ranks.free_port(), str(tmp_path), "bench8", max_ranks=8)      # (no device is opened: MAX_RANKS does not bind)
    got = np.zeros(n)
    gmax = []
    for r in range(8):
        z = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        gmax.append(float(z["gmax"]))
        lo, hi = boxes[r]
        got[tuple(slice(lo[q], hi[q] + 1) for q in range(3))] = z[f"box{r}"]
    assert np.array_equal(got, ref), np.abs(got - ref).max()
    assert all(g == np.abs(ref).max() for g in gmax)
