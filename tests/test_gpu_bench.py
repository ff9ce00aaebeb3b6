"""GPU: bench.py's plain run (what every measurement of the headline starts) and its --dump-outputs, at a small box: exactly --steps timed
steps in one region, the headline fields and nothing of what --full adds, and the dumped arrays equal the state of the same problem
advanced by warm-up + timed steps in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    from iamr_amd import ns as N
    n, steps, warmup = 32, 3, 2
    out_dir = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--n", str(n),
           "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "cells-advanced/sec" and d["unit"] == "cells/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == steps and d["warmup"] == warmup and d["repeats"] == 1 and d["n_gpus"] == 1
    assert abs(d["value"] - n ** 3 * steps / (d["ms_per_step"] * steps * 1e-3)) < 1e-9 * d["value"]
    for key in ("cpu_baseline", "amr", "kernels", "roofline", "sections_ms_per_step", "single_gpu_multibox", "rayleigh_taylor"):
        assert key not in d, key

    # the same problem advanced warm-up + timed steps here (bench.py main: one n^3 box, TaylorGreen prob.c = 1)
    g = gpu.Geom.make((n, n, n), prob_hi=(1.0, 1.0, 1.0))
    ns = N.NavierStokes(g, gpu.Layout([((0, 0, 0), (n - 1, n - 1, n - 1))], [0]),
                        N.ns_params(cfl=0.7, visc_coef=1e-4, init_iter=2, init_shrink=1.0), gpu.mg_opts())
    ns.init_taylorgreen(1.0, 1.0, 1.0, 1.0, 1.0)
    ns.post_init(-1.0)
    dt = [ns.step() for _ in range(warmup + steps)][-1]
    S = ns.data(N.NavierStokes.S_NEW).gather_valid((n, n, n)).reshape(-1, 5, order="F")
    P = ns.data(N.NavierStokes.P_NEW).gather_valid((n, n, n)).reshape(-1, order="F")
    want = {"velocity": S[:, 0:3], "density": S[:, 3], "tracer": S[:, 4], "pressure": P, "dt": np.array([dt])}
    files = sorted(os.listdir(out_dir))
    assert files == sorted(k + ".npy" for k in want), files
    total = 0
    for k, ref in want.items():
        a = np.load(os.path.join(out_dir, k + ".npy"))
        total += a.nbytes
        assert a.dtype == np.float64 and a.shape == ref.shape, (k, a.dtype, a.shape)
        assert np.all(np.isfinite(a)), k
        assert np.abs(a - ref).max() <= 1e-10 * max(1.0, float(np.abs(ref).max())), (k, float(np.abs(a - ref).max()))
    assert total <= 64 << 20


@pytest.mark.parametrize("typ,ncomp", [((0, 0, 0), 5), ((1, 1, 1), 1)], ids=["cells", "nodes"])
def test_dump_sample_of_large_boxes(gpu, typ, ncomp):
    """the seeded-sample branch of bench.sample_valid, which every 256^3 dump takes, at a small npts_max: two unequal boxes with ghost
    cells, cell and nodal data.  The sample is the listing of the valid points (box after box, i fastest; gather_valid's values) at the
    sorted positions a generator with the given seed draws, and the same in every call"""
    import bench
    n = (24, 16, 8)
    boxes = [((0, 0, 0), (15, 15, 7)), ((16, 0, 0), (23, 15, 7))]
    lay = gpu.Layout(boxes, [0, 0])
    mf = gpu.MultiFab(lay, typ, ncomp, 1)
    glo = (-1, -1, -1)
    G = np.random.default_rng(7).standard_normal(tuple(n[d] + typ[d] + 2 for d in range(3)) + (ncomp,))
    mf.set_from_global(np.asfortranarray(G), glo)
    V = mf.gather_valid(n)
    listing = []
    for li in range(mf.nlocal()):
        lo, hi, _ = lay.local_box(li)
        listing.append(V[tuple(slice(lo[d], hi[d] + typ[d] + 1) for d in range(3))].reshape(-1, ncomp, order="F"))
    listing = np.concatenate(listing)
    assert np.array_equal(bench.sample_valid(mf, listing.shape[0], seed=0), listing)        # the "all points" branch
    npts = 100
    pick = np.sort(np.random.default_rng(3).choice(listing.shape[0], npts, replace=False))
    got = bench.sample_valid(mf, npts, seed=3)
    assert got.shape == (npts, ncomp) and got.dtype == np.float64
    assert np.array_equal(got, listing[pick])
    assert np.array_equal(bench.sample_valid(mf, npts, seed=3), got)
    assert not np.array_equal(bench.sample_valid(mf, npts, seed=4), got)
