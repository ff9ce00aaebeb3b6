"""GPU: the slab-decomposed transform of the shell-summed diagnostics (registry key SPECTRUM_DIST = 1) on 2 and 4 ranks (ranks sharing
the one GPU over the gloo callback transport: tests/ranks.py).  Every rank returns the same bytes, and those bytes are the one-rank
result to the bit; iamrx_spectrum_slab_info shows that the slab path ran, that no rank held more than its share, and that exactly
the counted doubles travelled.  With the key back at 0 the same ranks gather, and return the same bytes again.  The rank processes run
with IAMRX_POISON_ALLOC = 1: an element of a slab, a buffer or the mirror image that nobody wrote is a NaN in the result.

Doubles a rank r of R sends through the communicator's exchange, shape (nx, ny, nz), N = nx ny nz, nzl = nz / R:
  scatter    S_r = the cells of the rank's send rows in iamrx_host_spectrum_slab_plan (a box piece outside the own slab; 1 double per cell)
  transpose  T = 2 (R - 1) N / R^2: one block of N / R^2 modes (2 doubles each) to every other rank; two transposes per transform
  mirror     M_r = 2 nx ny ([(R - r) % R != r] + nzl - 1): the first plane unless it mirrors into the rank itself, the others always
  one plain transform of a field  S_r + 2 T;  one packed pair of two fields on the layout  2 S_r + 2 T + M_r.
Doubles received: the same with the rank's receive rows in place of its send rows.  The sum of the slot arrays over the ranks and the
gather's sum of the field are all-reduces, not exchanges, and are not counted."""
import os
import sys
import numpy as np
import pytest
import ranks
import spectrum_numpy as SN

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
N3 = (16, 16, 16)
BUD = ("E", "T", "Pi", "D", "F", "count")
# name -> (n, L, max_grid_size); c16 takes Layout.decompose's owners, the others scatter their boxes over the ranks
CASES = {"c16": (N3, (1.0, 1.0, 1.0), (8, 8, 8)),
         "yz": ((16, 8, 32), (1.0, 0.5, 1.5), (16, 4, 8)),          # boxes cut in y and z, three different r_d
         "flat": ((16, 16, 4), (1.0, 1.0, 1.0), (8, 8, 4)),         # 4 ranks: one plane per rank
         "tiny": ((4, 4, 4), (1.0, 1.0, 1.0), (2, 2, 2))}           # 4 ranks: one plane and one row per rank


def layout_of(L, name, world):
    n, _, mg = CASES[name]
    lay = L.Layout.decompose(n, mg, world)
    if name == "c16" or world == 1:
        return lay
    return L.Layout(lay.boxes, [(i + 1) % world for i in range(len(lay.boxes))])


def geom_of(L, name):
    n, Lx, _ = CASES[name]
    return L.Geom.make(list(n), prob_hi=Lx, periodic=(1, 1, 1))


def fill_mf(L, lay, f):
    """f on the valid cells of every local box, NaN in all ghost cells"""
    nc = f.shape[3]
    mf = L.MultiFab(lay, L.CELL, nc, 1)
    for li in range(mf.nlocal()):
        glo, ghi = mf.fab_box(li)
        lo, hi, _ = lay.local_box(li)
        a = np.full(tuple(ghi[d] - glo[d] + 1 for d in range(3)) + (nc,), np.nan, order="F")
        a[tuple(slice(lo[d] - glo[d], hi[d] - glo[d] + 1) for d in range(3))] = f[tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
        mf.from_numpy(a, li)
    return mf


def diagnostics(L, name, world, info=None):
    """the calls of a case -> {column: array}; info(call, layout): called after each with the call's name"""
    from test_gpu_budget_multirank import level_of
    from test_gpu_profile import random_state
    n = CASES[name][0]
    lay, g = layout_of(L, name, world), geom_of(L, name)
    mf = fill_mf(L, lay, SN.noise(n, 11, 3))
    out = {}
    out["P"], out["cnt"] = L.mf_spectrum(g, mf, 0, 3)
    info and info("spectrum", lay)
    out["W"] = L.mf_spectrum_k2(g, mf, 0, 3)
    info and info("k2", lay)
    out["Cab"], out["Pa"], out["Pb"], out["ccnt"] = L.mf_cospectrum(g, mf, mf, 0, 2)
    info and info("pair", lay)
    if name == "c16":
        s = level_of(L, lay, random_state(N3, 12)).spectral_budget()
        info and info("budget", lay)
        out.update({"bud_" + c: s[c] for c in BUD})
    return out


def expected_traffic(L, name, lay, rank, world, call):
    n = CASES[name][0]
    N = n[0] * n[1] * n[2]
    ok, why, rows = L.host_spectrum_slab_plan(geom_of(L, name), lay.boxes, lay.owners, rank, world)
    assert ok, why
    cells = np.prod(rows[:, 6:9] - rows[:, 3:6] + 1, axis=1)
    S = {1: int(cells[rows[:, 0] == 1].sum()), 2: int(cells[rows[:, 0] == 2].sum())}
    T = 2 * (world - 1) * N // world ** 2
    M = 2 * n[0] * n[1] * (int((world - rank) % world != rank) + n[2] // world - 1)
    plain = {k: S[k] + 2 * T for k in S}
    pair = {k: 2 * S[k] + 2 * T + M for k in S}
    nt = {"spectrum": 3, "k2": 3, "pair": 1, "budget": 3}[call]
    per = plain if call in ("spectrum", "k2") else pair
    return nt, nt * per[1], nt * per[2]


def slab_ranks(rank, world, port, out_dir):
    os.environ["IAMRX_POISON_ALLOC"] = "1"
    L = ranks.start_rank(rank, world, port)
    assert L.tuning_get("POISON_ALLOC", 0) == 1
    res = {}
    for name in CASES:
        n = CASES[name][0]
        share = n[0] * n[1] * n[2] // world

        def on_slab(call, lay):
            i = L.spectrum_slab_info()
            nt, sent, received = expected_traffic(L, name, lay, rank, world, call)
            assert i["path"] == 1 and i["ranks"] == world and i["transforms"] == nt, (name, call, i)
            assert i["per_pass"] == share, (name, call, i)
            assert i["max_image"] == share if call in ("spectrum", "k2") else i["max_image"] <= 2 * share, (name, call, i)
            assert (i["sent"], i["received"]) == (sent, received), (name, call, i, sent, received)

        def on_gather(call, lay):
            i = L.spectrum_slab_info()
            assert i["path"] == 0 and i["ranks"] == world and i["sent"] == 0 and i["max_image"] == world * share, (name, call, i)

        L.tuning_set("SPECTRUM_DIST", 1)
        for k, v in diagnostics(L, name, world, on_slab).items():
            res[f"{name}_slab_{k}"] = v
        L.tuning_set("SPECTRUM_DIST", 0)
        for k, v in diagnostics(L, name, world, on_gather).items():
            res[f"{name}_gather_{k}"] = v
    np.savez(os.path.join(out_dir, f"slab_w{world}_r{rank}.npz"), **res)
    ranks.stop_rank()


_ONE = {}


def one_rank(gpu, name):
    """the one-rank result of a case, taken once in this process on the same boxes"""
    if name not in _ONE:
        _ONE[name] = diagnostics(gpu, name, 1)
        assert gpu.spectrum_slab_info()["path"] == 0
        for k in ("P", "W", "Cab") + (("bud_T", "bud_D") if name == "c16" else ()):
            assert _ONE[name][k].any(), (name, k)
    return _ONE[name]


@pytest.mark.parametrize("world", [2, ranks.MAX_RANKS])
def test_slab_ranks_against_one(gpu, tmp_path, world):
    d = str(tmp_path)
    ranks.spawn(slab_ranks, world, ranks.free_port(), d)
    got = [np.load(os.path.join(d, f"slab_w{world}_r{r}.npz")) for r in range(world)]
    for name in CASES:
        for k, v in one_rank(gpu, name).items():
            for path in ("slab", "gather"):
                key = f"{name}_{path}_{k}"
                for r in range(world):
                    assert got[r][key].dtype == v.dtype and got[r][key].tobytes() == v.tobytes(), (key, r)      # every rank: the one-rank bytes


def refused_ranks(rank, world, port, out_dir):
    L = ranks.start_rank(rank, world, port)
    lay = L.Layout.decompose(N3, 8, world)
    mf = fill_mf(L, lay, SN.noise(N3, 11, 1))
    g = L.Geom.make(list(N3), periodic=(1, 1, 1))
    L.tuning_set("SPECTRUM_DIST", 1)
    for call in (lambda: L.mf_spectrum(g, mf), lambda: L.mf_spectrum_k2(g, mf), lambda: L.mf_cospectrum(g, mf, mf)):
        with pytest.raises(L.IamrxError, match="not a power of two"):
            call()
    L.comm_barrier()                        # nobody is left waiting in a collective of the refused calls
    L.tuning_set("SPECTRUM_DIST", 0)
    P, _ = L.mf_spectrum(g, mf)             # and the gather still serves three ranks
    np.save(os.path.join(out_dir, f"refused_r{rank}.npy"), P)
    ranks.stop_rank()


def test_three_ranks_are_refused_on_every_rank(gpu, tmp_path):
    d = str(tmp_path)
    ranks.spawn(refused_ranks, 3, ranks.free_port(), d)
    lay = gpu.Layout.decompose(N3, 8)
    P, _ = gpu.mf_spectrum(gpu.Geom.make(list(N3), periodic=(1, 1, 1)), fill_mf(gpu, lay, SN.noise(N3, 11, 1)))
    for r in range(3):
        assert np.load(os.path.join(d, f"refused_r{r}.npy")).tobytes() == P.tobytes()


def _rccl_slab_pair(rank, world, out_dir):
    """one process per DEVICE: the c16 case over the RCCL transport"""
    import ctypes as C
    import time
    sys.path.insert(0, ranks.ROOT)
    sys.path.insert(0, os.path.join(ranks.ROOT, "tests"))
    os.environ.update(IAMRX_COALESCE="0", IAMRX_POISON_ALLOC="1")
    from iamr_amd import lib
    lib.init(rank)
    Lb = lib.lib()
    Lb.iamrx_comm_last_error.restype = C.c_char_p
    idf = os.path.join(out_dir, "rccl_id.bin")
    buf = (C.c_char * 128)()
    if rank == 0:
        assert Lb.iamrx_comm_get_unique_id(buf) == 0, Lb.iamrx_comm_last_error()
        with open(idf + ".tmp", "wb") as f:
            f.write(bytes(buf))
        os.replace(idf + ".tmp", idf)
    else:
        t0 = time.time()
        while not os.path.exists(idf):
            assert time.time() - t0 < 120, "rank 0 never published the RCCL unique id"
            time.sleep(0.05)
        buf = (C.c_char * 128).from_buffer_copy(open(idf, "rb").read())
    assert Lb.iamrx_comm_init_rccl(buf, rank, 2) == 0, Lb.iamrx_comm_last_error()
    lib.tuning_set("SPECTRUM_DIST", 1)

    def on_slab(call, lay):
        assert lib.spectrum_slab_info()["path"] == 1
    np.savez(os.path.join(out_dir, f"slab_rccl_r{rank}.npz"), **diagnostics(lib, "c16", 2, on_slab))


def test_slab_over_rccl_between_two_devices(gpu, tmp_path):
    """Needs two visible devices; on one GPU it is SKIPPED LOUDLY: the slab path has then run over the callback transport only."""
    import torch
    nd = torch.cuda.device_count()
    if nd < 2:
        msg = (f"SLAB TRANSFORM OVER RCCL NOT EXERCISED: {nd} device(s) visible -- the slab-decomposed spectra have run over the callback "
               "transport only (tests/test_gpu_spectrum_slab.py::test_slab_over_rccl_between_two_devices runs as soon as 2 GPUs are visible)")
        print("\n*** " + msg + " ***", file=sys.stderr, flush=True)
        pytest.skip(msg)
    ranks.spawn(_rccl_slab_pair, 2, str(tmp_path))
    for r in range(2):
        z = np.load(os.path.join(str(tmp_path), f"slab_rccl_r{r}.npz"))
        for k, v in one_rank(gpu, "c16").items():
            assert z[k].tobytes() == v.tobytes(), (k, r)
