"""GPU: the device scratch of the diagnostics belongs to the call (DevBuf / PassTimer, iamr_amd/csrc/mf.h).  What a caller can observe
through the C-ABI: the bytes in use (iamrx_mem_info) are after a call what they were before it -- also after a refusal that comes when
the work arrays already exist -- and a bench entry fills exactly its NP * reps floats.

Every entry is called once before the reading it is measured against: the first call on a layout may build that LAYOUT's cached lists
(tile lists, profile lists: mf.hip level_tile_list, k_profile.hip profile_list), which live as long as the layout and are no scratch of
the call.  The eight-box layout runs the pack and unpack over several boxes; the gather of spec_pack, with its own block R, needs
several ranks and runs under test_gpu_specop_multirank.py."""
import ctypes as C
import numpy as np
import pytest
from test_gpu_spectrum import make_mf, geom_of, UNIT
from test_gpu_specop import nan_mf, all_nan
from test_gpu_profile import one_level, random_state

pytestmark = pytest.mark.gpu
PF = C.POINTER(C.c_float)
PD = C.POINTER(C.c_double)


def _mem(lib):
    live, cached = C.c_size_t(), C.c_size_t()
    lib.check(lib.lib().iamrx_mem_info(C.byref(live), C.byref(cached)))
    return live.value, cached.value


def _live_returns(lib, tag, call):
    call()
    lib.sync()
    live0 = _mem(lib)[0]
    call()
    lib.sync()
    assert _mem(lib)[0] == live0, (tag, _mem(lib)[0] - live0)


def _field(n, ncomp, seed=5):
    return np.random.default_rng(seed).standard_normal(tuple(n) + (ncomp,)) + 0.3


# ------------------------------------------------------------------------------------------------------------------ 1. the live bytes
@pytest.mark.parametrize("mgs", [None, 4])
def test_live_bytes_come_back(gpu, mgs):
    """8^3 as one box and as eight 4^3 boxes: every diagnostic entry that works through arena scratch leaves `live` where it was"""
    from iamr_amd.spectrum import nbins_of
    lib = gpu
    n = (8, 8, 8)
    g = geom_of(n)
    src, lay = make_mf(n, _field(n, 3), mgs)
    dst, _ = nan_mf(n, 3, mgs)
    ns, _ = one_level(n, random_state(n, 11), mgs)
    nb = nbins_of(n, UNIT)
    E = np.zeros(nb)
    E[1:4] = 1.0
    out, nbv = np.zeros(2 * nb), C.c_int()

    def spectrum_without_count():
        lib.check(lib.lib().iamrx_mf_spectrum(C.byref(g), src.h, 0, 2, nb, out.ctypes.data_as(PD), None, C.byref(nbv)))

    calls = [("spectrum, count", lambda: lib.mf_spectrum(g, src, 0, 2)),
             ("spectrum, no count", spectrum_without_count),
             ("cospectrum", lambda: lib.mf_cospectrum(g, src, src, 0, 1)),
             ("spectrum_k2", lambda: lib.mf_spectrum_k2(g, src, 0, 2))]
    calls += [(f"filter {kind}", lambda kind=kind: lib.mf_filter(g, dst, src, kind, 2.5)) for kind in ("identity", "sharp", "gaussian", "box")]
    calls += [(f"solenoidal {w}", lambda w=w: lib.mf_solenoidal(g, dst, src, w)) for w in ("exact", "centred")]
    calls += [("synthesize", lambda: lib.mf_synthesize(g, dst, E, 7, "centred")),
              ("strfn", lambda: lib.mf_structure(g, src, 0, 2, pmax=4)),
              ("histogram", lambda: lib.mf_histogram(src, 0, 2, nbins=16, range=(-4.0, 4.0)))]
    calls += [(f"plane profile {d}", lambda d=d: ns.plane_profile(d)) for d in range(3)]
    for tag, call in calls:
        _live_returns(lib, f"{tag}, max_grid_size {mgs}", call)
    assert nbv.value == nb


def test_live_bytes_come_back_after_a_late_refusal(gpu):
    """the input of test_synthesis_refuses_an_empty_shell (test_gpu_specop.py): the refusal comes from the device, when every work array
    of the synthesis exists.  The same message as ever, dst untouched, `live` back."""
    from iamr_amd.lib import IamrxError
    from iamr_amd.spectrum import nbins_of
    lib = gpu
    n, L = (4, 4, 4), (1.0, 1.0, 4.0)
    g = geom_of(n, L)
    dst, _ = nan_mf(n, 3)
    E = np.zeros(nbins_of(n, L))
    E[2] = 1.0
    E[3] = 1.0

    def refused():
        with pytest.raises(IamrxError, match="spectrum: the target spectrum asks for energy in shell 3, where the projected noise has none"):
            lib.mf_synthesize(g, dst, E, 1, "centred")

    _live_returns(lib, "synthesize, empty shell", refused)
    assert all_nan(dst)


# ------------------------------------------------------------------------------------------------------------------ 2. the bench entries
def _bench(lib, tag, NP, call, reps=2):
    """call(reps, ms) as the tools call it: returns 0, fills NP * reps finite times >= 0 and not one float more; `live` comes back"""
    def run(r):
        ms = np.full(NP * r + 1, np.nan, dtype=np.float32)
        assert call(r, ms.ctypes.data_as(PF)) == 0, (tag, lib.lib().iamrx_last_error())
        return ms
    run(1)
    lib.sync()
    live0 = _mem(lib)[0]
    ms = run(reps)
    lib.sync()
    assert _mem(lib)[0] == live0, (tag, _mem(lib)[0] - live0)
    assert np.isnan(ms[NP * reps]), tag
    assert np.all(np.isfinite(ms[:NP * reps])) and np.all(ms[:NP * reps] >= 0.0), (tag, ms)


@pytest.mark.parametrize("n", [(8, 8, 8), (16, 8, 8)])
def test_spectral_bench_entries(gpu, n):
    lib = gpu
    L = lib.lib()
    g = geom_of(n)
    src, _ = make_mf(n, _field(n, 2))
    dst, _ = nan_mf(n, 3)
    assert L.iamrx_specop_bench_np() == 17
    _bench(lib, "spectrum", 5, lambda r, ms: L.iamrx_spectrum_bench(C.byref(g), src.h, 0, r, ms))
    _bench(lib, "cospectrum", 5, lambda r, ms: L.iamrx_cospectrum_bench(C.byref(g), src.h, 0, src.h, 1, r, ms))
    _bench(lib, "specop", 17, lambda r, ms: L.iamrx_specop_bench(C.byref(g), dst.h, src.h, 0, 2, C.c_double(1.0), 1, r, ms))


def test_other_bench_entries(gpu):
    lib = gpu
    L = lib.lib()
    n = (8, 8, 8)
    g = geom_of(n)
    vel, lay = make_mf(n, _field(n, 3))
    vel.fill_boundary(g)
    out = lib.MultiFab(lay, lib.CELL, 3, 0)
    lo, hi = np.full(2, -4.0), np.full(2, 4.0)
    ids = (C.c_int * 3)(7, 8, 4)
    _bench(lib, "strfn", 4, lambda r, ms: L.iamrx_strfn_bench(C.byref(g), vel.h, 0, 4, (C.c_int * 3)(4, 4, 4), r, ms))
    _bench(lib, "hist", 1, lambda r, ms: L.iamrx_hist_bench(vel.h, 0, 2, None, lo.ctypes.data_as(PD), hi.ctypes.data_as(PD), 16, 0, r, ms))
    _bench(lib, "velgrad", 1, lambda r, ms: L.iamrx_velgrad_bench(C.byref(g), out.h, 3, ids, vel.h, 0, C.c_double(0.001), 0, 0, r, ms))
    _bench(lib, "convective", 1, lambda r, ms: L.iamrx_convective_bench(C.byref(g), out.h, vel.h, 0, r, ms))
