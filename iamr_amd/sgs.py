"""A-priori LES analysis of a triply periodic level (include/iamrx.h: iamrx_mf_sgs / iamrx_ns_sgs / iamrx_amr_sgs; kernels in
csrc/k_sgs.hip, driver in csrc/k_spectrum.hip): the subgrid stress tau_ij = (u_i u_j)~ - u~_i u~_j of the filtered velocity, the
inter-scale flux Pi = -tau_ij S~_ij, how much of it is backscatter, and which Smagorinsky constant reproduces it -- for the textbook
operator ("strain", D = Delta^2 |S~|) and for the one the closure of this code runs ("gradient", D = Delta^2 sqrt(2 A~:A~), what
ns.smago_Cs_cst multiplies).  The calls into the library, the ratios derived on the host, and the text file the driver writes
(ns.sgs_interval, inputs.py) with its reader.  Apart from `mf_sgs` and `level_sgs` this is host-only code."""
import ctypes as C
import math
import os
import numpy as np

STAT_NAMES = ("Pi", "Pi2", "Pi_neg", "k_sgs", "S2", "taud2",
              "P_strain", "P2_strain", "PiP_strain", "MM_strain", "LM_strain",
              "P_gradient", "P2_gradient", "PiP_gradient", "MM_gradient", "LM_gradient")
FIELD_NAMES = ("tau_xx", "tau_xy", "tau_xz", "tau_yy", "tau_yz", "tau_zz", "k_sgs", "sgs_flux", "filtered_strain", "smag_flux")
MODELS = ("strain", "gradient")
COUNT_NAMES = ("N", "negative_cells")
FILTERS = ("sharp", "gaussian", "box")          # what ns.sgs_filter may name (the identity filter has no subgrid scales)


def field_ids(fields):
    """names or ids -> ids; a single name or id is a list of one"""
    if isinstance(fields, (str, int, np.integer)):
        fields = [fields]
    ids = []
    for f in fields:
        if isinstance(f, str):
            if f not in FIELD_NAMES:
                raise ValueError(f"sgs: field '{f}', known are {' '.join(FIELD_NAMES)}")
            ids.append(FIELD_NAMES.index(f))
        else:
            ids.append(int(f))
    return ids


def delta_of(geom, kc):
    """the filter width Delta = L_max / (2 kc)"""
    return max(geom.prob_hi[d] - geom.prob_lo[d] for d in range(3)) / (2.0 * float(kc))


def _ratio(a, b):
    return a / b if b != 0.0 else math.nan


def derived(stats, counts):
    """the host-side ratios of a statistics vector (16 doubles) and the two counts: {"backscatter_fraction", "backscatter_share", and per
    model name a dict "Cs2_flux", "Cs2_lsq", "rho_tensor", "rho_flux"}; a ratio whose denominator is 0 is nan"""
    s = [float(v) for v in stats]
    N, neg = int(counts[0]), int(counts[1])
    out = dict(backscatter_fraction=_ratio(float(neg), float(N)), backscatter_share=_ratio(-s[2], s[0] - s[2]))
    for m, name in enumerate(MODELS):
        P, P2, PiP, MM, LM = s[6 + 5 * m: 11 + 5 * m]
        var = (s[1] - s[0] * s[0]) * (P2 - P * P)
        out[name] = dict(Cs2_flux=_ratio(s[0], P), Cs2_lsq=_ratio(-LM, MM),
                         rho_tensor=_ratio(-2.0 * LM, math.sqrt(s[5] * 2.0 * MM) if s[5] * MM > 0.0 else 0.0),
                         rho_flux=_ratio(PiP - s[0] * P, math.sqrt(var) if var > 0.0 else 0.0))
    return out


def as_dict(stats, counts, delta, fields=None):
    """the dict the Python layer hands out: the 16 named statistics, "N", "negative_cells", "delta", "stats" (the vector), the derived
    ratios and "fields" (the MultiFab, component q = the q-th requested field, or None)"""
    d = {nm: float(stats[q]) for q, nm in enumerate(STAT_NAMES)}
    d.update(N=int(counts[0]), negative_cells=int(counts[1]), delta=float(delta), stats=np.array(stats, dtype=np.float64), fields=fields)
    d.update(derived(stats, counts))
    return d


def _call(entry, head, geom, kc, layout, fields):
    """one of the three entries; head: its leading arguments up to and including kind"""
    from .lib import lib, check, MultiFab, CELL
    ids = field_ids(fields)
    n = lib().iamrx_sgs_nstat()
    if n != len(STAT_NAMES):
        raise RuntimeError(f"sgs: the library has {n} statistics, sgs.py names {len(STAT_NAMES)}")
    stats = np.zeros(n)
    counts = (C.c_long * 2)()
    out = MultiFab(layout, CELL, len(ids), 0) if ids else None
    which = (C.c_int * len(ids))(*ids) if ids else None
    check(entry(*head, C.c_double(float(kc)), out.h if out else None, 0, len(ids), which, stats.ctypes.data_as(C.POINTER(C.c_double)), counts))
    return as_dict(stats, counts, delta_of(geom, kc), out)


def mf_sgs(geom, vel, kind, kc, fields=(), vcomp=0, layout=None):
    """iamrx_mf_sgs of vel(vcomp .. vcomp + 2), a cell-centred MultiFab that tiles the fully periodic domain of geom; kind / kc: the
    filter of mf_filter.  fields: names or ids of FIELD_NAMES, returned under "fields" as a new MultiFab on `layout` (default: that
    of vel).  Collective."""
    from .lib import lib
    from .spectral import _kind
    return _call(lib().iamrx_mf_sgs, (C.byref(geom), vel.h, int(vcomp), _kind(kind)), geom, kc, layout or vel.layout, fields)


def level_sgs(entry, handle, geom, layout, kind, kc, fields=()):
    """iamrx_ns_sgs / iamrx_amr_sgs (entry: the library's function) on a level or hierarchy handle"""
    from .spectral import _kind
    return _call(entry, (handle, _kind(kind)), geom, kc, layout, fields)


# ------------------------------------------------------------------------------------------------------------------ the time series
COLUMNS = ("kc",) + STAT_NAMES + COUNT_NAMES


def header_line():
    return "# step time " + " ".join(COLUMNS)


def start_file(path, append=False):
    """a fresh file with its header line; append (a restarted run): an existing file is kept and must carry the same header"""
    if append and os.path.exists(path):
        with open(path) as f:
            first = f.readline().rstrip("\n")
        if first != header_line():
            raise ValueError(f"sgs: {path} holds '{first}', this run writes '{header_line()}'")
        return
    with open(path, "w") as f:
        f.write(header_line() + "\n")


def append_row(path, step, time, kc, stats, counts):
    """one row `step time kc` + the 16 statistics (17 significant digits: they read back to the bit) + the two counts"""
    if len(stats) != len(STAT_NAMES) or len(counts) != 2:
        raise ValueError(f"sgs: {len(stats)} statistics and {len(counts)} counts, a row holds {len(STAT_NAMES)} and 2")
    if not os.path.exists(path):
        start_file(path)
    with open(path, "a") as f:
        f.write(f"{int(step)} {float(time):.17g} {float(kc):.17g} " + " ".join(f"{float(v):.17g}" for v in stats) + f" {int(counts[0])} {int(counts[1])}\n")


def read_sgs(path):
    """the columns of the file: {"step" (int64), "time", "kc", every name of STAT_NAMES (float64), "N", "negative_cells" (int64), one entry
    per row; "stats": (rows, 16) float64}"""
    with open(path) as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if not lines or lines[0] != header_line():
        raise ValueError(f"sgs: {path} does not start with the header line '{header_line()}'")
    rows = [ln.split() for ln in lines[1:] if not ln.startswith("#")]
    for r in rows:
        if len(r) != 2 + len(COLUMNS):
            raise ValueError(f"sgs: {path}: a row holds {len(r)} columns, the header names {2 + len(COLUMNS)}")
    out = dict(step=np.array([int(r[0]) for r in rows], dtype=np.int64), time=np.array([float(r[1]) for r in rows], dtype=np.float64),
               kc=np.array([float(r[2]) for r in rows], dtype=np.float64))
    for q, nm in enumerate(STAT_NAMES):
        out[nm] = np.array([float(r[3 + q]) for r in rows], dtype=np.float64)
    for q, nm in enumerate(COUNT_NAMES):
        out[nm] = np.array([int(r[3 + len(STAT_NAMES) + q]) for r in rows], dtype=np.int64)
    out["stats"] = np.array([[float(v) for v in r[3:3 + len(STAT_NAMES)]] for r in rows], dtype=np.float64).reshape(len(rows), len(STAT_NAMES))
    return out
