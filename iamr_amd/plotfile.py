"""AMReX-format plotfiles: writer, reader and an fcompare-style comparison.

Format restated from the reference's committed plotfile `Exec/run2d/test_grids/plt0000_1` (Header, Level_*/Cell_H, Cell_D_* --
kept as a data fixture under tests/golden/plt0000_1) and from the call sites that produce it (NavierStokesBase::writePlotFile,
Source/NavierStokesBase.cpp:3344-3352 / AmrLevel::writePlotFile role):

  <dir>/Header            version string, ncomp, names, dim, time, finest_level, prob_lo, prob_hi, ref_ratio, domains, level steps,
                          dx per level, coord_sys, 0, then per level: "lev ngrids time", step, the physical extent of every grid,
                          and the relative path "Level_<l>/Cell"
  <dir>/Level_<l>/Cell_H  VisMF header: version 1, how 0, ncomp, ngrow, the BoxArray, "FabOnDisk: file offset" per grid, and the
                          per-grid / per-component minima and maxima
  <dir>/Level_<l>/Cell_D_00000   per grid: "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))(box) ncomp\\n" + the doubles
                          (little endian, Fortran order, one component after the other); a run on several ranks writes one
                          Cell_D_<rank:05d> per rank that owns grids of the level (PlotFile.write_data / write_headers)

Host-side I/O (control plane): plain Python + numpy, dimension-generic (2-D files of the reference can be read)."""
import os
import re
import numpy as np
from . import pdf as _pdf

REAL_DESC = "((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))"


def _fmt(x):
    """shortest round-trip representation, the way operator<< prints the reference's numbers (0.0625, 0, 1, 0.5 ...)"""
    x = float(x)
    if x == int(x) and abs(x) < 1e15:
        return str(int(x))
    return repr(x)


def _fmt17(x):
    return "%.15g" % x if float("%.15g" % x) == x else "%.17g" % x


def _box_str(lo, hi):
    dim = len(lo)
    return "((" + ",".join(str(v) for v in lo) + ") (" + ",".join(str(v) for v in hi) + ") (" + ",".join("0" for _ in range(dim)) + "))"


def data_file(rank):
    """name (after the MultiFab's prefix) of the data file rank `rank` writes: VisMF's one file per writer"""
    return f"_D_{rank:05d}"


def write_fabs(path, fabs):
    """one writer's data file: fabs = [(box text of the FAB header, array (n..., ncomp))] one after the other -> per fab
    (offset, minima[nc], maxima[nc]).  The doubles go out x fastest, component outermost (the FAB byte order)."""
    out = []
    with open(path, "wb") as f:
        for box, a in fabs:
            a = np.asarray(a, dtype="<f8")
            nc = a.shape[-1]
            off = f.tell()
            f.write(f"FAB {REAL_DESC}{box} {nc}\n".encode())
            f.write(np.asfortranarray(a).tobytes(order="F"))
            out.append((off, [a[..., n].min() for n in range(nc)], [a[..., n].max() for n in range(nc)]))
    return out


def write_vismf_header(path, nc, ngrow, boxes, fab_files, mins, maxs):
    """VisMF header of one MultiFab: boxes = the BoxArray as text, fab_files = (file, offset) per grid, mins / maxs per grid and component,
    all in global box order"""
    with open(path, "w") as f:
        f.write(f"1\n0\n{nc}\n{ngrow}\n({len(boxes)} 0\n")
        for b in boxes:
            f.write(b + "\n")
        f.write(f")\n{len(boxes)}\n")
        for fn, o in fab_files:
            f.write(f"FabOnDisk: {fn} {o}\n")
        for vals in (mins, maxs):
            f.write(f"\n{len(boxes)},{nc}\n")
            for row in vals:
                f.write("".join(_fmt17(v) + "," for v in row) + "\n")


def merge_meta(nboxes, metas):
    """metas = {rank: [(global box index, offset, minima, maxima), ...]} of one MultiFab from every writer -> (owner, offset, minima,
    maxima) per box in global order; every box must have exactly one writer"""
    rows = [None] * nboxes
    for rank in sorted(metas):
        for gi, off, mn, mx in metas[rank]:
            if rows[gi] is not None:
                raise ValueError(f"box {gi} was written by ranks {rows[gi][0]} and {rank}")
            rows[gi] = (rank, int(off), list(mn), list(mx))
    missing = [q for q, r in enumerate(rows) if r is None]
    if missing:
        raise ValueError(f"no rank wrote boxes {missing}")
    return rows


def gather_meta(nboxes, nc, meta, owners, allreduce):
    """the metadata exchange of a collective write: `meta` = this rank's [(global box index, offset, minima, maxima)] of one MultiFab;
    every box has one owner, who contributes its row of an [nboxes x (1 + 2 nc)] table, everyone else zeros; one sum (`allreduce(table,
    0)`: lib.comm_allreduce) gives every rank the table (offsets are far below 2^53: doubles carry them exactly).  Returns the `metas`
    dictionary merge_meta takes."""
    T = np.zeros((nboxes, 1 + 2 * nc))
    for gi, off, mn, mx in meta:
        T[gi, 0] = off
        T[gi, 1:1 + nc] = mn
        T[gi, 1 + nc:] = mx
    allreduce(T, 0)
    metas = {}
    for gi in range(nboxes):
        metas.setdefault(int(owners[gi]), []).append((gi, int(T[gi, 0]), list(T[gi, 1:1 + nc]), list(T[gi, 1 + nc:])))
    return metas


class Level:
    """one AMR level of a plotfile: index domain, mesh spacing, boxes and the data of every box (array (n..., ncomp), Fortran order).
    A rank of a multi-rank run holds the whole box list but only the data of the boxes it owns: `owned` = their global indices,
    increasing, one per entry of `data` (None: every box, in order)."""

    def __init__(self, domain, dx, boxes, data=None, step=0, time=0.0, owned=None):
        self.domain = (tuple(domain[0]), tuple(domain[1]))
        self.dx = tuple(dx)
        self.boxes = [(tuple(lo), tuple(hi)) for lo, hi in boxes]
        self.data = data
        self.step = step
        self.time = time
        self.owned = None if owned is None else [int(q) for q in owned]
        self.fab_files = None      # reader: (file, offset) per box


class PlotFile:
    def __init__(self, names, time, prob_lo, prob_hi, levels, ref_ratio=None, coord_sys=0, version="HyperCLaw-V1.1"):
        self.names = list(names)
        self.time = time
        self.prob_lo = tuple(prob_lo)
        self.prob_hi = tuple(prob_hi)
        self.levels = levels
        self.ref_ratio = list(ref_ratio) if ref_ratio is not None else [2] * (len(levels) - 1)
        self.coord_sys = coord_sys
        self.version = version

    # ------------------------------------------------------------------------------------------------ writer
    def header_text(self):
        dim = len(self.prob_lo)
        L = [self.version, str(len(self.names))] + self.names + [str(dim), _fmt(self.time), str(len(self.levels) - 1)]
        L.append(" ".join(_fmt(v) for v in self.prob_lo) + " ")
        L.append(" ".join(_fmt(v) for v in self.prob_hi) + " ")
        L.append(" ".join(str(r) for r in self.ref_ratio) + (" " if self.ref_ratio else ""))
        L.append(" ".join(_box_str(*lv.domain) for lv in self.levels) + " ")
        L.append(" ".join(str(lv.step) for lv in self.levels) + " ")
        for lv in self.levels:
            L.append(" ".join(_fmt(v) for v in lv.dx) + " ")
        L += [str(self.coord_sys), "0"]
        for l, lv in enumerate(self.levels):
            L.append(f"{l} {len(lv.boxes)} {_fmt(lv.time)}")
            L.append(str(lv.step))
            for lo, hi in lv.boxes:
                for d in range(dim):
                    L.append(f"{_fmt(self.prob_lo[d] + lo[d] * lv.dx[d])} {_fmt(self.prob_lo[d] + (hi[d] + 1) * lv.dx[d])}")
            L.append(f"Level_{l}/Cell")
        return "\n".join(L) + "\n"

    def write(self, path):
        """one writer holding every box (pinned byte for byte on the reference's plotfiles, tests/test_cpu_plotfile.py; the two-phase
        form below writes the same files for one rank, tests/test_cpu_multirank_io.py)"""
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "Header"), "w") as f:
            f.write(self.header_text())
        nc = len(self.names)
        for l, lv in enumerate(self.levels):
            ld = os.path.join(path, f"Level_{l}")
            os.makedirs(ld, exist_ok=True)
            offsets, mins, maxs = [], [], []
            fname = "Cell_D_00000"
            with open(os.path.join(ld, fname), "wb") as f:
                for (lo, hi), a in zip(lv.boxes, lv.data):
                    a = np.asarray(a, dtype="<f8")
                    assert a.shape == tuple(h - q + 1 for q, h in zip(lo, hi)) + (nc,), (a.shape, lo, hi)
                    offsets.append(f.tell())
                    f.write(f"FAB {REAL_DESC}{_box_str(lo, hi)} {nc}\n".encode())
                    f.write(np.asfortranarray(a).tobytes(order="F"))
                    mins.append([a[..., n].min() for n in range(nc)])
                    maxs.append([a[..., n].max() for n in range(nc)])
            with open(os.path.join(ld, "Cell_H"), "w") as f:
                f.write(f"1\n0\n{nc}\n0\n({len(lv.boxes)} 0\n")
                for lo, hi in lv.boxes:
                    f.write(_box_str(lo, hi) + "\n")
                f.write(f")\n{len(lv.boxes)}\n")
                for o in offsets:
                    f.write(f"FabOnDisk: {fname} {o}\n")
                for vals in (mins, maxs):
                    f.write(f"\n{len(lv.boxes)},{nc}\n")
                    for row in vals:
                        f.write("".join(_fmt17(v) + "," for v in row) + "\n")

    # ------------------------------------------------------------------------------ writer of a multi-rank run, in two phases
    # (AMReX's format: one data file per writer, headers that name a file and an offset per grid).  Neither phase knows about
    # communicators: the caller carries the metadata from the writers to the rank that writes the headers (write_collective does).
    def make_dirs(self, path):
        """the plotfile's directories (one rank, before anyone writes data)"""
        for l in range(len(self.levels)):
            os.makedirs(os.path.join(path, f"Level_{l}"), exist_ok=True)

    def write_data(self, path, rank=0):
        """phase A, every rank: Level_<l>/Cell_D_<rank:05d> with the fabs this rank owns (Level.owned / Level.data) in increasing global
        box index; a rank without a box of a level writes no file for it.  Returns per level [(global index, offset, minima, maxima)]."""
        nc = len(self.names)
        meta = []
        for l, lv in enumerate(self.levels):
            owned = list(range(len(lv.boxes))) if lv.owned is None else lv.owned
            assert len(owned) == len(lv.data) and all(a < b for a, b in zip(owned, owned[1:])), owned
            fabs = []
            for gi, a in zip(owned, lv.data):
                lo, hi = lv.boxes[gi]
                assert np.shape(a) == tuple(h - q + 1 for q, h in zip(lo, hi)) + (nc,), (np.shape(a), lo, hi)
                fabs.append((_box_str(lo, hi), a))
            if not fabs:
                meta.append([])
                continue
            ld = os.path.join(path, f"Level_{l}")
            os.makedirs(ld, exist_ok=True)
            res = write_fabs(os.path.join(ld, "Cell" + data_file(rank)), fabs)
            meta.append([(gi, off, mn, mx) for gi, (off, mn, mx) in zip(owned, res)])
        return meta

    def write_headers(self, path, metas):
        """phase B, one rank, once all data files are complete: Header and every Level_<l>/Cell_H from metas = {rank: what that rank's
        write_data returned}; grids, FabOnDisk lines and the min / max tables in global box order"""
        os.makedirs(path, exist_ok=True)
        nc = len(self.names)
        for l, lv in enumerate(self.levels):
            rows = merge_meta(len(lv.boxes), {r: m[l] for r, m in metas.items()})
            ld = os.path.join(path, f"Level_{l}")
            os.makedirs(ld, exist_ok=True)
            write_vismf_header(os.path.join(ld, "Cell_H"), nc, 0, [_box_str(lo, hi) for lo, hi in lv.boxes],
                               [("Cell" + data_file(r), off) for r, off, _, _ in rows], [r[2] for r in rows], [r[3] for r in rows])
        with open(os.path.join(path, "Header"), "w") as f:      # last: a complete Header implies complete data
            f.write(self.header_text())

    # ------------------------------------------------------------------------------------------------ reader
    @staticmethod
    def read(path, load_data=True):
        with open(os.path.join(path, "Header")) as f:
            T = f.read().split("\n")
        it = iter(T)
        version = next(it).strip()
        nc = int(next(it))
        names = [next(it).strip() for _ in range(nc)]
        dim = int(next(it))
        time = float(next(it))
        finest = int(next(it))
        prob_lo = tuple(float(v) for v in next(it).split())
        prob_hi = tuple(float(v) for v in next(it).split())
        ref_ratio = [int(v) for v in next(it).split()]
        doms = re.findall(r"\(\(([-\d,]+)\) \(([-\d,]+)\) \([-\d,]+\)\)", next(it))
        steps = [int(v) for v in next(it).split()]
        dxs = [tuple(float(v) for v in next(it).split()) for _ in range(finest + 1)]
        coord = int(next(it))
        next(it)
        levels = []
        for l in range(finest + 1):
            lev, ngrids, ltime = next(it).split()
            lstep = int(next(it))
            for _ in range(int(ngrids) * dim):
                next(it)
            rel = next(it).strip()
            dlo, dhi = (tuple(int(v) for v in s.split(",")) for s in doms[l])
            lv = Level((dlo, dhi), dxs[l], [], None, lstep, float(ltime))
            PlotFile._read_level(path, rel, lv, nc, load_data)
            levels.append(lv)
        return PlotFile(names, time, prob_lo, prob_hi, levels, ref_ratio, coord, version)

    @staticmethod
    def _read_level(path, rel, lv, nc, load_data):
        with open(os.path.join(path, rel + "_H")) as f:
            txt = f.read()
        boxes = re.findall(r"\(\(([-\d,]+)\) \(([-\d,]+)\) \([-\d,]+\)\)", txt)
        lv.boxes = [(tuple(int(v) for v in lo.split(",")), tuple(int(v) for v in hi.split(","))) for lo, hi in boxes]
        lv.fab_files = [(m.group(1), int(m.group(2))) for m in re.finditer(r"FabOnDisk: (\S+) (\d+)", txt)]
        assert len(lv.fab_files) == len(lv.boxes)
        if not load_data:
            return
        lv.data = []
        ld = os.path.dirname(os.path.join(path, rel))
        for (lo, hi), (fn, off) in zip(lv.boxes, lv.fab_files):
            with open(os.path.join(ld, fn), "rb") as f:
                f.seek(off)
                head = f.readline().decode()
                m = re.match(r"FAB \(\((\d+), \(([\d ]+)\)\),\((\d+), \(([\d ]+)\)\)\)", head)
                assert m and int(m.group(1)) == 8, head
                order = [int(v) for v in m.group(4).split()]
                little = order == [8, 7, 6, 5, 4, 3, 2, 1]
                assert little or order == [1, 2, 3, 4, 5, 6, 7, 8], head
                n = int(head.rsplit(" ", 1)[1])
                shape = tuple(h - q + 1 for q, h in zip(lo, hi)) + (n,)
                cnt = int(np.prod(shape))
                a = np.frombuffer(f.read(8 * cnt), dtype="<f8" if little else ">f8").reshape(shape, order="F")
                lv.data.append(a.astype(np.float64))


def comm_ops(world):
    """(allreduce(array, op), barrier()) of the library's communicator for the collective writers; one rank: nothing to do (and no
    library needed)"""
    if world == 1:
        return (lambda a, op=0: a), (lambda: None)
    from .lib import comm_allreduce, comm_barrier
    return comm_allreduce, comm_barrier


def write_collective(pf, path, owners, rank=0, world=1):
    """every rank of a run writes its part of plotfile `pf` (Level.owned / Level.data = what this rank holds; owners[l] = owner rank of
    every box of level l): rank 0 makes the directories -- barrier -- data files -- one sum per level carries offsets, minima and maxima
    to everyone (gather_meta) and orders the data before the headers -- rank 0 writes the headers.  Collective over the library's
    communicator (lib.comm_allreduce: RCCL or the callback transport alike)."""
    allreduce, barrier = comm_ops(world)
    if rank == 0:
        pf.make_dirs(path)
    barrier()
    meta = pf.write_data(path, rank)
    nc = len(pf.names)
    gathered = [gather_meta(len(lv.boxes), nc, meta[l], owners[l], allreduce) for l, lv in enumerate(pf.levels)]
    if rank == 0:
        ranks = sorted({r for g in gathered for r in g})
        pf.write_headers(path, {r: [g.get(r, []) for g in gathered] for r in ranks})
    barrier()


def compare(path_a, path_b):
    """fcompare role: {name: (abs Linf, rel Linf)} of the level-wise difference of two plotfiles with identical grids"""
    A, B = PlotFile.read(path_a), PlotFile.read(path_b)
    if A.names != B.names or len(A.levels) != len(B.levels):
        raise ValueError("plotfiles differ in variables or number of levels")
    out = {}
    for n, name in enumerate(A.names):
        ea, ma = 0.0, 0.0
        for la, lb in zip(A.levels, B.levels):
            if la.boxes != lb.boxes:
                raise ValueError("plotfiles differ in their grids")
            for a, b in zip(la.data, lb.data):
                ea = max(ea, float(np.abs(a[..., n] - b[..., n]).max()))
                ma = max(ma, float(np.abs(a[..., n]).max()))
        out[name] = (ea, ea / ma if ma > 0 else 0.0)
    return out


STATE_NAMES_3D = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer"]


def state_names(do_trac2=0, do_temp=0):
    """names of the State_Type components (NS_setup.cpp:250-283), then divu and dsdt (Divu_Type, Dsdt_Type) in a temperature run"""
    return STATE_NAMES_3D + (["tracer2"] if do_trac2 else []) + (["temp", "divu", "dsdt"] if do_temp else [])


DERIVE_NAMES = ["energy", "mag_vort", "avg_pressure"]          # derive_lst order (NS_setup.cpp:436-449; without particles and time averages)
# this library's own derived fields of the velocity-gradient tensor (csrc/k_velgrad.hip): amr.derive_plot_vars may name them; they are
# not part of upstream's derive list, so ALL does not expand to them
VELGRAD_NAMES = list(_pdf.VELGRAD_NAMES)
# with tracer particles (do_nspc, NS_setup.cpp:452-466): the two counts follow avg_pressure
PARTICLE_DERIVE_NAMES = ["particle_count", "total_particle_count"]


# "velocity_average" (NS_setup.cpp:412-431): one derived quantity of six plotfile components; declared only with ns.avg_interval > 0, and
# then in front of "energy"
VEL_AVG_NAMES = ["x_vel_average", "y_vel_average", "z_vel_average", "x_vel_rms", "y_vel_rms", "z_vel_rms"]


def plot_selection(state, plot_vars="ALL", derive_plot_vars="NONE", averaging=False, particles=False):
    """(indices of the state components, names of the derived quantities) a plotfile holds: amr.plot_vars picks state variables (ALL: every
    one), amr.derive_plot_vars derived ones (ALL: the derive list in its order; default NONE) -- Amr::initPltAndChk / fillDerivePlotVarList.
    Unknown names raise, as amrex::Amr aborts on them.  averaging (ns.avg_interval > 0): "velocity_average" exists, first in the derive
    list; it is returned as its six component names VEL_AVG_NAMES (run.level_arrays derives them together).  particles: a run with tracer
    particles also knows PARTICLE_DERIVE_NAMES, after avg_pressure.  A list may also name the velocity-gradient fields VELGRAD_NAMES."""
    known = (["velocity_average"] if averaging else []) + DERIVE_NAMES + (PARTICLE_DERIVE_NAMES if particles else [])

    def expand(names):
        return [c for nm in names for c in (VEL_AVG_NAMES if nm == "velocity_average" else [nm])]
    if plot_vars == "ALL":
        keep = list(range(len(state)))
    elif plot_vars == "NONE":
        keep = []
    else:
        bad = [v for v in plot_vars if v not in state]
        if bad:
            raise ValueError(f"amr.plot_vars: not state variables: {bad} (have {state})")
        keep = [q for q, nm in enumerate(state) if nm in plot_vars]           # plotfile order = state order (Amr::statePlotVars is a list filled in descriptor order)
    if derive_plot_vars == "ALL":
        der = expand(known)                 # (upstream's derive list: without VELGRAD_NAMES)
    elif derive_plot_vars == "NONE":
        der = []
    else:
        bad = [v for v in derive_plot_vars if v not in known + VELGRAD_NAMES]
        if bad:
            raise ValueError(f"amr.derive_plot_vars: unknown derived quantities {bad} (have {known + VELGRAD_NAMES})")
        der = expand(derive_plot_vars)
    return keep, der


def from_level_data(geom_n, prob_lo, prob_hi, boxes, arrays, time, step, names=None):
    """single-level PlotFile from per-box arrays (valid region, (nx,ny,nz,ncomp))"""
    dim = len(geom_n)
    dx = [(prob_hi[d] - prob_lo[d]) / geom_n[d] for d in range(dim)]
    lv = Level(((0,) * dim, tuple(v - 1 for v in geom_n)), dx, boxes, arrays, step, time)
    return PlotFile(names or STATE_NAMES_3D, time, prob_lo, prob_hi, [lv])
