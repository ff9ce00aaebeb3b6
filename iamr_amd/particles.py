"""Tracer particles: the ctypes view of iamrx_particles_* (include/iamrx.h; csrc/k_particles.hip) and the host-side particle files.

The container follows AMReX's AmrTracerParticleContainer as IAMR uses it (reference Source/NavierStokesBase.cpp:198-222, 3751-4057).  AMReX
is not part of the reference tree, so the container's arithmetic is UNPINNED; tests/particles_numpy.py restates
what is implemented.

Files (no device needed):
  read_particle_file   the reference's ASCII `particle_file`: a count on the first line, then one position per line
  write_ascii          particles.particle_output_file: the count, then `x y z id cpu` per line, %.17g, sorted by id
  write_particles_dir / read_particles_dir
                       the `Particles/` directory of a checkpoint or plotfile -- THIS project's own format,
                       not AMReX's binary particle format: a text `Header` and raw little-endian arrays.  One rank writes format 1
                       (`iamr_amd-particles-1`); several ranks write format 2: every rank its own arrays, rank 0 the Header last

Several ranks: Particles.add / redistribute / count_global / total_particle_count and save / restore / gather_sorted below are COLLECTIVE
(every rank calls them); count / read / set_positions / sample / timestamp speak of this rank's particles (include/iamrx.h).

Timestamp files (NavierStokesBase::post_timestep_particle, NavierStokesBase.cpp:3881-3951): after set_timestamp(basename, indices) the steps of
the level or hierarchy the container is attached to append `id cpu x y z time r0 r1 r2 v..` per particle to <basename>_NN (NN: the rank),
v the state components `indices` interpolated to the particle (Particles.sample; tests/timestamp_numpy.py restates it).
"""
import ctypes as C
import os
import numpy as np
from .lib import lib, check

PARTICLES_DIR = "Particles"          # the_ns_particle_file_name, NavierStokesBase.cpp:209
_HEADER_MAGIC = "iamr_amd-particles-1"
_HEADER_MAGIC_2 = "iamr_amd-particles-2"          # several writers: the arrays of writer q are <name>.<q:05d>
_FILES = (("xyz.f64", "<f8", 3), ("r.f64", "<f8", 3), ("id.i32", "<i4", 1), ("cpu.i32", "<i4", 1))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


class Particles:
    """device-resident tracer particles on the levels (geoms[l], layouts[l]), coarsest first; attach with NavierStokes.set_particles or
    Amr.set_particles, which rebinds the container to that object's boxes"""

    def __init__(self, geoms, layouts, ratio=2):
        geoms, layouts = list(geoms), list(layouts)
        if len(geoms) != len(layouts) or not geoms:
            raise ValueError("Particles: one geometry per layout, at least one level")
        from .lib import Geom
        ga = (Geom * len(geoms))(*geoms)
        la = (C.c_void_p * len(layouts))(*[l.h for l in layouts])
        self._keep = (geoms, layouts)
        self.h = C.c_void_p()
        check(lib().iamrx_particles_create(len(geoms), ga, la, int(ratio), C.byref(self.h)))

    @staticmethod
    def for_run(run):
        """a container on the levels of a NavierStokes level or an Amr hierarchy"""
        return Particles([run.level_geom(l) for l in range(run.nlev)], run.layouts, run.ratio)

    for_level = for_hierarchy = for_run

    def add(self, xyz, ids=None, r=None, cpus=None):
        """add particles at the positions xyz (n, 3) -- an empty list is fine; ids default to the container's counter (from 1).  Returns the
        number of particles removed because they lie outside a non-periodic domain.  Several ranks: collective; every rank passes its own
        list and the particles go to the owners of their boxes; without ids rank q's new ids follow rank q - 1's."""
        x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
        n = x.shape[0]
        if n == 0:
            x, ids, cpus, r = None, None, None, None
        i = None if ids is None else np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(n))
        c = None if cpus is None else np.ascontiguousarray(np.asarray(cpus, dtype=np.int32).reshape(n))
        rr = None if r is None else np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(n, 3))
        rm = C.c_long()
        check(lib().iamrx_particles_add(self.h, C.c_long(n), _dp(x), _dp(rr), _ip(i), _ip(c), C.byref(rm)))
        return rm.value

    def _counts(self):
        per = (C.c_long * 8)()
        tot, rm, nid = C.c_long(), C.c_long(), C.c_int()
        check(lib().iamrx_particles_count(self.h, per, C.byref(tot), C.byref(nid), C.byref(rm)))
        return list(per), tot.value, nid.value, rm.value

    def count(self, lev=None):
        """number of particles (on level lev)"""
        per, tot, _, _ = self._counts()
        return tot if lev is None else per[lev]

    def count_global(self, lev=None):
        """number of particles on all ranks (on level lev); collective"""
        per = (C.c_long * 8)()
        tot = C.c_long()
        check(lib().iamrx_particles_count_global(self.h, per, C.byref(tot)))
        return tot.value if lev is None else per[lev]

    @property
    def next_id(self):
        return self._counts()[2]

    @next_id.setter
    def next_id(self, v):
        check(lib().iamrx_particles_set_next_id(self.h, int(v)))

    @property
    def removed(self):
        """particles removed beyond non-periodic domain faces so far"""
        return self._counts()[3]

    def set_fixed_dir(self, d):
        check(lib().iamrx_particles_set_fixed_dir(self.h, int(d)))

    def read(self):
        """-> dict(xyz (n, 3), r (n, 3), id, cpu, level, box) in storage order (grouped by level and box)"""
        n = self.count()
        out = dict(xyz=np.zeros((n, 3)), r=np.zeros((n, 3)), id=np.zeros(n, np.int32), cpu=np.zeros(n, np.int32), level=np.zeros(n, np.int32),
                   box=np.zeros(n, np.int32))
        if n:
            check(lib().iamrx_particles_read(self.h, _dp(out["xyz"]), _dp(out["r"]), _ip(out["id"]), _ip(out["cpu"]), _ip(out["level"]), _ip(out["box"])))
        return out

    def read_sorted(self):
        """read(), sorted by id"""
        d = self.read()
        o = np.argsort(d["id"], kind="stable")
        return {k: v[o] for k, v in d.items()}

    def set_positions(self, xyz):
        """overwrite the positions, in the storage order of read(); follow with redistribute()"""
        x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
        if x.shape[0] != self.count():
            raise ValueError("set_positions: one position per particle")
        check(lib().iamrx_particles_set_positions(self.h, _dp(x)))

    def advect(self, lev, umac, dt):
        """AdvectWithUmac for the particles of level lev on the caller's face MultiFabs umac[0..2]"""
        check(lib().iamrx_particles_advect(self.h, int(lev), umac[0].h, umac[1].h, umac[2].h, C.c_double(dt)))

    def redistribute(self, lev_min=0, lev_max=None, ngrow=0):
        rm = C.c_long()
        check(lib().iamrx_particles_redistribute(self.h, int(lev_min), 1000 if lev_max is None else int(lev_max), int(ngrow), C.byref(rm)))
        return rm.value

    def particle_count(self, lev, out, ocomp=0):
        check(lib().iamrx_particles_derive_count(self.h, 0, int(lev), out.h, int(ocomp)))

    def total_particle_count(self, lev, out, ocomp=0):
        check(lib().iamrx_particles_derive_count(self.h, 1, int(lev), out.h, int(ocomp)))

    def sample(self, lev, mf, comps):
        """the components `comps` of the cell-centred MultiFab mf (on the level's boxes, ghost cells filled) at the particles of level lev,
        this rank's, in storage order -> dict(id, cpu, values (n, M)); trilinear between cell centres (include/iamrx.h)"""
        c = np.ascontiguousarray(np.asarray(comps, dtype=np.int32).reshape(-1))
        n = self.count(lev)
        out = dict(id=np.zeros(n, np.int32), cpu=np.zeros(n, np.int32), values=np.zeros((n, len(c))))
        check(lib().iamrx_particles_sample(self.h, int(lev), mf.h, len(c), _ip(c), _dp(out["values"]), _ip(out["id"]), _ip(out["cpu"])))
        return out

    def set_timestamp(self, basename, indices=()):
        """timestamp files <basename>_NN with the state components `indices` sampled at the particles; basename None or "": off"""
        c = np.ascontiguousarray(np.asarray(list(indices), dtype=np.int32).reshape(-1))
        check(lib().iamrx_particles_set_timestamp(self.h, os.fsencode(basename) if basename else None, len(c), _ip(c) if len(c) else None))

    def timestamp(self, lev, mf, time):
        """append the records of this rank's particles of level lev (mf: the sampled components, or None)"""
        check(lib().iamrx_particles_timestamp(self.h, int(lev), None if mf is None else mf.h, C.c_double(time)))

    def __del__(self):
        try:
            if self.h:
                lib().iamrx_particles_destroy(self.h)
        except Exception:
            pass


# ---- files (host only) --------------------------------------------------------------------------------------------------------------------
def read_particle_file(path, slab_y=None):
    """positions of the reference's ASCII particle file (InitFromAsciiFile with no extra data): the count, then one position per line.
    Three numbers per line, or two for a two-dimensional file: (x, y) lifts to (x, slab_y, y) like inputs.lift_2d (slab_y: the mid-slab
    coordinate).  -> (n, 3) float64"""
    with open(path) as f:
        tok = f.read().split("\n")
    lines = [t.split() for t in tok if t.strip()]
    if not lines or len(lines[0]) != 1:
        raise ValueError(f"{path}: the first line must hold the number of particles")
    n = int(lines[0][0])
    if len(lines) - 1 < n:
        raise ValueError(f"{path}: {n} particles announced, {len(lines) - 1} lines follow")
    rows = lines[1:1 + n]
    dim = {len(r) for r in rows}
    if n and dim not in ({2}, {3}):
        raise ValueError(f"{path}: every line must hold two or three coordinates")
    out = np.zeros((n, 3))
    for q, r in enumerate(rows):
        v = [float(s) for s in r]
        if len(v) == 2:
            if slab_y is None:
                raise ValueError(f"{path}: two-dimensional positions in a three-dimensional run")
            out[q] = (v[0], slab_y, v[1])
        else:
            if slab_y is not None:
                raise ValueError(f"{path}: three-dimensional positions in a two-dimensional run")
            out[q] = v
    return out


def write_ascii(path, xyz, ids, cpus):
    """particles.particle_output_file: the count, then `x y z id cpu` per particle with %.17g, sorted by id"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    ids, cpus = np.asarray(ids).reshape(-1), np.asarray(cpus).reshape(-1)
    o = np.argsort(ids, kind="stable")
    with open(path, "w") as f:
        f.write(f"{len(ids)}\n")
        for q in o:
            f.write("%.17g %.17g %.17g %d %d\n" % (xyz[q, 0], xyz[q, 1], xyz[q, 2], ids[q], cpus[q]))


def read_ascii(path):
    """what write_ascii wrote -> (xyz, ids, cpus)"""
    with open(path) as f:
        n = int(f.readline())
        rows = [f.readline().split() for _ in range(n)]
    xyz = np.array([[float(v) for v in r[:3]] for r in rows], dtype=np.float64).reshape(n, 3)
    return xyz, np.array([int(r[3]) for r in rows], np.int32), np.array([int(r[4]) for r in rows], np.int32)


def _sorted_arrays(xyz, r, ids, cpus):
    ids = np.asarray(ids, np.int32).reshape(-1)
    o = np.argsort(ids, kind="stable")
    return (np.asarray(xyz, np.float64).reshape(-1, 3)[o], np.asarray(r, np.float64).reshape(-1, 3)[o], ids[o], np.asarray(cpus, np.int32).reshape(-1)[o])


def write_particles_dir(parent, xyz, r, ids, cpus, next_id, rank=0, world=1, counts=None):
    """<parent>/Particles/, this project's own format.  world 1: `Header` (text: magic, count, next id, then one line `file dtype columns`
    per array) and the raw little-endian arrays, sorted by id.  world > 1 (format 2): the caller is writer `rank` of `world` and passes its
    own particles; it writes them, sorted by id, to <file>.<rank:05d>; counts: the number of particles of every writer, which rank 0 needs
    for the Header (magic, total count, next id, the number of writers, their counts on one line, then the array lines) -- to be called by
    rank 0 LAST, after every other writer has finished (save() below does that through the communicator; a caller without one calls the
    writers one after another, rank 0 at the end)."""
    d = os.path.join(parent, PARTICLES_DIR)
    os.makedirs(d, exist_ok=True)
    arrs = _sorted_arrays(xyz, r, ids, cpus)
    n = len(arrs[2])
    if world == 1:
        with open(os.path.join(d, "Header"), "w") as f:
            f.write(f"{_HEADER_MAGIC}\n{n}\n{int(next_id)}\n")
            for name, dt, nc in _FILES:
                f.write(f"{name} {dt} {nc}\n")
        for (name, dt, nc), a in zip(_FILES, arrs):
            np.ascontiguousarray(a).astype(dt).tofile(os.path.join(d, name))
        return d
    if not 0 <= rank < world:
        raise ValueError(f"write_particles_dir: writer {rank} of {world}")
    for (name, dt, nc), a in zip(_FILES, arrs):
        np.ascontiguousarray(a).astype(dt).tofile(os.path.join(d, f"{name}.{rank:05d}"))
    if rank == 0:
        counts = [int(c) for c in counts]
        if len(counts) != world or counts[0] != n:
            raise ValueError(f"write_particles_dir: {world} writers, counts {counts}, writer 0 holds {n}")
        with open(os.path.join(d, "Header"), "w") as f:
            f.write(f"{_HEADER_MAGIC_2}\n{sum(counts)}\n{int(next_id)}\n{world}\n{' '.join(str(c) for c in counts)}\n")
            for name, dt, nc in _FILES:
                f.write(f"{name} {dt} {nc}\n")
    return d


def _read_arrays(d, lines, n, suffix=""):
    out = {}
    for line, key in zip(lines, ("xyz", "r", "id", "cpu")):
        name, dt, nc = line.split()
        a = np.fromfile(os.path.join(d, name + suffix), dtype=dt)
        if a.size != n * int(nc):
            raise ValueError(f"{d}/{name}{suffix}: {a.size} values, the header announces {n} x {nc}")
        out[key] = a.reshape(n, 3).astype(np.float64) if int(nc) == 3 else a.astype(np.int32)
    return out


def read_particles_dir(parent, rank=0, world=1):
    """-> dict(xyz, r, id, cpu, next_id) of <parent>/Particles/, either format: the share of reader `rank` of `world`.  Format 2: the files
    of the writers q with q % world == rank, one after another; format 1: the rank-th of `world` contiguous slices.  The shares of all
    readers are disjoint and together they are everything; world 1 reads everything."""
    if not 0 <= rank < world:
        raise ValueError(f"read_particles_dir: reader {rank} of {world}")
    d = os.path.join(parent, PARTICLES_DIR)
    with open(os.path.join(d, "Header")) as f:
        lines = [l.strip() for l in f if l.strip()]
    if lines[0] not in (_HEADER_MAGIC, _HEADER_MAGIC_2):
        raise ValueError(f"{d}/Header: not a particle directory of this project ({lines[0]!r})")
    n, next_id = int(lines[1]), int(lines[2])
    if lines[0] == _HEADER_MAGIC:
        out = _read_arrays(d, lines[3:], n)
        lo, hi = (n * rank) // world, (n * (rank + 1)) // world
        out = {k: v[lo:hi] for k, v in out.items()}
    else:
        writers, counts = int(lines[3]), [int(v) for v in lines[4].split()]
        if len(counts) != writers or sum(counts) != n:
            raise ValueError(f"{d}/Header: {writers} writers with counts {counts}, {n} particles announced")
        parts = [_read_arrays(d, lines[5:], counts[q], f".{q:05d}") for q in range(writers) if q % world == rank]
        empty = dict(xyz=np.zeros((0, 3)), r=np.zeros((0, 3)), id=np.zeros(0, np.int32), cpu=np.zeros(0, np.int32))
        out = {k: np.concatenate([p[k] for p in parts]) if parts else empty[k] for k in empty}
    out["next_id"] = next_id
    return out


def _rank_counts(n):
    """(rank, world, the number n of every rank); the allreduce is also the barrier between the ranks' file writes"""
    from .lib import comm_rank, comm_allreduce
    rank, world = comm_rank()
    v = np.zeros(world)
    v[rank] = float(n)
    if world > 1:
        v = comm_allreduce(v, 0)
    return rank, world, [int(c) for c in v]


def save(parent, pc):
    """the container's particles into <parent>/Particles/.  Several ranks: collective -- every rank writes its own, rank 0 the Header once
    all have written (plotfile.write_collective's order)."""
    from .lib import comm_barrier
    p = pc.read()
    next_id = pc.next_id
    rank, world, counts = _rank_counts(len(p["id"]))
    if world == 1:
        return write_particles_dir(parent, p["xyz"], p["r"], p["id"], p["cpu"], next_id)
    if rank == 0:
        os.makedirs(os.path.join(parent, PARTICLES_DIR), exist_ok=True)
    comm_barrier()                                      # the directory exists
    if rank != 0:
        write_particles_dir(parent, p["xyz"], p["r"], p["id"], p["cpu"], next_id, rank, world)
    comm_barrier()                                      # the others have written
    if rank == 0:
        write_particles_dir(parent, p["xyz"], p["r"], p["id"], p["cpu"], next_id, 0, world, counts)
    comm_barrier()                                      # the Header is there
    return os.path.join(parent, PARTICLES_DIR)


def restore(parent, pc):
    """add the particles of <parent>/Particles/ to the (empty) container, bit for bit, with the id counter.  Several ranks: collective;
    every rank adds its share (read_particles_dir) and the container sends the particles to the owners of their boxes, so a directory
    written on any number of ranks restores on any other."""
    from .lib import comm_rank
    rank, world = comm_rank()
    d = read_particles_dir(parent, rank, world)
    pc.add(d["xyz"], ids=d["id"], r=d["r"], cpus=d["cpu"])
    pc.next_id = d["next_id"]


def gather_sorted(pc):
    """-> (xyz, id, cpu) of ALL particles, sorted by id, on every rank; collective.  Every rank puts its rows at its offset into a zero
    array and the arrays are summed (exact: every entry has one non-zero term; ids and cpus are 32-bit integers held as doubles).  For
    small sets: every rank holds everything."""
    from .lib import comm_allreduce
    p = pc.read()
    rank, world, counts = _rank_counts(len(p["id"]))
    if world == 1:
        o = np.argsort(p["id"], kind="stable")
        return p["xyz"][o], p["id"][o], p["cpu"][o]
    off = sum(counts[:rank])
    a = np.zeros((sum(counts), 5))
    a[off:off + counts[rank], :3] = p["xyz"]
    a[off:off + counts[rank], 3] = p["id"]
    a[off:off + counts[rank], 4] = p["cpu"]
    a = comm_allreduce(a, 0) if a.size else a
    o = np.argsort(a[:, 3], kind="stable")
    return a[o, :3].copy(), a[o, 3].astype(np.int32), a[o, 4].astype(np.int32)
