"""GPU: tracer particles on several ranks (ranks sharing the one GPU over the gloo callback transport:
tests/ranks.py): placement against the global box list, migration, collective errors, counts, particle files and restart.

Two parts, ONE spawn per world size (1, 2, 3) serving both:
A. the container on caller-owned arrays: 16^3 in eight 8^3 boxes dealt round robin, periodic in x and y, walls in z, one patch (coarse
   cells 4 .. 11) in two fine boxes of different owners (on three ranks rank 0 owns none of them).  Yardstick: tests/particles_numpy.py on the
   GLOBAL box list; across world sizes the results are compared by id TO THE BIT (a particle's arithmetic does not depend on its owner).
B. runs through iamr_amd.run.main: against one rank within 1e-8 modulo the period (the bound tests/test_gpu_dist.py gives the state of a
   hierarchy run on several ranks; a particle moved with a stale ghost face is off by about 1e-3), restart on the same rank count to the bit.
A fourth spawn (2 ranks) repeats one run of B in the library's default box mode (IAMRX_COALESCE=1: the level objects merge a rank's boxes)."""
import os
import numpy as np
import pytest
import ranks
from ranks import free_port

import particles_numpy as pn

pytestmark = [pytest.mark.gpu, pytest.mark.boxes_kept]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL_RUN = 1e-8

# ---- part A: geometry ------------------------------------------------------------------------------------------------------------------
N0 = (16, 16, 16)
PLO, PHI = (0.0, 0.0, 0.0), (2.0, 1.5, 1.0)
PER = (1, 1, 0)
DX0 = tuple((PHI[e] - PLO[e]) / N0[e] for e in range(3))
DX1 = tuple(0.5 * d for d in DX0)
BOXES0 = [((i, j, k), (i + 7, j + 7, k + 7)) for k in (0, 8) for j in (0, 8) for i in (0, 8)]
BOXES1 = [((8, 8, 8), (15, 23, 23)), ((16, 8, 8), (23, 23, 23))]          # the refinement of coarse cells 4 .. 11, cut in x
PATCH_LO = tuple(8 * DX1[e] for e in range(3))
PATCH_HI = tuple(24 * DX1[e] for e in range(3))
DT = 0.03            # max |u| < 1: nobody moves further than a fine cell (1 / 32), the one ghost face of either level suffices


def owners(world):
    return [q % world for q in range(8)], [1 % world, 2 % world]


def levels():
    return [dict(n=N0, dlo=(0, 0, 0), dx=DX0, boxes=BOXES0), dict(n=tuple(2 * n for n in N0), dlo=(0, 0, 0), dx=DX1, boxes=BOXES1)]


def start_positions():
    """about 2 000 positions from a fixed seed: random ones plus positions within 1e-12 of box faces, patch faces and domain faces"""
    rng = np.random.default_rng(11)
    span = np.array(PHI) - np.array(PLO)
    x = rng.uniform(0.0, 1.0, size=(1700, 3)) * span
    faces = [(0, 1.0), (1, 0.75), (2, 0.5), (0, PATCH_LO[0]), (0, PATCH_HI[0]), (1, PATCH_LO[1]), (1, PATCH_HI[1]), (2, PATCH_LO[2]), (2, PATCH_HI[2]),
             (0, 0.0), (0, 2.0), (1, 0.0), (1, 1.5), (2, 0.0), (2, 1.0)]
    extra = []
    for e, c in faces:
        for s in (-1e-12, 1e-12, -3e-13, 0.0):
            q = rng.uniform(0.0, 1.0, size=(5, 3)) * span
            q[:, e] = c + s
            extra.append(q)
    return np.concatenate([x] + extra)


def umac_formula(d, lev, idx):
    """face velocity of component d at the face indices idx (three 1-d integer arrays) of level lev: one closed formula of the INDEX, so
    that every rank fills the same numbers into a box whoever owns it; periodic in x and y through the index modulo the level's extent"""
    n = [N0[e] * 2 ** lev for e in range(3)]
    ph = []
    for e in range(3):
        pos = idx[e] + (0.0 if e == d else 0.5)
        if PER[e]:
            pos = np.mod(pos, n[e])
        ph.append(2.0 * np.pi * pos / n[e])
    X, Y, Z = np.meshgrid(*ph, indexing="ij")
    return (0.35 * np.cos(X + 2.0 * Y + 0.7 * d) * np.cos(0.5 * Z + 0.3) + 0.25 * np.sin(2.0 * X - Y + Z + d) + (0.2, -0.15, -0.3)[d])


def pushed(xyz, ids, lev):
    """part A check 3: every second particle of level 1 goes up to 1.5 fine cells outside the patch, through a face picked by its id"""
    x = xyz.copy()
    for q in np.nonzero((lev == 1) & (ids % 2 == 0))[0]:
        i = int(ids[q])
        e, side, amt = i % 3, (i // 3) % 2, 0.02 + 1.46 * ((i * 37) % 100) / 100.0
        x[q, e] = (PATCH_HI[e] + amt * DX1[e]) if side else (PATCH_LO[e] - amt * DX1[e])
    return x


# ---- the rank processes ------------------------------------------------------------------------------------------------------------------
def _state(pc, lays):
    """this rank's particles with the GLOBAL box index"""
    d = pc.read()
    g = [[lays[l].local_box(li)[2] for li in range(lays[l].nlocal())] for l in range(2)]
    d["gbox"] = np.array([g[int(l)][int(b)] for l, b in zip(d["level"], d["box"])], dtype=np.int64)
    return d


def container_checks(rank, world, out_dir):
    """part A on this rank; what the tests compare goes to <out_dir>/A_w<world>_r<rank>.npz"""
    from iamr_amd import lib
    from iamr_amd.particles import Particles
    o0, o1 = owners(world)
    g0, g1 = lib.Geom.make(N0, PLO, PHI, PER), lib.Geom.make(tuple(2 * n for n in N0), PLO, PHI, PER)
    lays = (lib.Layout(BOXES0, o0), lib.Layout(BOXES1, o1))
    out = {}

    def keep(tag, d):
        out.update({f"{tag}_{k}": v for k, v in d.items()})

    x0 = start_positions()
    # 1. add: a third (a world-th) on each rank without ids; then everything on rank 0
    part = np.array_split(np.arange(len(x0)), world)[rank]
    pc3 = Particles([g0, g1], lays, 2)
    rm3 = pc3.add(x0[part])
    keep("add3", _state(pc3, lays))
    out["add3_meta"] = np.array([rm3, pc3.next_id, pc3.count_global(), pc3.removed, pc3.count_global(0), pc3.count_global(1)])
    del pc3
    pc = Particles([g0, g1], lays, 2)
    rm = pc.add(x0 if rank == 0 else np.zeros((0, 3)))
    keep("add0", _state(pc, lays))
    out["add0_meta"] = np.array([rm, pc.next_id, pc.count_global(), pc.removed, pc.count_global(0), pc.count_global(1)])
    # 2. advect both levels with the analytic u_mac (one ghost face), then redistribute(0, 1, 0)
    faces = []                                         # (kept until the stream has been drained by the read below)
    for l, lay in enumerate(lays):
        um = [lib.MultiFab(lay, lib.face(d), 1, 1) for d in range(3)]
        faces.append(um)
        for d in range(3):
            for li in range(um[d].nlocal()):
                lo, hi = um[d].fab_box(li)
                um[d].from_numpy(umac_formula(d, l, [np.arange(lo[e], hi[e] + 1) for e in range(3)])[..., None], li)
        pc.advect(l, um, DT)
    keep("moved", _state(pc, lays))                    # advected, not yet redistributed
    rm = pc.redistribute(0, 1, 0)
    keep("adv", _state(pc, lays))
    out["adv_meta"] = np.array([rm, pc.next_id, pc.count_global(), pc.removed, pc.count_global(0), pc.count_global(1)])
    # 3. grown boxes
    s = pc.read()
    pc.set_positions(pushed(s["xyz"], s["id"], s["level"]))
    keep("pushed", _state(pc, lays))
    rm = pc.redistribute(1, 1, 2)
    keep("grown", _state(pc, lays))
    out["grown_meta"] = np.array([rm, pc.next_id, pc.count_global(), pc.removed, pc.count_global(0), pc.count_global(1)])
    # 4. counts on this rank's boxes
    for l, lay in enumerate(lays):
        for which, name in ((0, "pcount"), (1, "tcount")):
            m = lib.MultiFab(lay, lib.CELL, 1, 0)
            (pc.particle_count if which == 0 else pc.total_particle_count)(l, m)
            for li in range(lay.nlocal()):
                out[f"{name}_l{l}_b{lay.local_box(li)[2]}"] = m.to_numpy(li)[0][..., 0]
    pc.redistribute(0, 1, 0)                           # everybody back into a valid box
    # 5. collective error: the owner of fine box 0 sends its first level-1 particle far from the patch; redistribute(1, 1, 1) cannot place it
    s = pc.read()
    x = s["xyz"].copy()
    if rank == o1[0]:
        q = int(np.nonzero(s["level"] == 1)[0][0])
        x[q] = (0.05, 0.05, 0.05)
        out["err_id"] = np.array([s["id"][q]])
    pc.set_positions(x)
    before = pc.read()
    try:
        pc.redistribute(1, 1, 1)
        msg = ""
    except lib.IamrxError as e:
        msg = str(e)
    after = pc.read()
    out["err_msg"] = np.array([msg])
    out["err_unchanged"] = np.array([all(np.array_equal(before[k], after[k]) for k in before)])
    rm = pc.redistribute(0, 1, 0)                      # the next valid collective call works, and the particle drops to level 0
    keep("after_err", _state(pc, lays))
    out["after_err_meta"] = np.array([rm, pc.next_id, pc.count_global(), pc.removed, pc.count_global(0), pc.count_global(1)])
    np.savez(os.path.join(out_dir, f"A_w{world}_r{rank}.npz"), **out)


def group_ranks(rank, world, port_a, ports, jobs, out_dir, group, with_container, merge):
    """one rank of a spawned group: part A (its own process group), then R.main once per job"""
    if with_container:
        ranks.start_rank(rank, world, port_a, merge)
        container_checks(rank, world, out_dir)
        ranks.stop_rank()
    else:
        ranks.rank_env(rank, world, merge=merge)
    ranks.run_jobs(rank, ports, jobs, out_dir, group)


def run_group(world, jobs, out_dir, group, with_container=True, merge=False):
    ranks.spawn(group_ranks, world, free_port(), [free_port() for _ in jobs], jobs, out_dir, group, with_container, merge)


# ---- part B: the runs ----------------------------------------------------------------------------------------------------------------------
def _particle_file(path, n_side, seed):
    """n_side^3 jittered lattice points in the unit cube, the reference's ASCII particle file"""
    rng = np.random.default_rng(seed)
    c = (np.arange(n_side) + 0.5) / n_side
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1) + rng.uniform(-0.3, 0.3, (n_side ** 3, 3)) / n_side
    with open(path, "w") as f:
        f.write(f"{len(x)}\n")
        for p in x:
            f.write("%.17g %.17g %.17g\n" % tuple(p))
    return x


def _amr(d, tag, p512):
    return [os.path.join(GOLD, "inputs.3d.taylorgreen_amr16"), f"particles.particle_init_file={p512}", "particles.particles_in_plotfile=1", "particles.verbose=1",
            "amr.derive_plot_vars=particle_count total_particle_count", "amr.check_int=1", "max_step=2", f"amr.plot_file={d}/plt{tag}_",
            f"amr.check_file={d}/chk{tag}_"]


def _rst(d, tag, frm, p512, extra=()):
    return _amr(d, tag, p512) + [f"amr.restart={d}/chk{frm}_00001"] + list(extra)


def _regrid(d, tag, p64):
    return [os.path.join(GOLD, "inputs.3d.tracer_regrid16"), f"particles.particle_init_file={p64}", "particles.verbose=1", "max_step=2", "amr.plot_int=-1",
            "amr.check_int=2", f"amr.check_file={d}/rg{tag}_"]


def _single(d, tag, p64):
    return [os.path.join(GOLD, "inputs.3d.taylorgreen"), "amr.n_cell=16 16 16", "amr.max_grid_size=8", "amr.max_level=0", f"particles.particle_init_file={p64}",
            "max_step=2", "amr.plot_int=-1", "amr.check_int=2", f"amr.check_file={d}/sl{tag}_"]


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("particles_multirank"))
    _particle_file(os.path.join(d, "p512.txt"), 8, 5)
    _particle_file(os.path.join(d, "p64.txt"), 4, 6)
    return d


@pytest.fixture(scope="module")
def two_ranks(out_dir):
    """2 ranks: part A; the full run C, its restart D from step 1 (with particles.particle_output_file), the regridding and the
    single-level run"""
    d = out_dir
    p512, p64 = f"{d}/p512.txt", f"{d}/p64.txt"
    run_group(2, [_amr(d, "C", p512), _rst(d, "D", "C", p512, [f"particles.particle_output_file={d}/ascii_D.txt"]), _regrid(d, "2", p64), _single(d, "2", p64)], d, "two")
    return d


@pytest.fixture(scope="module")
def one_rank(two_ranks):
    d = two_ranks
    p512, p64 = f"{d}/p512.txt", f"{d}/p64.txt"
    run_group(1, [_amr(d, "A", p512), _rst(d, "E", "C", p512), _regrid(d, "1", p64), _single(d, "1", p64)], d, "one")
    return d


@pytest.fixture(scope="module")
def three_ranks(one_rank):
    d = one_rank
    p512 = f"{d}/p512.txt"
    run_group(3, [_amr(d, "B", p512), _rst(d, "F", "C", p512)], d, "three")
    return d


@pytest.fixture(scope="module")
def all_worlds(three_ranks):
    return three_ranks


# ---- part A: the checks ----------------------------------------------------------------------------------------------------------------------
def _load(d, world):
    return [np.load(os.path.join(d, f"A_w{world}_r{r}.npz")) for r in range(world)]


def _union(Z, tag):
    """the ranks' particles of one stage, sorted by id; `rank` says who held each"""
    keys = ("xyz", "r", "id", "cpu", "level", "box", "gbox")
    cat = {k: np.concatenate([z[f"{tag}_{k}"] for z in Z]) for k in keys}
    cat["rank"] = np.concatenate([np.full(len(z[f"{tag}_id"]), r) for r, z in enumerate(Z)])
    o = np.argsort(cat["id"], kind="stable")
    return {k: v[o] for k, v in cat.items()}


def _owned_right(u, world):
    """every particle once, on the rank that owns its box, under that rank's local index of the box"""
    assert len(set(u["id"].tolist())) == len(u["id"])
    own = owners(world)
    for l in (0, 1):
        sel = u["level"] == l
        o = np.array(own[l])
        assert np.array_equal(u["rank"][sel], o[u["gbox"][sel]])
        local = np.array([sum(1 for b in range(g) if own[l][b] == own[l][g]) for g in range(len(own[l]))])
        assert np.array_equal(u["box"][sel], local[u["gbox"][sel]])


def _yardstick(ids, x, lev, gbox, lev_min, lev_max, ngrow):
    return pn.redistribute(x, ids, lev, gbox, levels(), PLO, PHI, PER, lev_min, lev_max, ngrow)


@pytest.fixture(scope="module")
def container(all_worlds):
    return {w: _load(all_worlds, w) for w in (1, 2, 3)}


@pytest.mark.parametrize("world", [1, 2, 3])
def test_add_places_on_the_owner(container, world):
    """check 1: everything on rank 0, and a share on each rank without ids: every particle once, on the owner of the box the yardstick
    names; ids 1 .. n in the documented order (rank q's follow rank q - 1's: the input order); next_id equal on all ranks"""
    Z = container[world]
    x0 = start_positions()
    n = len(x0)
    ex, el, eb, st = _yardstick(np.arange(1, n + 1), x0, np.zeros(n, int), np.zeros(n, int), 0, 1, 0)
    kept = st == 0
    assert (st == 1).sum() >= 5 and not (st == 2).any() and (el[kept] == 1).sum() > 100
    for tag in ("add0", "add3"):
        u = _union(Z, tag)
        _owned_right(u, world)
        assert np.array_equal(u["id"], np.nonzero(kept)[0] + 1)                     # particle j of the input order has id j + 1
        assert np.array_equal(u["xyz"], ex[kept]) and np.array_equal(u["level"], el[kept]) and np.array_equal(u["gbox"], eb[kept])
        for z in Z:
            assert list(z[f"{tag}_meta"]) == [int((st == 1).sum()), n + 1, int(kept.sum()), int((st == 1).sum()), int((el[kept] == 0).sum()), int((el[kept] == 1).sum())]
    if world == 3:
        assert not (container[3][0]["add0_level"] == 1).any() and (container[3][0]["add0_level"] == 0).any()      # rank 0 owns no fine box


@pytest.mark.parametrize("world", [1, 2, 3])
def test_advect_and_redistribute(container, world):
    """check 2: by id, position, r, level and global box equal the one-rank result to the bit; what was removed through the z walls and
    where everything went is what the yardstick says of the advected positions"""
    Z, ref = container[world], _union(container[1], "adv")
    m = _union(Z, "moved")
    assert np.abs(m["xyz"] - _union(Z, "add0")["xyz"]).max() > 1e-3
    ex, el, eb, st = _yardstick(m["id"], m["xyz"], m["level"], m["gbox"], 0, 1, 0)
    kept = st == 0
    assert (st == 1).sum() >= 3 and not (st == 2).any()
    u = _union(Z, "adv")
    _owned_right(u, world)
    if world > 1:
        assert (u["rank"] != m["rank"][kept]).sum() > 10                            # particles did change ranks
    assert np.array_equal(u["id"], m["id"][kept]) and np.array_equal(u["xyz"], ex[kept])
    assert np.array_equal(u["level"], el[kept]) and np.array_equal(u["gbox"], eb[kept]) and np.array_equal(u["r"], m["r"][kept])
    for k in ("id", "xyz", "r", "cpu", "level", "gbox"):
        assert np.array_equal(u[k], ref[k]), k
    for z in Z:
        assert z["adv_meta"][0] == (st == 1).sum() and z["adv_meta"][2] == kept.sum() and np.array_equal(z["adv_meta"], container[1][0]["adv_meta"])


@pytest.mark.parametrize("world", [1, 2, 3])
def test_grown_boxes(container, world):
    """check 3: level-1 particles up to 1.5 fine cells outside the patch stay on level 1 under redistribute(1, 1, 2): level, global box
    (the lowest index whose grown region holds the particle, whoever owns it) and position are the yardstick's"""
    Z = container[world]
    p = _union(Z, "pushed")
    ex, el, eb, st = _yardstick(p["id"], p["xyz"], p["level"], p["gbox"], 1, 1, 2)
    assert not st.any()
    u = _union(Z, "grown")
    _owned_right(u, world)
    outside = np.any((p["xyz"] < np.array(PATCH_LO)) | (p["xyz"] >= np.array(PATCH_HI)), axis=1) & (p["level"] == 1)
    assert outside.sum() > 50 and np.all(u["level"][outside] == 1)
    assert np.array_equal(u["id"], p["id"]) and np.array_equal(u["xyz"], ex) and np.array_equal(u["level"], el) and np.array_equal(u["gbox"], eb)
    ref = _union(container[1], "grown")
    for k in ("id", "xyz", "r", "level", "gbox"):
        assert np.array_equal(u[k], ref[k]), k


@pytest.mark.parametrize("world", [1, 2, 3])
def test_counts(container, world):
    """check 4: particle_count and total_particle_count on both levels, on every rank's boxes, equal the yardstick's arrays exactly --
    also where a fine box and the coarse box under it have different owners"""
    Z = container[world]
    u = _union(Z, "grown")
    own = owners(world)
    L = levels()
    seen = 0
    for name, fn in (("pcount", pn.particle_count), ("tcount", pn.total_particle_count)):
        for l in (0, 1):
            ref = fn(u["xyz"], u["level"], u["gbox"], L, PLO, l)
            for g, (lo, hi) in enumerate(L[l]["boxes"]):
                got = Z[own[l][g]][f"{name}_l{l}_b{g}"]
                assert np.array_equal(got, ref[tuple(slice(lo[e], hi[e] + 1) for e in range(3))]), (name, l, g)
                seen += 1
            if name == "tcount" and l == 0:
                assert ref.sum() < len(u["id"]) and ref.sum() > pn.particle_count(u["xyz"], u["level"], u["gbox"], L, PLO, 0).sum() + 50
    assert seen == 20
    if world > 1:                                               # a fine box over coarse boxes of another owner
        assert any(own[1][g] != own[0][q] for g in range(2) for q in range(8))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_collective_error(container, world):
    """check 5: one particle on one rank cannot be placed: every rank gets the error, every rank's read() is unchanged, and the next valid
    collective call works"""
    Z = container[world]
    bad = [int(z["err_id"][0]) for z in Z if "err_id" in z.files]
    assert len(bad) == 1
    for z in Z:
        assert "1 particles are in no box of levels 1 .. 1" in str(z["err_msg"][0]) and bool(z["err_unchanged"][0])
        assert np.array_equal(z["after_err_meta"], Z[0]["after_err_meta"]) and z["after_err_meta"][0] == 0
    u = _union(Z, "after_err")
    _owned_right(u, world)
    assert len(u["id"]) == Z[0]["grown_meta"][2] == Z[0]["after_err_meta"][2]
    q = int(np.nonzero(u["id"] == bad[0])[0][0])
    assert u["level"][q] == 0 and u["gbox"][q] == 0 and np.array_equal(u["xyz"][q], (0.05, 0.05, 0.05))


# ---- part B: the checks ----------------------------------------------------------------------------------------------------------------------
def _particles(path):
    """everything in <path>/Particles/, sorted by id (a directory of several writers holds one sorted part per writer)"""
    from iamr_amd.particles import read_particles_dir
    d = read_particles_dir(path)
    o = np.argsort(d["id"], kind="stable")
    return {k: (v[o] if k != "next_id" else v) for k, v in d.items()}


def _close(a, b, tol=TOL_RUN, period=1.0):
    """same ids and count; positions within tol modulo the period; returns the largest difference"""
    assert np.array_equal(a["id"], b["id"]) and a["next_id"] == b["next_id"] and len(a["id"]) > 0
    dlt = np.abs(a["xyz"] - b["xyz"])
    dlt = np.minimum(dlt, np.abs(period - dlt))
    print(f"largest position difference {dlt.max():.3e} (bound {tol:.0e})")
    assert dlt.max() <= tol, dlt.max()
    return dlt.max()


def _log(d, group, job, rank=0):
    return open(os.path.join(d, f"{group}_job{job}_r{rank}.txt")).read()


def test_runs_against_one_rank(all_worlds):
    """taylorgreen_amr16 (three levels, sub-cycling), 512 particles, two coarse steps on 1, 2 and 3 ranks: the checkpoints' Particles/
    hold the same ids; positions within 1e-8 of the one-rank run; format 2 with one writer per rank"""
    d = all_worlds
    x0 = np.loadtxt(f"{d}/p512.txt", skiprows=1)
    for step in (1, 2):
        A = _particles(f"{d}/chkA_0000{step}")
        assert np.array_equal(A["id"], np.arange(1, 513)) and A["next_id"] == 513
        assert np.abs(A["xyz"] - x0).max() > 1e-3                                     # they moved
        for tag, world in (("C", 2), ("B", 3)):
            _close(_particles(f"{d}/chk{tag}_0000{step}"), A)
            head = open(f"{d}/chk{tag}_0000{step}/Particles/Header").read().split("\n")
            assert head[0] == "iamr_amd-particles-2" and head[1] == "512" and int(head[3]) == world and sum(int(v) for v in head[4].split()) == 512
    assert open(f"{d}/chkA_00002/Particles/Header").read().startswith("iamr_amd-particles-1\n512\n513\n")
    _close(_particles(f"{d}/pltC_00002"), _particles(f"{d}/chkC_00002"), 0.0)         # particles_in_plotfile: the same particles


def test_total_count_and_report(all_worlds):
    """total_particle_count on level 0 of the plotfile sums to 512 exactly on every world; the PARTICLES: line says 512, on rank 0 only"""
    from iamr_amd.plotfile import PlotFile
    d = all_worlds
    for tag, group, world in (("A", "one", 1), ("C", "two", 2), ("B", "three", 3)):
        pf = PlotFile.read(f"{d}/plt{tag}_00002")
        t, c = pf.names.index("total_particle_count"), pf.names.index("particle_count")
        assert sum(float(a[..., t].sum()) for a in pf.levels[0].data) == 512.0
        assert sum(float(a[..., c].sum()) for lv in pf.levels for a in lv.data) == 512.0
        assert len(pf.levels) == 3 and sum(float(a[..., c].sum()) for a in pf.levels[1].data) > 0
        assert "PARTICLES: 512 (removed outside the domain: 0)" in _log(d, group, 0)
        for r in range(1, world):
            assert "PARTICLES:" not in _log(d, group, 0, r)


def test_restart(all_worlds):
    """restart from the two-rank checkpoint of step 1: on 2 ranks step 2 equals the uninterrupted two-rank run to the bit (positions, r,
    ids, next_id); on 1 and on 3 ranks within 1e-8; the ASCII file of particles.particle_output_file holds the checkpoint's particles"""
    from iamr_amd.particles import read_ascii
    d = all_worlds
    C, D = _particles(f"{d}/chkC_00002"), _particles(f"{d}/chkD_00002")
    for k in ("id", "xyz", "r", "cpu"):
        assert np.array_equal(C[k], D[k]), k
    assert C["next_id"] == D["next_id"] == 513
    for tag in ("E", "F"):
        assert "RESTART from" in _log(d, {"E": "one", "F": "three"}[tag], 1)
        _close(_particles(f"{d}/chk{tag}_00002"), C)
    xyz, ids, cpus = read_ascii(f"{d}/ascii_D.txt")
    C1 = _particles(f"{d}/chkC_00001")
    assert np.array_equal(ids, C1["id"]) and np.array_equal(xyz, C1["xyz"]) and np.array_equal(cpus, C1["cpu"])


def test_regrid_and_single_level(all_worlds):
    """a regridding run (the knapsack hands boxes to other ranks; the particles follow them) and a single-level run in eight boxes, 64
    particles, two steps, 2 ranks against 1: no particle lost, same ids, positions within 1e-8"""
    d = all_worlds
    x0 = np.loadtxt(f"{d}/p64.txt", skiprows=1)
    for kind in ("rg", "sl"):
        one, two = _particles(f"{d}/{kind}1_00002"), _particles(f"{d}/{kind}2_00002")
        assert np.array_equal(one["id"], np.arange(1, 65)) and np.abs(one["xyz"] - x0).max() > 1e-3
        _close(two, one)
    assert "PARTICLES: 64 (" in _log(d, "two", 2)


def test_merged_boxes(all_worlds):
    """check 6: the two-rank hierarchy run again in the library's default box mode (the level objects merge the boxes a rank owns, so the
    particles' boxes are not the callers'): ids and positions modulo the period against the one-rank run"""
    d = all_worlds
    run_group(2, [_amr(d, "M", f"{d}/p512.txt")], d, "merged", with_container=False, merge=True)
    for step in (1, 2):
        _close(_particles(f"{d}/chkM_0000{step}"), _particles(f"{d}/chkA_0000{step}"))
