"""Host-side I/O of a multi-rank run, driven by hand in one process: the two-phase plotfile writer (every rank its Cell_D_<rank>, rank 0
the headers), the same for the checkpoint's VisMF files incl. the subset read, and the owner deal of a restart on another world size."""
import filecmp
import os
import numpy as np
import pytest
from iamr_amd.plotfile import PlotFile, Level, gather_meta

NAMES = ["x_velocity", "y_velocity", "z_velocity", "density", "tracer", "mag_vort"]
BOXES = [[((0, 0, 0), (7, 7, 3)), ((8, 0, 0), (15, 7, 3)), ((0, 0, 4), (7, 7, 7)), ((8, 0, 4), (15, 7, 7))],
         [((8, 4, 4), (15, 11, 11)), ((16, 4, 4), (19, 11, 7)), ((16, 4, 8), (23, 11, 11))]]
# owner of every box per level; in the 3-rank deal rank 2 owns no box of level 1, in the 2-rank deal rank 1 owns no box of level 0
OWNERS = {1: [[0, 0, 0, 0], [0, 0, 0]], 2: [[0, 0, 0, 0], [1, 0, 1]], 3: [[2, 0, 1, 0], [1, 0, 1]]}


def hierarchy(seed=0):
    rng = np.random.default_rng(seed)
    return [[rng.standard_normal(tuple(h - q + 1 for q, h in zip(lo, hi)) + (len(NAMES),)) for lo, hi in BOXES[l]] for l in range(2)]


def plotfile(data, owners=None, rank=None):
    """the PlotFile a rank holds: every box, the data of its own boxes (rank None: everything, as a one-rank writer)"""
    levels = []
    for l in range(2):
        own = None if rank is None else [q for q, o in enumerate(owners[l]) if o == rank]
        arrs = data[l] if own is None else [data[l][q] for q in own]
        dom = ((0, 0, 0), (15 * 2 ** l + 2 ** l - 1, 7 * 2 ** l + 2 ** l - 1, 7 * 2 ** l + 2 ** l - 1))
        levels.append(Level(dom, (0.0625 / 2 ** l,) * 3, BOXES[l], arrs, 3 * 2 ** l, 0.375, owned=own))
    return PlotFile(NAMES, 0.375, (0.0, 0.0, 0.0), (1.0, 0.5, 0.5), levels)


def tree(path):
    return sorted(os.path.relpath(os.path.join(dp, f), path) for dp, _, fs in os.walk(path) for f in fs)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_two_phase_plotfile_writer(tmp_path, world):
    data = hierarchy()
    owners = OWNERS[world]
    out = str(tmp_path / "plt")
    pfs = [plotfile(data, owners, r) for r in range(world)]
    pfs[0].make_dirs(out)
    metas = {r: pfs[r].write_data(out, r) for r in range(world)}                  # phase A, every "rank"
    for r in range(world):
        for l in range(2):
            mine = [q for q, o in enumerate(owners[l]) if o == r]
            assert [m[0] for m in metas[r][l]] == mine
            assert os.path.exists(os.path.join(out, f"Level_{l}", f"Cell_D_{r:05d}")) == bool(mine)      # no box of a level: no file
    assert not os.path.exists(os.path.join(out, "Header"))
    pfs[0].write_headers(out, metas)                                               # phase B, rank 0
    back = PlotFile.read(out)
    assert back.names == NAMES and back.time == 0.375
    for l in range(2):
        assert back.levels[l].boxes == BOXES[l]
        assert [fn for fn, _ in back.levels[l].fab_files] == [f"Cell_D_{o:05d}" for o in owners[l]]
        for q in range(len(BOXES[l])):
            assert np.array_equal(back.levels[l].data[q], data[l][q]), (l, q)
        # the min / max tables are in global box order
        H = open(os.path.join(out, f"Level_{l}", "Cell_H")).read().split("\n")
        at = H.index(f"{len(BOXES[l])},{len(NAMES)}")
        for q in range(len(BOXES[l])):
            assert [float(v) for v in H[at + 1 + q].split(",")[:-1]] == [data[l][q][..., n].min() for n in range(len(NAMES))]
    # every file equals the one-rank writer's, apart from where the fabs lie
    ref = str(tmp_path / "ref")
    plotfile(data).write(ref)
    assert open(os.path.join(out, "Header")).read() == open(os.path.join(ref, "Header")).read()
    if world == 1:
        assert tree(out) == tree(ref) == ["Header", "Level_0/Cell_D_00000", "Level_0/Cell_H", "Level_1/Cell_D_00000", "Level_1/Cell_H"]
        for f in tree(ref):
            assert filecmp.cmp(os.path.join(out, f), os.path.join(ref, f), shallow=False), f


def test_two_phase_writer_refuses_unowned_and_doubly_owned_boxes(tmp_path):
    data = hierarchy()
    out = str(tmp_path / "plt")
    a, b = plotfile(data, OWNERS[2], 0), plotfile(data, OWNERS[2], 1)
    a.make_dirs(out)
    ma, mb = a.write_data(out, 0), b.write_data(out, 1)
    with pytest.raises(ValueError):
        a.write_headers(out, {0: ma})                   # the boxes of rank 1 are missing
    with pytest.raises(ValueError):
        a.write_headers(out, {0: ma, 1: mb, 2: ma})     # written twice


def test_metadata_table_carries_offsets_and_extrema_exactly():
    """gather_meta: the owner's row plus everyone else's zeros; offsets up to 2^53 survive the trip through doubles"""
    nb, nc = 5, 3
    owners = [1, 0, 2, 1, 0]
    rng = np.random.default_rng(3)
    full = [(q, int(rng.integers(0, 2 ** 53)), list(rng.standard_normal(nc)), list(rng.standard_normal(nc))) for q in range(nb)]
    tables = []

    def collect(T, op):
        tables.append(T.copy())
    for r in range(3):
        gather_meta(nb, nc, [m for m in full if owners[m[0]] == r], owners, collect)
    total = sum(tables)

    def hand_back(T, op):
        T[:] = total
    metas = gather_meta(nb, nc, [], owners, hand_back)
    assert sorted(metas) == [0, 1, 2]
    for r in metas:
        assert metas[r] == [m for m in full if owners[m[0]] == r]


@pytest.mark.parametrize("typ,ngrow,nc", [((0, 0, 0), 1, 5), ((1, 1, 1), 1, 1), ((0, 0, 0), 0, 1)])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_two_phase_vismf(tmp_path, world, typ, ngrow, nc):
    """the checkpoint's MultiFab files: cell-centred and nodal arrays with ghost cells, written by 1 / 2 / 3 ranks, read back whole and
    as a subset of grids"""
    from iamr_amd import checkpoint as ck
    boxes = [(list(lo), list(hi)) for lo, hi in BOXES[1]]
    owners = OWNERS[world][1]
    rng = np.random.default_rng(7)
    arrays = [rng.standard_normal(tuple(hi[d] - lo[d] + 1 + typ[d] + 2 * ngrow for d in range(3)) + (nc,)) for lo, hi in boxes]
    d = str(tmp_path)
    metas = {}
    for r in range(world):
        mine = [q for q, o in enumerate(owners) if o == r]
        metas[r] = ck._write_vismf_data(d, "SD_0_New_MF", boxes, typ, [arrays[q] for q in mine], ngrow, r, mine)
        assert os.path.exists(os.path.join(d, f"SD_0_New_MF_D_{r:05d}")) == bool(mine)
    ck._write_vismf_header(d, "SD_0_New_MF", boxes, typ, nc, ngrow, metas)
    assert ck._vismf_ncomp(d, "SD_0_New_MF") == nc
    back = ck._read_vismf(d, "SD_0_New_MF")
    assert len(back) == len(arrays) and all(np.array_equal(x, y) for x, y in zip(back, arrays))
    for grids in ([2], [0, 2], [1], []):
        sub = ck._read_vismf(d, "SD_0_New_MF", grids)
        assert len(sub) == len(grids) and all(np.array_equal(x, arrays[q]) for x, q in zip(sub, grids))
    if world == 1:                                      # the one-writer form is these two phases
        os.makedirs(os.path.join(d, "one"))
        ck._write_vismf(os.path.join(d, "one"), "SD_0_New_MF", boxes, typ, arrays, ngrow)
        for f in ("SD_0_New_MF_H", "SD_0_New_MF_D_00000"):
            assert filecmp.cmp(os.path.join(d, f), os.path.join(d, "one", f), shallow=False), f


def decompose_owners(nboxes, nranks):
    """the owner formula of lib.Layout.decompose: contiguous chunks of the box list"""
    per = (nboxes + nranks - 1) // nranks
    return [min(i // per, nranks - 1) for i in range(nboxes)]


@pytest.mark.parametrize("world", [1, 2, 3, 4, 7])
def test_owner_deal_of_a_restart_on_another_world_size(world):
    from iamr_amd.checkpoint import deal_owners
    rng = np.random.default_rng(11)
    l0 = [((8 * i, 8 * j, 8 * k), (8 * i + 7, 8 * j + 7, 8 * k + 7)) for k in range(2) for j in range(2) for i in range(3)]
    fine = []
    for q in range(9):
        lo = [int(v) for v in rng.integers(0, 32, 3)]
        ext = [int(v) for v in rng.choice([4, 8, 16], 3)]
        fine.append((tuple(lo), tuple(lo[d] + ext[d] - 1 for d in range(3))))
    own = deal_owners([l0, fine, fine[:2]], world)
    assert own == deal_owners([list(l0), list(fine), fine[:2]], world)                 # deterministic
    assert [len(o) for o in own] == [12, 9, 2]
    assert all(isinstance(o, int) and 0 <= o < world for lv in own for o in lv)        # one owner per box, a rank of this world
    assert own[0] == decompose_owners(len(l0), world)
    # refined levels: largest box first onto the least-loaded rank -- no rank carries more than the lightest rank plus one largest box
    cells = [int(np.prod([hi[d] - lo[d] + 1 for d in range(3)])) for lo, hi in fine]
    load = [sum(c for c, o in zip(cells, own[1]) if o == r) for r in range(world)]
    assert max(load) - min(load) <= max(cells)
    if world >= 2:
        big = sorted(range(9), key=lambda q: (-cells[q], q))
        assert own[1][big[0]] == 0 and own[1][big[1]] == 1                             # ties by box index, ranks in order


def test_comm_allreduce_without_a_communicator():
    """one process, no transport installed: one rank, the buffer stays as it is, the barrier returns; wrong arguments are refused"""
    from iamr_amd import lib
    assert lib.comm_rank() == (0, 1)
    v = np.array([3.0, -1.5, 0.0, 2.0 ** 53 - 1])
    for op in (0, 1, 2):
        a = v.copy()
        assert lib.comm_allreduce(a, op) is a and np.array_equal(a, v)
    lib.comm_barrier()
    with pytest.raises(lib.IamrxError):
        lib.comm_allreduce(v.copy(), 3)
    with pytest.raises(TypeError):
        lib.comm_allreduce(v.astype(np.float32))
    with pytest.raises(TypeError):
        lib.comm_allreduce(np.zeros((4, 4))[:, ::2])
