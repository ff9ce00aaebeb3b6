"""Host only: the particle directory written by several ranks (iamr_amd/particles.py: format 2, `iamr_amd-particles-2`) and read back in
shares.  The writers are played one after another, rank 0 last, the way particles.save orders them through the communicator."""
import os
import numpy as np
import pytest

from iamr_amd import particles as P


def _set(n, seed):
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(3, 3 + n)).astype(np.int32)          # shuffled, not starting at 1
    return dict(xyz=rng.uniform(-1.0, 2.0, (n, 3)), r=rng.normal(size=(n, 3)), id=ids, cpu=rng.integers(0, 5, n).astype(np.int32))


def _write_as(parent, full, split, next_id):
    """the set cut into len(split) writers' parts, written rank 0 last"""
    edges = np.concatenate([[0], np.cumsum(split)])
    world = len(split)
    for rank in list(range(1, world)) + [0]:
        s = slice(edges[rank], edges[rank + 1])
        P.write_particles_dir(parent, full["xyz"][s], full["r"][s], full["id"][s], full["cpu"][s], next_id, rank, world,
                              counts=split if rank == 0 else None)


def _union_sorted(shares):
    cat = {k: np.concatenate([s[k] for s in shares]) for k in ("xyz", "r", "id", "cpu")}
    o = np.argsort(cat["id"], kind="stable")
    return {k: v[o] for k, v in cat.items()}


def _check_shares(parent, full, world, next_id):
    shares = [P.read_particles_dir(parent, rank, world) for rank in range(world)]
    ids = np.concatenate([s["id"] for s in shares])
    assert len(ids) == len(full["id"]) and len(set(ids.tolist())) == len(ids)          # disjoint, nothing twice
    got = _union_sorted(shares)
    o = np.argsort(full["id"], kind="stable")
    for k in ("xyz", "r", "id", "cpu"):
        assert got[k].dtype == full[k].dtype and np.array_equal(got[k], full[k][o]), (world, k)      # to the bit
    for s in shares:
        assert s["next_id"] == next_id and s["xyz"].shape == (len(s["id"]), 3) and s["r"].shape == (len(s["id"]), 3)
    return shares


def test_format2_round_trip(tmp_path):
    full = _set(37, 1)
    parent = str(tmp_path)
    _write_as(parent, full, [20, 0, 17], 91)
    d = os.path.join(parent, P.PARTICLES_DIR)
    head = open(os.path.join(d, "Header")).read().split("\n")
    assert head[:5] == ["iamr_amd-particles-2", "37", "91", "3", "20 0 17"]
    assert os.path.getsize(os.path.join(d, "xyz.f64.00001")) == 0 and os.path.getsize(os.path.join(d, "id.i32.00002")) == 17 * 4
    for world in (1, 2, 4):
        shares = _check_shares(parent, full, world, 91)
        if world == 2:                                  # writers 0 and 2 go to reader 0, the empty writer 1 to reader 1
            assert [len(s["id"]) for s in shares] == [37, 0]
        if world == 4:
            assert [len(s["id"]) for s in shares] == [20, 0, 17, 0]
    one = P.read_particles_dir(parent)                  # the old call: everything
    assert len(one["id"]) == 37 and one["next_id"] == 91


def test_world_one_writes_the_format_1_bytes(tmp_path):
    full = _set(11, 2)
    d = P.write_particles_dir(str(tmp_path), full["xyz"], full["r"], full["id"], full["cpu"], 40, 0, 1, counts=[11])
    o = np.argsort(full["id"], kind="stable")
    assert sorted(os.listdir(d)) == ["Header", "cpu.i32", "id.i32", "r.f64", "xyz.f64"]
    assert open(os.path.join(d, "Header")).read() == "iamr_amd-particles-1\n11\n40\nxyz.f64 <f8 3\nr.f64 <f8 3\nid.i32 <i4 1\ncpu.i32 <i4 1\n"
    assert open(os.path.join(d, "xyz.f64"), "rb").read() == full["xyz"][o].astype("<f8").tobytes()
    assert open(os.path.join(d, "r.f64"), "rb").read() == full["r"][o].astype("<f8").tobytes()
    assert open(os.path.join(d, "id.i32"), "rb").read() == full["id"][o].astype("<i4").tobytes()
    assert open(os.path.join(d, "cpu.i32"), "rb").read() == full["cpu"][o].astype("<i4").tobytes()


def test_format1_shares(tmp_path):
    full = _set(23, 3)
    P.write_particles_dir(str(tmp_path), full["xyz"], full["r"], full["id"], full["cpu"], 77)
    shares = _check_shares(str(tmp_path), full, 3, 77)
    assert [len(s["id"]) for s in shares] == [7, 8, 8]                  # contiguous slices of the id-sorted arrays
    assert shares[0]["id"].max() < shares[1]["id"].min() < shares[2]["id"].min()
    with pytest.raises(ValueError):
        P.read_particles_dir(str(tmp_path), 3, 3)


def test_header_must_match_the_files(tmp_path):
    full = _set(9, 4)
    parent = str(tmp_path)
    _write_as(parent, full, [4, 5], 20)
    hp = os.path.join(parent, P.PARTICLES_DIR, "Header")
    good = open(hp).read()
    open(hp, "w").write(good.replace("\n4 5\n", "\n5 4\n"))             # the sum still fits, the files do not
    with pytest.raises(ValueError, match="announces"):
        P.read_particles_dir(parent)
    open(hp, "w").write(good.replace("\n4 5\n", "\n4 4\n"))             # the counts do not add up to the total
    with pytest.raises(ValueError, match="writers"):
        P.read_particles_dir(parent)
    open(hp, "w").write(good.replace("iamr_amd-particles-2", "iamr_amd-particles-9"))
    with pytest.raises(ValueError, match="not a particle directory"):
        P.read_particles_dir(parent)
    with pytest.raises(ValueError):                                     # rank 0 must be given counts that fit what it holds
        P.write_particles_dir(parent, full["xyz"][:4], full["r"][:4], full["id"][:4], full["cpu"][:4], 20, 0, 2, counts=[3, 6])
