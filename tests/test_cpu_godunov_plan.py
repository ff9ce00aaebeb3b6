"""CPU suite: the plan of one call of the fused Godunov kernels (god_z_plan and god_tile_lists_host, iamr_amd/csrc/k_godunov.hip, through the
host-only query iamrx_host_godunov_plan): which launches of which instantiation in which order, the z-chunks, and which tile runs the
boundary-condition variant.  No device is needed.

1. The tile classes that the docstring of tests/test_gpu_godunov_bc_matrix.py lists for its shapes, as assertions: per case, layout and
   tile shape the x-tiles and y-tiles of every box and the z-chunks with their "at the wall" flag, written out below from that docstring; a
   tile is at the wall when one of its three ranges is, and the plan must hold exactly these tiles in exactly these classes.
2. The two classes partition the (box, tile, chunk) triples; dead entries only pad a class of >= 64 tiles to a multiple of 8.
3. The launch matrix that tests/test_gpu_godunov_spec.py asserts from the launch counters, here from the plan itself, with the template
   values and component tables: the rules in the comment in front of god_z_plan ("one plan per call"), restated in
   `expected_launches`.  The exact order of a dealt list is pinned against `dealt`, the dealing rule restated in Python.
4. Nothing outlives a call: a tuning key flipped between two calls changes the second plan."""
import itertools
import pytest

PLM, PPM = 0, 1
DEFAULTS = {"GODUNOV_ZTX": 14, "GODUNOV_PTX": 14, "GODUNOV_ZKC": 0, "GODUNOV_SPLIT_BC": 1, "GODUNOV_SPEC": 1}


class tuning:
    """set tuning keys for a block, restore them afterwards"""

    def __init__(self, lib, **kv):
        self.lib, self.kv = lib, kv

    def __enter__(self):
        self.old = {k: self.lib.tuning_get(k, DEFAULTS[k]) for k in self.kv}
        for k, v in self.kv.items():
            self.lib.tuning_set(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.lib.tuning_set(k, v)


def plan(lib, n, periodic, boxes, tile=14, **kw):
    with tuning(lib, GODUNOV_ZTX=tile, GODUNOV_PTX=tile):
        return lib.host_godunov_plan(lib.Geom.make(n, periodic=periodic), boxes, **kw)


def tile_ranges(p, boxes):
    """the plan's tiles as {(box, (x0, x1), (y0, y1), (k0, k1)): class} in cell indices; dead entries left out"""
    tx, ty = p["tile"]
    out = {}
    for cls, b, ix, iy, c in p["tiles"]:
        if b < 0:
            continue
        lo, hi = boxes[b]
        x0, y0 = lo[0] + ix * tx, lo[1] + iy * ty
        key = (b, (x0, min(x0 + tx - 1, hi[0])), (y0, min(y0 + ty - 1, hi[1])), (lo[2] + p["chunks"][c][0], min(lo[2] + p["chunks"][c][1], hi[2])))
        assert key not in out, key
        out[key] = cls
    return out


# ------------------------------------------------------------------ 1. the classes of the bc_matrix shapes
W, O = True, False          # at the wall / off the walls, per range of one direction
A_N, A_PER = (36, 34, 36), (0, 0, 0)
A_BOXES = {"1box": [((0, 0, 0), (35, 33, 35))], "2box": [((0, 0, 0), (19, 33, 35)), ((20, 0, 0), (35, 33, 35))]}
A_Z = {(0, 7): W, (8, 13): O, (14, 20): O, (21, 27): O, (28, 35): W}          # thin first and last chunk
A_Y = {14: {(0, 13): W, (14, 27): O, (28, 33): W}, 16: {(0, 7): W, (8, 15): O, (16, 23): O, (24, 31): W, (32, 33): W}}
A_X = {("1box", 14): [{(0, 13): W, (14, 27): O, (28, 35): W}],
       ("2box", 14): [{(0, 13): W, (14, 19): O}, {(20, 33): W, (34, 35): W}],
       ("1box", 16): [{(0, 15): W, (16, 31): O, (32, 35): W}],
       ("2box", 16): [{(0, 15): W, (16, 19): O}, {(20, 35): W}]}
B_N, B_PER = (20, 34, 24), (1, 0, 1)
B_BOXES = {"2box": [((0, 0, 0), (19, 17, 23)), ((0, 18, 0), (19, 33, 23))], "2box_y2": [((0, 0, 0), (19, 1, 23)), ((0, 2, 0), (19, 33, 23))]}
B_Z = {(0, 7): O, (8, 15): O, (16, 23): O}                                    # z periodic: no thin chunks, none at a wall
B_X = {14: {(0, 13): O, (14, 19): O}, 16: {(0, 15): O, (16, 19): O}}            # x periodic: never at a wall
B_Y = {("2box", 14): [{(0, 13): W, (14, 17): O}, {(18, 31): W, (32, 33): W}],
       ("2box", 16): [{(0, 7): W, (8, 15): O, (16, 17): O}, {(18, 25): O, (26, 33): W}],
       # the tile that starts at y = 2 owns no wall cell and is at the wall by the margin of god_tile_at_wall (ty0 <= 4) alone
       ("2box_y2", 14): [{(0, 1): W}, {(2, 15): W, (16, 29): O, (30, 33): W}],
       ("2box_y2", 16): [{(0, 1): W}, {(2, 9): W, (10, 17): O, (18, 25): O, (26, 33): W}]}


def expected_classes(xs, ys, zs):
    """{(box, x range, y range, z range): class} from the per-direction tables of every box"""
    return {(b, x, y, z): int(xw or yw or zw) for b in range(len(xs))
            for (x, xw), (y, yw), (z, zw) in itertools.product(xs[b].items(), ys[b].items(), zs.items())}


@pytest.mark.parametrize("pred", [False, True], ids=["advection", "prediction"])
@pytest.mark.parametrize("tile", [14, 16])
@pytest.mark.parametrize("layout", ["1box", "2box"])
def test_bc_matrix_case_A_classes(layout, tile, pred):
    from iamr_amd import lib
    boxes = A_BOXES[layout]
    p = plan(lib, A_N, A_PER, boxes, tile, pred=pred)
    assert p["tile"] == ((14, 14) if tile == 14 else (16, 8)) and p["kc"] == 9
    assert p["chunks"] == list(A_Z)
    got = tile_ranges(p, boxes)
    assert got == expected_classes(A_X[layout, tile], [A_Y[tile]] * len(boxes), A_Z)
    assert set(got.values()) == {0, 1}                      # both launches have tiles
    assert (0, (0, 13) if tile == 14 else (0, 15), (14, 27) if tile == 14 else (8, 15), (14, 20)) in got


@pytest.mark.parametrize("pred", [False, True], ids=["advection", "prediction"])
@pytest.mark.parametrize("tile", [14, 16])
@pytest.mark.parametrize("layout", ["2box", "2box_y2"])
def test_bc_matrix_case_B_classes(layout, tile, pred):
    from iamr_amd import lib
    boxes = B_BOXES[layout]
    p = plan(lib, B_N, B_PER, boxes, tile, pred=pred)
    assert p["kc"] == 8 and p["chunks"] == list(B_Z)
    got = tile_ranges(p, boxes)
    assert got == expected_classes([B_X[tile]] * 2, B_Y[layout, tile], B_Z)
    assert set(got.values()) == {0, 1}
    if layout == "2box_y2":                                 # the "margin only" tile
        assert all(got[1, x, (2, 15) if tile == 14 else (2, 9), z] == 1 for x in B_X[tile] for z in B_Z)


# ------------------------------------------------------------------ 2. partition, padding
BIG_N = (128, 128, 64)
PARTITION_CASES = [(A_N, A_PER, b) for b in A_BOXES.values()] + [(B_N, B_PER, b) for b in B_BOXES.values()] + [
    (BIG_N, (0, 0, 0), [((0, 0, 0), (127, 127, 63))]), (BIG_N, (0, 0, 0), [((0, 0, 0), (63, 127, 63)), ((64, 0, 0), (127, 127, 63))])]


@pytest.mark.parametrize("tile", [14, 16])
@pytest.mark.parametrize("case", range(len(PARTITION_CASES)))
def test_classes_partition_the_tiles(case, tile):
    from iamr_amd import lib
    n, per, boxes = PARTITION_CASES[case]
    p = plan(lib, n, per, boxes, tile)
    tx, ty = p["tile"]
    every = set()
    for b, (lo, hi) in enumerate(boxes):
        nx, ny = -(-(hi[0] - lo[0] + 1) // tx), -(-(hi[1] - lo[1] + 1) // ty)
        every |= {(b, ix, iy, c) for ix in range(nx) for iy in range(ny) for c, (k0, _k1) in enumerate(p["chunks"]) if lo[2] + k0 <= hi[2]}
    real = [t[1:] for t in p["tiles"] if t[1] >= 0]
    assert len(real) == len(set(real)) and set(real) == every          # every (box, tile, chunk) exactly once over both classes
    for cls in (0, 1):
        entries = [t for t in p["tiles"] if t[0] == cls]
        nreal = sum(1 for t in entries if t[1] >= 0)
        if nreal < 64:
            assert len(entries) == nreal                               # no padding: the list as it is, xcd_cnt = 0
        else:
            assert len(entries) % 8 == 0                               # eight equal shares, the short ones padded
    if n == BIG_N:
        assert all(sum(1 for t in p["tiles"] if t[0] == cls and t[1] >= 0) >= 64 for cls in (0, 1))
    # the classes are listed one after the other: off the walls first
    assert [t[0] for t in p["tiles"]] == sorted(t[0] for t in p["tiles"])


def test_big_level_chunks_and_bucket_order():
    """64 planes with walls in z: thin chunks of 8, three middle chunks of 16; inside an XCD's share the longest tiles come first"""
    from iamr_amd import lib
    p = plan(lib, BIG_N, (0, 0, 0), [((0, 0, 0), (127, 127, 63))])
    assert p["kc"] == 16 and p["chunks"] == [(0, 7), (8, 23), (24, 39), (40, 55), (56, 63)]
    wall = [t for t in p["tiles"] if t[0] == 1]
    share = len(wall) // 8
    length = lambda t: p["chunks"][t[4]][1] - p["chunks"][t[4]][0] + 1 if t[1] >= 0 else 0
    for q in range(8):
        lens = [length(t) for t in wall[q * share:(q + 1) * share]]
        assert lens == sorted(lens, reverse=True), q


def dealt(entries, planes):
    """the dealing rule of god_tile_lists_host on a class's tiles in box order (box; chunk; tile row; tile): runs of 6 to the bucket
    with the least work so far (work = planes + 6, the lowest bucket on a tie), the longest first inside a bucket (stable), every bucket
    padded to the longest with (-1, 0, 0, 0)"""
    buckets, load = [[] for _ in range(8)], [0] * 8
    for i in range(0, len(entries), 6):
        q = load.index(min(load))
        for e in entries[i:i + 6]:
            buckets[q].append(e)
            load[q] += planes(e) + 6
    mx = max(len(b) for b in buckets)
    out = []
    for b in buckets:
        b = sorted(b, key=lambda e: -planes(e))
        out += b + [(-1, 0, 0, 0)] * (mx - len(b))
    return out


@pytest.mark.parametrize("tile", [14, 16])
@pytest.mark.parametrize("case", [len(PARTITION_CASES) - 2, len(PARTITION_CASES) - 1])
def test_order_of_the_dealt_lists(case, tile):
    from iamr_amd import lib
    n, per, boxes = PARTITION_CASES[case]
    p = plan(lib, n, per, boxes, tile)
    tx, ty = p["tile"]
    planes = lambda e: min(p["chunks"][e[3]][1], boxes[e[0]][1][2] - boxes[e[0]][0][2]) - p["chunks"][e[3]][0] + 1
    got = tile_ranges(p, boxes)
    for cls in (0, 1):
        in_box_order = []
        for b, (lo, hi) in enumerate(boxes):
            nx, ny = -(-(hi[0] - lo[0] + 1) // tx), -(-(hi[1] - lo[1] + 1) // ty)
            for c, (k0, k1) in enumerate(p["chunks"]):
                for iy in range(ny):
                    for ix in range(nx):
                        x0, y0 = lo[0] + ix * tx, lo[1] + iy * ty
                        key = (b, (x0, min(x0 + tx - 1, hi[0])), (y0, min(y0 + ty - 1, hi[1])), (lo[2] + k0, min(lo[2] + k1, hi[2])))
                        if got[key] == cls:
                            in_box_order.append((b, ix, iy, c))
        assert len(in_box_order) >= 64
        assert [t[1:] for t in p["tiles"] if t[0] == cls] == dealt(in_box_order, planes)


def test_zkc_key_sets_the_chunk_length():
    from iamr_amd import lib
    with tuning(lib, GODUNOV_ZKC=8):
        p = plan(lib, (20, 18, 20), (1, 1, 1), [((0, 0, 0), (19, 17, 19))])
    assert p["kc"] == 8 and p["chunks"] == [(0, 5), (6, 12), (13, 19)] and p["tiles"] == []


# ------------------------------------------------------------------ 3. the launch matrix
COMP_LISTS = {"conv": (0, 0, 0, 0, 0), "cons": (1, 1, 1, 1, 1), "mixed": (0, 0, 0, 1, 0)}
DOMAINS = {"periodic": ((1, 1, 1), 1), "walls": ((0, 0, 0), 1), "walls_nosplit": ((0, 0, 0), 0)}


def expected_launches(pred, domain, scheme, tile, spec, forcing, divu, out, ic):
    per, split = DOMAINS[domain]
    classes = [(0, False)] if all(per) else [(0, True)] if not split else [(1, False), (2, True)]
    has_inst = bool(spec) and tile == 14 and scheme == PLM and forcing == "late" and (pred or out != "edge+flux")
    every = tuple(range(3 if pred else len(ic)))
    launches = []
    for sel, bcs in classes:
        if not has_inst:
            launches.append(dict(sel=sel, bcs=bcs, frc=-1, dvu=-1, out=-1, cns=-1, comps=every))
        elif pred:
            launches.append(dict(sel=sel, bcs=bcs, frc=1, dvu=-1, out=-1, cns=-1, comps=every))
        else:
            for cns in (0, 1):                  # convective first, components ascending, an empty form issues nothing
                comps = tuple(c for c in every if ic[c] == cns)
                if comps:
                    launches.append(dict(sel=sel, bcs=bcs, frc=1, dvu=int(divu), out=2 if out == "flux" else 0, cns=cns, comps=comps))
    return launches


@pytest.mark.parametrize("spec", [0, 1], ids=["runtime", "spec"])
@pytest.mark.parametrize("tile", [14, 16])
@pytest.mark.parametrize("scheme", [PLM, PPM], ids=["plm", "ppm"])
@pytest.mark.parametrize("domain", list(DOMAINS))
def test_advection_launch_matrix(domain, scheme, tile, spec):
    from iamr_amd import lib
    per, split = DOMAINS[domain]
    n, boxes = A_N, A_BOXES["1box"]
    with tuning(lib, GODUNOV_SPEC=spec, GODUNOV_SPLIT_BC=split):
        for forcing, divu, out, (name, ic) in itertools.product(("noforce", "late", "early"), (False, True), ("none", "flux", "edge+flux"), COMP_LISTS.items()):
            p = plan(lib, n, per, boxes, tile, scheme=scheme, has_force=forcing != "noforce", fit=forcing == "early", has_divu=divu,
                     edge_out=out == "edge+flux", flux_out=out != "none", iconserv=ic)
            want = expected_launches(False, domain, scheme, tile, spec, forcing, divu, out, ic)
            assert p["launches"] == want, (forcing, divu, out, name)
            assert len(want) <= 4
            assert bool(p["tiles"]) == (want[0]["sel"] != 0)           # lists exist exactly where a launch works through one
            # thin chunks iff the tiles are split in classes and z has walls
            assert (p["chunks"][0] == (0, 7)) == (want[0]["sel"] != 0)


@pytest.mark.parametrize("spec", [0, 1], ids=["runtime", "spec"])
@pytest.mark.parametrize("tile", [14, 16])
@pytest.mark.parametrize("scheme", [PLM, PPM], ids=["plm", "ppm"])
@pytest.mark.parametrize("domain", list(DOMAINS))
def test_prediction_launch_matrix(domain, scheme, tile, spec):
    from iamr_amd import lib
    per, split = DOMAINS[domain]
    with tuning(lib, GODUNOV_SPEC=spec, GODUNOV_SPLIT_BC=split):
        for forcing in ("noforce", "late", "early"):
            p = plan(lib, A_N, per, A_BOXES["2box"], tile, pred=True, scheme=scheme, has_force=forcing != "noforce", fit=forcing == "early")
            assert p["launches"] == expected_launches(True, domain, scheme, tile, spec, forcing, False, "none", None), forcing


def test_counts_of_the_spec_test_shape():
    """20 x 18 x 20 with walls (tests/test_gpu_godunov_spec.py): every tile is at the wall, so of the two planned classes only one has
    tiles -- the counters there move by one launch per form"""
    from iamr_amd import lib
    with tuning(lib, GODUNOV_ZKC=8):
        p = plan(lib, (20, 18, 20), (0, 0, 0), [((0, 0, 0), (19, 17, 19))], iconserv=COMP_LISTS["mixed"])
    assert [(l["sel"], l["cns"], l["comps"]) for l in p["launches"]] == [(1, 0, (0, 1, 2, 4)), (1, 1, (3,)), (2, 0, (0, 1, 2, 4)), (2, 1, (3,))]
    assert p["tiles"] and all(t[0] == 1 for t in p["tiles"])


# ------------------------------------------------------------------ 4. nothing is cached beyond the call
def test_keys_are_read_at_every_call():
    from iamr_amd import lib
    kw = dict(iconserv=COMP_LISTS["mixed"])
    first = plan(lib, A_N, A_PER, A_BOXES["1box"], **kw)
    assert [l["cns"] for l in first["launches"]] == [0, 1, 0, 1] and [l["sel"] for l in first["launches"]] == [1, 1, 2, 2]
    with tuning(lib, GODUNOV_SPEC=0):
        assert [(l["sel"], l["cns"]) for l in plan(lib, A_N, A_PER, A_BOXES["1box"], **kw)["launches"]] == [(1, -1), (2, -1)]
        with tuning(lib, GODUNOV_SPLIT_BC=0):
            p = plan(lib, A_N, A_PER, A_BOXES["1box"], **kw)
            assert [(l["sel"], l["bcs"], l["cns"]) for l in p["launches"]] == [(0, True, -1)] and p["tiles"] == []
            assert p["chunks"] == [(0, 8), (9, 17), (18, 26), (27, 35)]          # no classes: no thin chunks
    with tuning(lib, GODUNOV_SPLIT_BC=0):
        assert [(l["sel"], l["cns"]) for l in plan(lib, A_N, A_PER, A_BOXES["1box"], **kw)["launches"]] == [(0, 0), (0, 1)]
    assert plan(lib, A_N, A_PER, A_BOXES["1box"], **kw) == first
