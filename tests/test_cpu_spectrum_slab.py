"""CPU suite: the host-only planner of the slab-decomposed transform (include/iamrx.h: iamrx_host_spectrum_slab_plan; no device).  Every
rank derives both sides of the scatter from the boxes and their owners alone, so the plans of all ranks are taken here in one process
and executed in numpy: what p sends to q is what q expects from p, the pieces tile every slab exactly once, and a field scattered by
the rows alone is the field cut into slabs.  Eligibility and its reasons; the mirror map of a packed pair."""
import numpy as np
import pytest

KIND, PEER, BOX, LO, HI, OFF = 0, 1, 2, slice(3, 6), slice(6, 9), 9


def boxes_of(n, mg):
    out = []
    for k0 in range(0, n[2], mg[2]):
        for j0 in range(0, n[1], mg[1]):
            for i0 in range(0, n[0], mg[0]):
                out.append(((i0, j0, k0), (min(i0 + mg[0], n[0]) - 1, min(j0 + mg[1], n[1]) - 1, min(k0 + mg[2], n[2]) - 1)))
    return out


def round_robin(nb, world):
    per = (nb + world - 1) // world
    return [min(i // per, world - 1) for i in range(nb)]


def unequal_boxes():
    """(16, 8, 32) cut at x = 5, y = 3 and z = 3, 12, 13, 27: boxes of different sizes, none aligned with a slab of 2, 4 or 8 ranks"""
    xs, ys, zs = [0, 5, 16], [0, 3, 8], [0, 3, 12, 13, 27, 32]
    return [((xs[a], ys[b], zs[c]), (xs[a + 1] - 1, ys[b + 1] - 1, zs[c + 1] - 1)) for c in range(5) for b in range(2) for a in range(2)]


def cases():
    from test_cpu_dist import bench_layout
    n16 = (16, 16, 16)
    b8 = boxes_of(n16, (8, 8, 8))
    out = [("16^3 eight boxes, 2 ranks", n16, b8, round_robin(8, 2), 2), ("16^3 eight boxes, 4 ranks", n16, b8, round_robin(8, 4), 4)]
    n, boxes, owners = bench_layout(8)
    out.append(("bench layout, 8 ranks", n, boxes, owners, 8))
    ub = unequal_boxes()
    for world in (2, 4, 8):
        out.append((f"unequal boxes, {world} ranks", (16, 8, 32), ub, [(3 * i + 1) % world for i in range(len(ub))], world))
    b4 = boxes_of((4, 4, 4), (2, 2, 2))
    out.append(("4^3, 4 ranks", (4, 4, 4), b4, [(i + 1) % 4 for i in range(8)], 4))
    return out


CASES = cases()


def plans(n, boxes, owners, world):
    from iamr_amd import lib
    g = lib.Geom.make(n)
    res = [lib.host_spectrum_slab_plan(g, boxes, owners, r, world) for r in range(world)]
    for ok, why, _ in res:
        assert ok and why == ""
    return [rows for _, _, rows in res]


def npts(row):
    return int(np.prod(row[HI] - row[LO] + 1))


@pytest.mark.parametrize("name,n,boxes,owners,world", CASES, ids=[c[0] for c in CASES])
def test_send_rows_are_the_peers_receive_rows(name, n, boxes, owners, world):
    P = plans(n, boxes, owners, world)
    some = 0
    for p in range(world):
        for q in range(world):
            if p == q:
                continue
            send = P[p][(P[p][:, KIND] == 1) & (P[p][:, PEER] == q)]
            recv = P[q][(P[q][:, KIND] == 2) & (P[q][:, PEER] == p)]
            assert np.array_equal(send[:, BOX:], recv[:, BOX:]), (p, q)             # box, piece, offset: the same, in the same order
            off = 0
            for row in send:                                                        # the pieces follow one another without a gap
                assert row[OFF] == off and owners[row[BOX]] == p
                off += npts(row)
            some += len(send)
    nzl = n[2] // world
    aligned = all(lo[2] // nzl == owners[b] == hi[2] // nzl for b, (lo, hi) in enumerate(boxes))
    assert (some == 0) == aligned                                                   # (the eight boxes on 2 ranks: nothing travels)
    for r in range(world):
        kept = P[r][P[r][:, KIND] == 0]
        assert (kept[:, PEER] == r).all() and (kept[:, OFF] == -1).all()


@pytest.mark.parametrize("name,n,boxes,owners,world", CASES, ids=[c[0] for c in CASES])
def test_pieces_tile_every_slab_once_and_a_scatter_by_the_rows_is_the_field_in_slabs(name, n, boxes, owners, world):
    P = plans(n, boxes, owners, world)
    nzl = n[2] // world
    f = np.random.default_rng(5).standard_normal(n)
    # what every rank puts into its send buffers, from the rows alone: buffer (from, to)[off + p], x fastest inside a piece
    buf = {}
    for p in range(world):
        for row in P[p][P[p][:, KIND] == 1]:
            lo, hi = row[LO], row[HI]
            piece = f[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
            b = buf.setdefault((p, int(row[PEER])), {})
            b[int(row[OFF])] = piece.ravel(order="F")
    for r in range(world):
        slab = np.full((n[0], n[1], nzl), np.nan)
        hits = np.zeros((n[0], n[1], nzl), dtype=np.int64)
        for row in P[r][P[r][:, KIND] != 1]:
            lo, hi = row[LO], row[HI]
            assert r * nzl <= lo[2] and hi[2] < (r + 1) * nzl, "a piece outside the rank's slab"
            assert (lo >= 0).all() and (hi < np.array(n)).all()
            sl = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1), slice(lo[2] - r * nzl, hi[2] - r * nzl + 1))
            hits[sl] += 1
            if row[KIND] == 0:
                assert owners[row[BOX]] == r
                slab[sl] = f[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
            else:
                data = buf[(int(row[PEER]), r)][int(row[OFF])]
                slab[sl] = data.reshape(tuple(hi - lo + 1), order="F")
        assert hits.min() == 1 and hits.max() == 1
        assert np.array_equal(slab, f[:, :, r * nzl:(r + 1) * nzl])
    # every send row was consumed by somebody: the doubles sent are the doubles received
    sent = sum(npts(row) for p in range(world) for row in P[p][P[p][:, KIND] == 1])
    got = sum(npts(row) for p in range(world) for row in P[p][P[p][:, KIND] == 2])
    assert sent == got


def test_every_box_straddles_two_slabs_on_four_ranks():
    """the layout the first two cases share: 8^3 boxes on a 16^3 level against slabs of 4 planes"""
    name, n, boxes, owners, world = CASES[1]
    for r, rows in enumerate(plans(n, boxes, owners, world)):
        for b in range(len(boxes)):
            if owners[b] == r:
                assert (rows[:, BOX] == b).sum() >= 2


def test_eligibility():
    from iamr_amd import lib
    n16 = (16, 16, 16)
    b = boxes_of(n16, (8, 8, 8))
    ok, why, rows = lib.host_spectrum_slab_plan(lib.Geom.make(n16), b, [i % 3 for i in range(8)], 0, 3)
    assert not ok and "power of two" in why and len(rows) == 0
    flat = (16, 16, 4)
    bf = boxes_of(flat, (8, 8, 4))
    ok, why, rows = lib.host_spectrum_slab_plan(lib.Geom.make(flat), bf, [i % 8 for i in range(4)], 0, 8)
    assert not ok and "n_z = 4" in why and len(rows) == 0
    ok, why, rows = lib.host_spectrum_slab_plan(lib.Geom.make(flat), bf, [0, 1, 2, 3], 0, 4)
    assert ok and why == "" and len(rows) > 0
    ok, why, _ = lib.host_spectrum_slab_plan(lib.Geom.make((16, 4, 16)), [], [], 0, 8)
    assert not ok and "n_y = 4" in why
    with pytest.raises(lib.IamrxError):
        lib.host_spectrum_slab_plan(lib.Geom.make(n16), b, [0] * 8, 2, 2)


@pytest.mark.parametrize("R,nz", [(R, nz) for R in (1, 2, 4, 8) for nz in (4, 8, 16) if nz % R == 0])     # (8 ranks on 4 planes: not eligible)
def test_mirror_map(R, nz):
    """The mirror planes of a packed pair, restated: rank r sends its first plane to rank (R - r) % R, which stores it as plane 0 of
    its mirror image, and its other nzl - 1 planes, as they lie, to rank R - 1 - r, which stores them as planes 1 .. nzl - 1; the shell
    sums read the mirror of the slab's plane kl from plane (nzl - kl) % nzl of that image.  Then every rank has received exactly the
    planes {(nz - k) % nz : k in its slab}, each once, and reads each where it lies."""
    nzl = nz // R
    M = {r: {} for r in range(R)}             # rank -> storage plane of the mirror image -> global plane held
    for r in range(R):
        k0 = r * nzl
        p0, p1 = (R - r) % R, R - 1 - r
        assert 0 not in M[p0]
        M[p0][0] = k0
        for t in range(1, nzl):
            assert t not in M[p1]
            M[p1][t] = k0 + t
    for r in range(R):
        want = sorted((nz - k) % nz for k in range(r * nzl, (r + 1) * nzl))
        assert sorted(M[r].values()) == want and len(M[r]) == nzl
        for kl in range(nzl):
            assert M[r][(nzl - kl) % nzl] == (nz - (r * nzl + kl)) % nz
