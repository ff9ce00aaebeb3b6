"""CPU suite: which coarse levels of a cell-centred hierarchy run the down leg and the up leg of a V-cycle as one launch each
(abec_leg_plan through the host-only query iamrx_host_abec_leg_plan), at the shapes that separate yes from no.  A workgroup holds its tile
grown by 2 nu cells in an LDS array of 16^3 cells, so the tile is 16 - 4 nu long (at most the level's length) and nu <= 3."""
import pytest

STORED, DENSITY, UNIFORM = 0, 1, 2
NEUMANN = 102


def box(n):
    return [((0, 0, 0), tuple(v - 1 for v in n))]


def plan(lib, n, level, boxes=None, per=(1, 1, 1), **kw):
    bcs = tuple(0 if per[d] else NEUMANN for d in range(3))
    return lib.host_abec_leg_plan(lib.Geom.make(n, periodic=per), boxes or box(n), level, lobc=bcs, hibc=bcs, **kw)


@pytest.mark.parametrize("has_a", [False, True])
@pytest.mark.parametrize("coef", [STORED, UNIFORM])
@pytest.mark.parametrize("n, level", [((64, 64, 64), 1), ((32, 32, 32), 2), ((16, 16, 16), 3)])
def test_periodic_one_box_levels_take_legs(n, level, coef, has_a):
    from iamr_amd import lib
    got = plan(lib, n, level, coef=coef, has_a=has_a)
    assert got == dict(legs=True, tile_down=(8, 8, 8), tile_up=(8, 8, 8), halo_down=4, halo_up=4), got


TWO_BOXES = [((0, 0, 0), (31, 15, 31)), ((0, 16, 0), (31, 31, 31))]
REFUSED = {
    "finest level": ((32, 32, 32), 0, {}),
    "three components": ((32, 32, 32), 1, dict(ncomp=3, coef=UNIFORM)),
    "coarse/fine faces": ((32, 32, 32), 1, dict(has_cf=True)),
    "two boxes": ((32, 32, 32), 1, dict(boxes=TWO_BOXES)),
    "a direction with walls": ((32, 32, 32), 1, dict(per=(1, 0, 1))),
    "slab transition": ((32, 32, 32), 1, dict(slab_transition=True)),
    "agglomeration transition": ((32, 32, 32), 1, dict(agg_transition=True)),
    "no pre-smoothing": ((32, 32, 32), 1, dict(nu1=0)),
    "no post-smoothing": ((32, 32, 32), 1, dict(nu2=0)),
    "nu1 too large for the tile": ((32, 32, 32), 1, dict(nu1=4)),
    "nu2 too large for the tile": ((32, 32, 32), 1, dict(nu2=4)),
    "density form": ((32, 32, 32), 1, dict(coef=DENSITY, ngrow=(1, 0, 1, 0))),
    "odd length": ((32, 18, 9), 2, {}),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_levels_that_keep_their_launches(name):
    from iamr_amd import lib
    n, level, kw = REFUSED[name]
    got = plan(lib, n, level, **kw)
    assert not got["legs"], got
    # the same level without the obstacle takes legs: the refusal is the obstacle's
    if name not in ("finest level", "odd length"):
        assert plan(lib, n, level)["legs"]


def test_size_bound_and_switch():
    from iamr_amd import lib
    old = lib.tuning_get("MG_LEGS_MAX_CELLS", -1.0)
    lib.tuning_set("MG_LEGS_MAX_CELLS", 32 ** 3)
    try:
        assert plan(lib, (32, 32, 32), 1)["legs"]
        assert not plan(lib, (64, 32, 32), 1)["legs"]          # a level above the bound
        lib.tuning_set("MG_LEGS", 0)
        try:
            assert not plan(lib, (32, 32, 32), 1)["legs"]
        finally:
            lib.tuning_set("MG_LEGS", 1)
        assert plan(lib, (32, 32, 32), 1)["legs"]              # nothing is cached beyond the call
    finally:
        if old < 0:
            lib.tuning_set("MG_LEGS_MAX_CELLS", DEFAULT_MAX_CELLS)
        else:
            lib.tuning_set("MG_LEGS_MAX_CELLS", old)


DEFAULT_MAX_CELLS = 64 ** 3


def test_default_size_bound():
    from iamr_amd import lib
    assert lib.tuning_get("MG_LEGS_MAX_CELLS", DEFAULT_MAX_CELLS) == DEFAULT_MAX_CELLS
    assert plan(lib, (64, 64, 64), 1)["legs"]
    assert not plan(lib, (128, 64, 64), 1)["legs"]


@pytest.mark.parametrize("nu1, nu2", [(2, 2), (1, 1), (2, 1), (1, 3), (3, 3)])
def test_halo_is_two_cells_per_sweep_and_the_tile_what_is_left_of_sixteen(nu1, nu2):
    from iamr_amd import lib
    got = plan(lib, (32, 32, 32), 1, nu1=nu1, nu2=nu2)
    assert got["legs"] and got["halo_down"] == 2 * nu1 and got["halo_up"] == 2 * nu2
    assert got["tile_down"] == (16 - 4 * nu1,) * 3 and got["tile_up"] == (16 - 4 * nu2,) * 3


def test_tile_is_no_longer_than_the_level():
    from iamr_amd import lib
    got = plan(lib, (24, 12, 4), 2, nu1=1, nu2=2)
    assert got["legs"] and got["tile_down"] == (12, 12, 4) and got["tile_up"] == (8, 8, 4)
