"""The persistent kernels' grid rule and tile walks (csrc/tile_walk.hpp), checked on the host: itermvs_persistent_plan against an
independent restatement of the rule each kernel's launch code carried before they were gathered, and itermvs_tile_walk_owner --
the kernels' own inline walk functions, run for every workgroup of a plan -- against the post-conditions the kernels rely on."""
import ctypes as C

import numpy as np
import pytest

DIMS = -2
STRIDED, RUNS, PLAIN, LEAD = 0, 1, 2, 3


# ---- the eight launch rules as they stood before tile_walk.hpp (file:line of the commit before it), `resident` = the cap each
# ---- caller still computes itself.  Each returns (grid, banded, run, run_extra).
def rule_conv_tile(tiles, resident):         # conv_tile.hpp:44-49 (conv_tile and conv_tile3, per channel block)
    gx = resident
    if gx > tiles:
        gx = tiles
    if gx < 1:
        gx = 1
    if gx >= 16:
        gx &= ~7
    return gx, int(gx % 8 == 0 and tiles >= gx), 0, 0


def rule_res_chain(tiles, cus):              # res_chain.hip:379-381
    grid = tiles if tiles < cus else cus
    return grid, int(grid % 8 == 0 and tiles >= grid), 0, 0


rule_lat_conv = rule_res_chain               # lat_conv.hip:443-445, the same three lines


def rule_gru(tiles, cus):                    # gru.hip:335-339
    grid = tiles if tiles < cus else cus
    if grid >= 16:
        grid &= ~7
    return grid, int(grid % 8 == 0), tiles // grid, tiles % grid


rule_down_conv = rule_gru                    # down_conv.hip:289-293, the same five lines


def rule_stack2(tiles, resident):            # stack2.hip:335-336 (resident = 2 * CUs); the kernel strides by gridDim.x
    return (tiles if tiles < resident else resident), 0, 0, 0


rule_head = rule_stack2                      # head.hip:706-709 (resident = wgs_per_cu * CUs)


def rule_stem(tiles, resident):              # stem.hip:264-265 (+ n_comp workgroups in front); stem.hip:106: banded when tstep >= 8
    grid = tiles if tiles < resident else resident
    return grid, int(grid >= 8), 0, 0


RULES = [("conv_tile", rule_conv_tile, STRIDED, 1), ("res_chain16", rule_res_chain, STRIDED, 0), ("lat_conv", rule_lat_conv, STRIDED, 0),
         ("gru_conv", rule_gru, RUNS, 1), ("down_conv", rule_down_conv, RUNS, 1), ("stack2", rule_stack2, PLAIN, 0),
         ("head_coop", rule_head, PLAIN, 0), ("stem", rule_stem, LEAD, 0)]


@pytest.fixture(scope="module")
def lib():
    from itermvs_amd import _lib
    return _lib.load()


def plan_of(lib, tiles, resident, round8, kind):
    from itermvs_amd import _lib
    p = _lib.PersistentPlan()
    rc = lib.itermvs_persistent_plan(tiles, resident, round8, kind, C.byref(p))
    return rc, p


@pytest.mark.parametrize("name,rule,kind,round8", RULES, ids=[r[0] for r in RULES])
def test_plan_equals_the_rule_each_kernel_had(lib, name, rule, kind, round8):
    for tiles in (1, 7, 8, 9, 15, 16, 17, 23, 24, 250, 255, 256, 257, 263, 1600, 2 ** 31 - 1):
        for resident in (1, 2, 8, 15, 16, 21, 80, 256, 304, 512):
            rc, p = plan_of(lib, tiles, resident, round8, kind)
            assert rc == 0, (tiles, resident)
            assert (p.grid, p.banded, p.run, p.run_extra) == rule(tiles, resident), (tiles, resident)
    for tiles in (0, 2 ** 31):
        assert plan_of(lib, tiles, 256, round8, kind)[0] == DIMS


def test_plan_and_owner_reject_bad_arguments(lib):
    from itermvs_amd import _lib
    assert lib.itermvs_persistent_plan(8, 8, 0, STRIDED, None) == -1
    assert plan_of(lib, 8, 8, 0, 4)[0] == DIMS and plan_of(lib, 8, 8, 0, -1)[0] == DIMS and plan_of(lib, 8, 0, 0, STRIDED)[0] == DIMS
    rc, p = plan_of(lib, 8, 8, 0, STRIDED)
    buf = (C.c_int32 * 8)()
    assert lib.itermvs_tile_walk_owner(None, 8, STRIDED, 0, buf, buf) == -1 and lib.itermvs_tile_walk_owner(C.byref(p), 8, STRIDED, 0, None, buf) == -1
    assert lib.itermvs_tile_walk_owner(C.byref(p), 0, STRIDED, 0, buf, buf) == DIMS
    assert lib.itermvs_tile_walk_owner(C.byref(p), 8, STRIDED, 1, buf, buf) == DIMS        # a lead exists for the stem's walk only
    assert lib.itermvs_tile_walk_owner(C.byref(p), 8, LEAD, -1, buf, buf) == DIMS


RESIDENTS = list(range(1, 41)) + [248, 255, 256, 257]
WALKS = [("conv_tile", STRIDED, 1, 0), ("res_chain16", STRIDED, 0, 0), ("gru_conv", RUNS, 1, 0), ("stack2", PLAIN, 0, 0),
         ("stem lead 0", LEAD, 0, 0), ("stem lead 1", LEAD, 0, 1), ("stem lead 3", LEAD, 0, 3), ("stem lead 9", LEAD, 0, 9)]


@pytest.mark.parametrize("name,kind,round8,lead", WALKS, ids=[w[0] for w in WALKS])
def test_walk_visits_every_tile_once_in_order_inside_its_eighth(lib, name, kind, round8, lead):
    """tiles 1..600 x 44 resident caps: one call per plan; the checks run on all 44 walks of a tile count at once"""
    from itermvs_amd import _lib
    R = len(RESIDENTS)
    plans = (_lib.PersistentPlan * R)()
    for tiles in range(1, 601):
        owner = np.full((R, tiles), -2, np.int32)
        order = np.full((R, tiles), -2, np.int32)
        for r, resident in enumerate(RESIDENTS):
            assert lib.itermvs_persistent_plan(tiles, resident, round8, kind, C.byref(plans[r])) == 0
            dup = lib.itermvs_tile_walk_owner(C.byref(plans[r]), tiles, kind, lead, owner.ctypes.data + r * tiles * 4, order.ctypes.data + r * tiles * 4)
            assert dup == 0, (tiles, resident, dup)
        grid = np.array([p.grid for p in plans], np.int32)
        banded = np.array([p.banded for p in plans], bool)
        assert owner.min() >= 0 and (owner < grid[:, None]).all(), tiles                            # every tile has an owner
        # a workgroup's tiles, taken in increasing tile order, carry the positions 0, 1, 2, ...
        idx = np.argsort(owner, axis=1, kind="stable")
        so, oo = np.take_along_axis(owner, idx, 1), np.take_along_axis(order, idx, 1)
        pos = np.arange(tiles)[None, :]
        first = np.ones((R, tiles), bool)
        first[:, 1:] = so[:, 1:] != so[:, :-1]
        start = np.maximum.accumulate(np.where(first, pos, 0), axis=1)
        assert (oo == pos - start).all(), tiles
        # banded: workgroup b stays inside eighth b % 8 = [tiles * x / 8, tiles * (x + 1) / 8)
        t = np.arange(tiles)
        eighth = np.searchsorted(np.array([tiles * (x + 1) // 8 for x in range(8)]), t, side="right")
        xcd = (owner + lead) % 8
        if kind == RUNS:
            # the run walk puts its `run_extra` longer runs first, so an XCD's share is not cut at exactly tiles * x / 8: XCD x
            # owns ONE contiguous range of the list and the ranges follow each other in XCD order
            assert ((xcd[:, 1:] >= xcd[:, :-1]).all(axis=1) | ~banded).all(), tiles
        else:
            assert ((xcd == eighth[None, :]) | ~banded[:, None]).all(), tiles
        if kind != LEAD:
            # no workgroup without a tile: conv_tile_kernel and conv_tile3_kernel have no early return (the stem's walk may leave
            # a workgroup of a ragged grid empty: that kernel tests tile0 < tend)
            assert (first.sum(1) == grid).all(), tiles
        if kind in (STRIDED, LEAD) and lead == 0:
            # the general strided form (tile_walk_strided, which STRIDED runs at lead 0) equals the simple one the four other kernels
            # carried, and conv_tile / conv_tile3 still carry written out: w = tiles * x / 8 + b / 8, step grid / 8
            # (where the grid is a multiple of 8 or the order is plain; the stem's ragged banded grids have no simple form)
            rows = (grid % 8 == 0) | ~banded
            assert rows.all() or kind == LEAD
            g = grid[:, None]
            step = np.maximum(g // 8, 1)
            s = np.array([tiles * x // 8 for x in range(8)])[eighth][None, :]
            want_owner = np.where(banded[:, None], (t - s) % step * 8 + eighth, t % g)
            want_order = np.where(banded[:, None], (t - s) // step, t // g)
            assert np.array_equal(owner[rows], want_owner[rows]) and np.array_equal(order[rows], want_order[rows]), tiles
