"""Scan mode without a GPU: the cache planner, the scan-contiguous shard, the slot entry points' argument checks."""
import ctypes as C
import itertools
import random

import pytest

from itermvs_amd import shard
from itermvs_amd.scan_cache import plan_schedule


def dtu_like_maps(n_scans=2, n_img=12, n_views=5, seed=0):
    """per scan, every image is a reference once with n_views - 1 neighbours as sources (some overlap)"""
    rng = random.Random(seed)
    maps = []
    for sc in range(n_scans):
        for r in range(n_img):
            srcs = rng.sample([v for v in range(n_img) if v != r], n_views - 1)
            maps.append([(sc, r)] + [(sc, v) for v in srcs])
    return maps


def belady_misses(maps, capacity):
    """brute force: at every miss with a full cache, try every victim set and keep the one that minimises the misses of
    the rest of the list (exhaustive search over the remaining decisions, small inputs only)"""
    from functools import lru_cache
    maps = [tuple(m) for m in maps]

    @lru_cache(maxsize=None)
    def best(i, resident):
        if i == len(maps):
            return 0
        m = maps[i]
        missing = [k for k in m if k not in resident]
        free = capacity - len(resident)
        need = len(missing) - free
        if need <= 0:
            return len(missing) + best(i + 1, frozenset(resident | set(missing)))
        cands = [k for k in resident if k not in m]
        out = None
        for victims in itertools.combinations(sorted(cands), need):
            r = frozenset((resident - set(victims)) | set(missing))
            c = len(missing) + best(i + 1, r)
            out = c if out is None else min(out, c)
        return out

    return best(0, frozenset())


def check_plan(maps, steps, capacity):
    resident = {}
    computed = 0
    for m, st in zip(maps, steps):
        for k, slot in st.compute:
            assert 0 <= slot < capacity
            for kk in [kk for kk, s in resident.items() if s == slot]:
                del resident[kk]                 # evicted: its slot is reused
            assert k not in resident
            resident[k] = slot
            computed += 1
        assert len(resident) <= capacity
        assert tuple(st.views) == tuple(m)
        # every view of the map is resident, at the slot the step names
        assert st.slots == tuple(resident[k] for k in m)
        assert len(set(st.slots)) == len(m)
    return computed


def test_planner_computes_each_image_once_with_enough_capacity():
    maps = dtu_like_maps(n_scans=2, n_img=12, n_views=5)
    images = {k for m in maps for k in m}
    for cap in (len(images), len(images) + 7):
        steps = plan_schedule(maps, cap, 5)
        assert check_plan(maps, steps, cap) == len(images)
    # first map: its five images in consecutive slots (one FeatureNet call)
    steps = plan_schedule(maps, 100, 5)
    assert [s for _, s in steps[0].compute] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("cap,seed", [(3, 0), (4, 1), (5, 2), (6, 3)])
def test_planner_eviction_matches_brute_force(cap, seed):
    maps = dtu_like_maps(n_scans=1, n_img=7, n_views=3, seed=seed)[:6]
    steps = plan_schedule(maps, cap, 3)
    assert check_plan(maps, steps, cap) == belady_misses(maps, cap)


def test_planner_evicts_the_furthest_next_use():
    a, b, c, d = "abcd"
    maps = [[a, b], [c, a], [d, a], [b, c]]
    steps = plan_schedule(maps, 3, 2)
    # before map 2 (needs d): resident a, b, c; a is needed now, b at map 3, c at map 3 -> b or c leaves, never a
    assert steps[2].compute[0][0] == d
    assert check_plan(maps, steps, 3) == 5


def test_planner_refuses_a_capacity_below_n_views():
    maps = dtu_like_maps(n_scans=1, n_img=6, n_views=5)
    with pytest.raises(ValueError, match="below n_views"):
        plan_schedule(maps, 4, 5)
    with pytest.raises(ValueError):
        plan_schedule([[1, 2, 3]], 3, 2)               # a map with more views than n_views


def test_scan_contiguous_shard_covers_every_view_once():
    items = [(s, v) for s in range(22) for v in range(49)]
    seen = []
    blocks = [shard.shard_contiguous(len(items), r, 8) for r in range(8)]
    for blk in blocks:
        assert blk == list(range(blk[0], blk[-1] + 1))                 # one contiguous block per rank
        seen += [items[i] for i in blk]
    assert sorted(seen) == items and len(seen) == len(set(seen))
    assert max(map(len, blocks)) - min(map(len, blocks)) <= 1
    assert [b[0] for b in blocks] == sorted(b[0] for b in blocks)      # rank order = list order
    assert shard.shard_contiguous(3, 5, 8) == [] and shard.shard_indices(10, 1, 4) == [1, 5, 9]
    with pytest.raises(ValueError):
        shard.shard_contiguous(10, 8, 8)


def test_slot_struct_follows_the_header():
    from itermvs_amd import _lib
    assert C.sizeof(_lib.LevelSlots) == 8 + 4 * 8 + 5 * 4 + 4 + 8            # (4 bytes of padding before `slot`)
    assert _lib.LevelSlots.slot.offset == 64


def test_slot_entry_points_validate_before_any_launch():
    from itermvs_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    addr = C.addressof(buf)
    aligned = (addr + 15) // 16 * 16
    slots = (_lib.LevelSlots * 3)()
    for i, c in enumerate((16, 32, 48)):
        s = slots[i]
        s.slab, s.slot, s.n_slots = aligned, aligned, 4
        s.C, s.H, s.W, s.dtype = c, 4, 4, _lib.F32
        s.sc, s.sx, s.sy, s.slot_stride = 1, c, 4 * c, 16 * c
    p = _lib.CorrInitParams()
    p.B, p.S, p.H, p.W, p.N = 1, 2, 4, 4, 32
    p.ref.data = addr; p.ref.C, p.ref.H, p.ref.W = 48, 4, 4
    p.proj = addr; p.inv_depth_min = addr; p.inv_depth_max = addr; p.out = addr
    init = lambda: lib.itermvs_corr_init_slots(C.byref(p), C.byref(slots[2]), None)
    assert lib.itermvs_corr_init_slots(None, C.byref(slots[2]), None) == -1
    assert lib.itermvs_corr_init_slots(C.byref(p), None, None) == -1
    p.S = 17
    assert init() == -4                                  # S out of range (ERR_VIEWS)
    p.S = 0
    assert init() == -4
    p.S = 2
    slots[2].slot = None
    assert init() == -1                                  # null slot table
    slots[2].slot = aligned
    slots[2].slot_stride = 100                           # slots would overlap (< H * sy)
    assert init() == -6
    slots[2].slot_stride = 16 * 48 + 2                   # not a multiple of 4 elements
    assert init() == -5
    slots[2].slot_stride = 16 * 48
    slots[2].sc = 16
    assert init() == -6                                  # not channels-last
    slots[2].sc = 1
    slots[2].n_slots = 0
    assert init() == -2
    slots[2].n_slots = 4
    slots[2].slab = aligned + 4
    assert init() == -5                                  # slab not 16-byte aligned
    slots[2].slab = aligned
    slots[2].dtype = _lib.F16
    assert init() == -8                                  # reference and sources of different storage types
    slots[2].dtype = _lib.F32
    q = _lib.CorrIterParams()
    q.B, q.S, q.H, q.W = 1, 2, 4, 4
    q.ref_q = aligned; q.proj = addr; q.view_w = addr; q.inv_depth_min = addr; q.inv_depth_max = addr
    q.norm_depth = addr
    for l in range(3):
        q.N[l], q.out[l] = 4, addr
    it = lambda: lib.itermvs_corr_iter_slots(C.byref(q), slots, None)
    assert lib.itermvs_corr_iter_slots(C.byref(q), None, None) == -1
    q.S = 17
    assert it() == -4
    q.S = 2
    slots[1].C = 20
    assert it() == -3                                    # channels
    slots[1].C = 32
    slots[0].slot = None
    assert it() == -1
    slots[0].slot = aligned
    slots[0].sx = 15
    assert it() == -5
    slots[0].sx = 16
    q.N[2] = 9
    assert it() == -2                                    # more hypotheses than ITERMVS_MAX_HYP (all checks before it passed)


def test_feature_cache_flag_is_refused_outside_folder_mode():
    import eval as E
    a = E.build_parser().parse_args(["--feature_cache", "8"])
    with pytest.raises(SystemExit, match="--dataset folder"):
        E.check_feature_cache(a)
    a = E.build_parser().parse_args(["--dataset", "folder", "--feature_cache", "3", "--n_views", "5"])
    with pytest.raises(SystemExit, match="below --n_views"):
        E.check_feature_cache(a)
    assert E.check_feature_cache(E.build_parser().parse_args([])) == 0
