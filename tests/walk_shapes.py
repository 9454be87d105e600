"""Shapes that put a persistent kernel's tile walk (csrc/tile_walk.hpp) into each of its regimes, from the device's CU count C:
    walk:3    3 tiles: grid < 8, plain order
    walk:9    9 tiles: 8 <= grid < 16, not a multiple of 8 (three images of three tiles: the one case that crosses the batch decode)
    walk:C-6  plain order where the grid is not rounded; a rounded grid with run = 1, run_extra = 2 for the run walks
    walk:C    banded, exactly one tile per workgroup
    walk:C+3  banded, ragged eighths, some workgroups with two tiles
(C = per_cu * CUs for a kernel that keeps more than one workgroup per CU resident.)
conv_tile / conv_tile3 keep min(4, what the occupancy query answers) workgroups per CU, which a test cannot know: they take the
regimes at per_cu = 1 (C - 6, C, C + 3: banded grids rounded to a multiple of 8, one or two tiles per workgroup whatever the cap) and
    walk:4C+3 more tiles than any resident cap: every workgroup walks several tiles of its eighth"""
import torch

REGIMES = ("walk:3", "walk:9", "walk:C-6", "walk:C", "walk:C+3")
CONV_REGIMES = REGIMES + ("walk:4C+3",)


def walk_tiles(regime, per_cu=1):
    c = per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    return {"walk:3": 3, "walk:9": 9, "walk:C-6": c - 6, "walk:C": c, "walk:C+3": c + 3, "walk:4C+3": 4 * c + 3}[regime]


def walk_shape(regime, th, tw, per_cu=1, ragged=1):
    """(N, H, W) in the kernel's OUTPUT pixels that make exactly walk_tiles(regime) tiles of th x tw; the last tile row and the last
    tile column are `ragged` pixels short of whole (where the tile is larger than that)"""
    n = 3 if regime == "walk:9" else 1
    per = walk_tiles(regime, per_cu) // n
    assert per * n == walk_tiles(regime, per_cu)
    tx = max(d for d in range(1, 17) if per % d == 0)
    ty = per // tx
    return n, ty * th - (ragged if th > ragged else 0), tx * tw - (ragged if tw > ragged else 0)
