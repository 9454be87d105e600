// The persistent kernels' index arithmetic, once: the grid rule (persistent_plan: pure, no HIP call, no getenv), the tile walks (the
// kernels and the host run the same inline functions; tests/test_tile_walk_cpu.py holds both to their post-conditions without a
// GPU) and the launch tail of the fused one-launch kernels.  DESIGN.md lists which kernel uses which.
//
// Tile order.  A persistent grid is at most what stays resident at once (a workgroup queued behind another would serialise its tile
// list).  Workgroups are dispatched round-robin over the 8 XCDs: workgroup b runs on XCD b % 8.  BANDED, the tiles of one XCD are a
// contiguous part of the tile list (whole image bands), so that tiles which share halo rows meet in the same 4 MB L2 instead of
// being fetched from the fabric once per XCD; otherwise workgroup b takes tiles b, b + grid, ... (plain order).
#pragma once

#include "common.hpp"

namespace itermvs {

using PersistentPlan = itermvs_persistent_plan_t;

// grid = min(tiles, resident), rounded down to a multiple of 8 from 16 on when `round8` (85 -> 80 costs nothing).  `banded`: STRIDED
// and RUNS: grid % 8 == 0; PLAIN: never; STRIDED_LEAD: grid >= 8 (stem_kernel decides it on the device, by the same rule).
// Post-conditions with the walks below: every tile is visited exactly once, a workgroup's tiles in increasing order.  STRIDED
// (and STRIDED_LEAD), banded: workgroup b stays inside eighth b % 8, [total * x / 8, total * (x + 1) / 8).  RUNS, banded: an XCD
// owns one contiguous range, the ranges in XCD order (the longer runs come first, so the cuts are not the exact eighths).
// STRIDED: every workgroup owns a tile (tiles >= grid; banded, an eighth holds >= grid / 8 tiles) -- conv_tile_kernel and
// conv_tile3_kernel have no early return.
static inline int persistent_plan(int64_t tiles, int resident, bool round8, itermvs_walk_kind kind, PersistentPlan* out) {
    ITERMVS_RETURN_IF(tiles < 1 || tiles >= ((int64_t)1 << 31) || resident < 1, ITERMVS_ERR_DIMS);
    int grid = (int)(tiles < resident ? tiles : resident);
    if (round8 && grid >= 16) grid &= ~7;
    const bool runs = kind == ITERMVS_WALK_RUNS;      // workgroup g owns run (+ 1 for the first run_extra) consecutive tiles
    *out = {grid, kind == ITERMVS_WALK_PLAIN ? 0 : kind == ITERMVS_WALK_STRIDED_LEAD ? grid >= 8 : grid % 8 == 0,
            runs ? (int)(tiles / grid) : 0, runs ? (int)(tiles % grid) : 0};
    return ITERMVS_OK;
}
// ... with per_cu workgroups per CU resident: the tile count is checked before the device is asked for its CUs
static inline int persistent_plan_cus(int64_t tiles, int per_cu, bool round8, itermvs_walk_kind kind, PersistentPlan* out) {
    const int rc = persistent_plan(tiles, 1, round8, kind, out);
    return rc != ITERMVS_OK ? rc : persistent_plan(tiles, per_cu * itermvs_num_cus(), round8, kind, out);
}

// Workgroup `block` of `nblocks` visits tiles w, w + wstep, ... < wend.  The first `lead` workgroups do other work (stem_kernel's
// composing workgroups) and nblocks - lead need not be a multiple of 8: XCD x's first tile workgroup is the first b >= lead with
// b % 8 == x.  With lead == 0 and nblocks % 8 == 0 this is w = total * x / 8 + block / 8, wstep = nblocks / 8 -- the form
// conv_tile_kernel and conv_tile3_kernel carry written out (see there).
struct TileWalk { int w, wstep, wend; };
__host__ __device__ __forceinline__ TileWalk tile_walk_strided(int total, int block, int nblocks, int lead, bool banded) {
    TileWalk t = {block - lead, nblocks - lead, total};
    if (banded) {
        const int xcd = block & 7;
        const int first = lead + ((xcd - lead) & 7);
        t.w = (int)((int64_t)total * xcd / 8) + ((block - first) >> 3);
        t.wend = (int)((int64_t)total * (xcd + 1) / 8);
        t.wstep = (nblocks - 1 - first) / 8 + 1;
    }
    return t;
}

// Workgroup `block` owns the tiles t0 .. t0 + count - 1 (banded: nblocks % 8 == 0, the runs of one XCD are neighbours); the host
// splits the tile list, so the kernels' prologue has no 64-bit division
struct TileRun { int t0, count; };
__host__ __device__ __forceinline__ TileRun tile_walk_run(int run, int run_extra, int block, int nblocks, bool banded) {
    const int g = banded ? (block & 7) * (nblocks >> 3) + (block >> 3) : block;
    return {g * run + (g < run_extra ? g : run_extra), run + (g < run_extra ? 1 : 0)};
}

// The tail of a fused one-launch kernel: the dynamic-LDS attribute once per instantiation, the launch -- inside the kind-3 profile
// bracket where `bracket` (bench.py's convolution roofline counts these launches like itermvs_conv2d ones) -- and its status
template <auto Kern, int LDS, class... Args>
static inline int launch_fused(dim3 grid, int block, hipStream_t stream, bool bracket, const Args&... args) {
    static const bool attr_ok =
        LDS == 0 || hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS) == hipSuccess;
    ITERMVS_RETURN_IF(!attr_ok, ITERMVS_ERR_LAUNCH);
    if (bracket) itermvs_profile_begin(3, stream);
    hipLaunchKernelGGL(Kern, grid, dim3(block), LDS, stream, args...);
    if (bracket) itermvs_profile_end(3, stream);
    return itermvs_launch_status();
}

}  // namespace itermvs
