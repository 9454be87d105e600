// The one-thread-per-item ("flat") kernels' grid, once: the item count, the rule that turns it into a grid or ITERMVS_ERR_DIMS, and
// the launch.  Host only, no HIP call before a check (tests/test_flat_entry_status_cpu.py holds every limit without a GPU); the limits
// are therefore constants, not device queries.  DESIGN.md lists each flat kernel, its index width and the limit its entry point passes.
//   kFlatMaxWork   gridDim.x * blockDim.x < 2^32: hip/hip_runtime_api.h, the note at hipModuleLaunchKernel ("HIP does not support
//                  kernel launch with total work items defined in dimension with size gridDim x blockDim >= 2^32"); the runtime
//                  refuses the launch past it.  At 256 threads: 2^24 - 1 blocks, 2^32 - 256 items.
//   kFlatMaxGridX  hipDeviceProp_t::maxGridSize is an int[3] (hip_runtime_api.h): no device reports more than 2^31 - 1 blocks
//   kFlatMaxGridY  65535, what the entry points with a batch or view count in grid.y held before this header (image_pyramid_jitter,
//                  gt_pyramid, ref_quarter); gfx9 devices report 65535 or 65536 in maxGridSize[1]
//   kFlatInt32     what an entry point passes when its kernel forms the item index, or a product of its dimensions, in an int
#pragma once

#include <initializer_list>

#include "common.hpp"

namespace itermvs {

constexpr int64_t kFlatMaxWork = ((int64_t)1 << 32) - 1, kFlatMaxGridX = 0x7fffffff, kFlatMaxGridY = 65535, kFlatInt32 = 0x7fffffff;

// product of dimensions, each an int32 of the ABI: 0 if one is < 1, INT64_MAX if the product leaves 64 bits (both rejected below)
static inline int64_t flat_items(std::initializer_list<int64_t> dims) {
    int64_t n = 1;
    for (const int64_t d : dims)
        if (d < 1 || __builtin_mul_overflow(n, d, &n)) return d < 1 ? 0 : INT64_MAX;
    return n;
}

// what a launch covers: `total` items, one thread each, at most `limit` of them; `y` goes into grid.y as it is (a batch or view count)
struct FlatItems { int64_t total, limit = kFlatMaxWork, y = 1; };

// THE rule: grid = (ceil(total / threads), y), or ITERMVS_ERR_DIMS
static inline int flat_grid(const FlatItems& n, int threads, dim3* grid) {
    ITERMVS_RETURN_IF(n.total < 1 || n.total > n.limit || threads < 1 || n.y < 1 || n.y > kFlatMaxGridY, ITERMVS_ERR_DIMS);
    const int64_t blocks = (n.total - 1) / threads + 1;           // (not total + threads - 1: total may be INT64_MAX)
    ITERMVS_RETURN_IF(blocks > kFlatMaxGridX || blocks * threads > kFlatMaxWork, ITERMVS_ERR_DIMS);
    *grid = dim3((unsigned)blocks, (unsigned)n.y);
    return ITERMVS_OK;
}

// Two pieces of work in one grid: piece a owns blocks [0, *blocks_a), piece b the blocks after them.  Each piece is counted by the
// rule, and so is their sum (in 64 bits): `both` describes the whole grid for flat_launch.
static inline int flat_pair(const FlatItems& a, const FlatItems& b, int threads, FlatItems* both, int* blocks_a) {
    dim3 ga, gb;
    ITERMVS_RETURN_IF(flat_grid(a, threads, &ga) != ITERMVS_OK || flat_grid(b, threads, &gb) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    *both = {((int64_t)ga.x + gb.x) * threads};
    *blocks_a = (int)ga.x;
    return ITERMVS_OK;
}

// check, launch, status
template <auto Kern, int Threads, class... Args>
static inline int flat_launch(const FlatItems& n, hipStream_t stream, const Args&... args) {
    dim3 grid;
    ITERMVS_RETURN_IF(flat_grid(n, Threads, &grid) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    hipLaunchKernelGGL(Kern, grid, dim3(Threads), 0, stream, args...);
    return itermvs_launch_status();
}

}  // namespace itermvs
