// Argument block and launch rule shared by the LDS-tiled 3x3 convolution kernels: conv_tile.hip (exact fp32 MFMA, weight_format 2)
// and conv_tile3.hip (bf16x3 split on the bf16 MFMA, weight_format 3).
#pragma once

#include "common.hpp"
#include "conv_plan.hpp"
#include "tile_walk.hpp"

namespace itermvs {

struct TileArgs : ConvArgsBase {
    // weight[]: packed [9][nchunk][4][CoutPad][S] (format 2) / [9][nchunk][3][CoutPad][16] bf16 (format 3)
    int Cin, Hin, Win, Cout, CoutPad, Hout, Wout;
    float* out_b;             // second result (channels >= split) or nullptr
    int64_t out_b_sn;
    int split, act_b;
    int pad, act, add_mode, out_nhwc, nchunk, nstage, tiles_x, tiles_y, ncb, total;
    uint32_t rcp_tiles_x, rcp_tiles_y;   // floor(2^32 / d) + 1
    int banded;                          // XCD-banded tile order (tile_walk.hpp)
};
static_assert(sizeof(TileArgs) == 264, "kernel argument layout");

constexpr uint32_t kTileOob = 0x7fffffffu;

static inline void fill_tile_args(TileArgs& a, const ConvArgsBase& base, const itermvs_conv_params* p, const itermvs_conv_plan& pl, int nchunk) {
    fill_conv_args(a, base, p, pl);
    a.CoutPad = (p->Cout + 15) / 16 * 16;
    a.add_mode = p->add_mode; a.out_nhwc = p->out_layout;
    a.split = p->split_cout; a.act_b = p->act_b; a.out_b = p->out_b; a.out_b_sn = p->out_b_sn;
    a.nchunk = nchunk; a.nstage = pl.nstage; a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y; a.ncb = pl.ncb; a.total = pl.total;
    a.rcp_tiles_x = (uint32_t)((1ull << 32) / (uint32_t)a.tiles_x + 1);   // (unused when the divisor is 1)
    a.rcp_tiles_y = (uint32_t)((1ull << 32) / (uint32_t)a.tiles_y + 1);
    a.banded = 0;
}

// Persistent grid of conv_tile_kernel / conv_tile3_kernel: about `persist` (ITERMVS_TILE_PERSIST, default 4; measured 630 / 645 /
// 650 / 648 depth-maps/s at 2 / 3 / 4 / 8, bounded by what fits a CU) workgroups per CU in total, each walking the tile list of
// its channel block (one tile each when there are fewer tiles than that); never more than are resident at once.  The resident cap
// comes from the occupancy query; the workgroup columns and the tile order from persistent_plan (tile_walk.hpp).
template <class Kernel>
static inline int persistent_grid(Kernel kern, int block, int lds, int ncb, int total, int persist, PersistentPlan* plan) {
    int fit = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kern, block, lds) != hipSuccess || fit < 1) fit = 1;
    const int resident = itermvs_num_cus() * (persist < fit ? persist : fit) / ncb;
    return persistent_plan(total, resident < 1 ? 1 : resident, true, ITERMVS_WALK_STRIDED, plan);
}

struct TileLaunch { TileArgs a; const itermvs_conv_plan& pl; int persist; hipStream_t stream; };

template <class Kernel>
static inline int launch_persistent(Kernel kern, TileLaunch& t) {
    PersistentPlan plan;
    const int rc = persistent_grid(kern, 256, t.pl.lds_bytes, t.a.ncb, t.a.total, t.persist, &plan);
    if (rc != ITERMVS_OK) return rc;
    t.a.banded = plan.banded;
    hipLaunchKernelGGL(kern, dim3(plan.grid, t.a.ncb), dim3(256), t.pl.lds_bytes, t.stream, t.a);
    return itermvs_launch_status();
}

// The ladder from a plan to the instantiation L<MB, STRIDE, DIL, TH, TWT, CPS>::run, shared by conv_tile and conv_tile3: channel
// blocking, tile shape, chunks per stage.  It decides nothing.  BIG3: the 8x32 tile exists at MB = 3 (at stride 2 its halo tile is
// too big for every MB); MULTI: instantiations with 2 and 3 chunks per stage exist.
#define ITERMVS_LADDER template <int, int, int, int, int, int> class L, int STRIDE, int DIL, bool BIG3, bool MULTI
template <ITERMVS_LADDER, int MB, int TH, int TWT>
static int launch_cps(TileLaunch& t) {
    if constexpr (MULTI) {
        if (t.pl.CPS == 3) return L<MB, STRIDE, DIL, TH, TWT, 3>::run(t);
        if (t.pl.CPS == 2) return L<MB, STRIDE, DIL, TH, TWT, 2>::run(t);
    }
    return L<MB, STRIDE, DIL, TH, TWT, 1>::run(t);
}
template <ITERMVS_LADDER, int MB>
static int launch_shape(TileLaunch& t) {
    if constexpr (STRIDE == 1 && (BIG3 || MB < 3)) {
        if (t.pl.TH == 8) return launch_cps<L, STRIDE, DIL, BIG3, MULTI, MB, 8, 2>(t);
    }
    if (t.pl.TWT == 2) return launch_cps<L, STRIDE, DIL, BIG3, MULTI, MB, 4, 2>(t);
    return launch_cps<L, STRIDE, DIL, BIG3, MULTI, MB, 4, 1>(t);
}
template <ITERMVS_LADDER>
static int launch_ladder(TileLaunch& t) {
    if (t.pl.MB == 3) return launch_shape<L, STRIDE, DIL, BIG3, MULTI, 3>(t);
    if (t.pl.MB == 2) return launch_shape<L, STRIDE, DIL, BIG3, MULTI, 2>(t);
    return launch_shape<L, STRIDE, DIL, BIG3, MULTI, 1>(t);
}
#undef ITERMVS_LADDER

}  // namespace itermvs
