// Host side of itermvs_conv2d shared by its four back ends: ConvArgsBase + fill_conv_base (the leading fields of every kernel argument
// block and their ONE fill) and the plan -- WHICH kernel a layer runs: back end, template arguments, LDS bytes, tile counts -- as a
// pure function of the scalar fields of itermvs_conv_params and a ConvTuning: no HIP call, no getenv, no read through a data pointer
// (tests/test_conv_plan_cpu.py holds it to recorded plans without a GPU).  The launch side of each back end decides nothing.
#pragma once

#include <limits.h>

#include "common.hpp"

namespace itermvs {

// ConvArgs, MfmaArgs and TileArgs BEGIN with these fields (152 bytes, no tail padding: the derived structs continue at offset 152)
struct ConvArgsBase {
    const float* in;
    float* out;
    float* out2;          // optional second copy of the result (contiguous [N,Cout,P])
    const float* add;     // residual, added before the activation
    const float* aux1;    // epilogue operand (h for the GRU forms)
    const float* aux2;    // epilogue operand (z for the GRU update)
    int64_t in_sn, out_sn, add_sn, aux1_sn, aux2_sn;
    const float* weight[3];
    const float* bias[3];
    int seg_end[3];
    int N;
};
static_assert(sizeof(ConvArgsBase) == 152, "the derived argument blocks continue at offset 152");

static inline int fill_conv_base(ConvArgsBase& a, const itermvs_conv_params* p) {
    a.in = p->in; a.out = p->out; a.out2 = p->out2; a.add = p->add; a.aux1 = p->aux1; a.aux2 = p->aux2;
    a.in_sn = p->in_sn; a.out_sn = p->out_sn; a.add_sn = p->add_sn; a.aux1_sn = p->aux1_sn; a.aux2_sn = p->aux2_sn;
    for (int i = 0; i < 3; ++i) {
        const int k = i < p->n_seg ? i : p->n_seg - 1;
        ITERMVS_RETURN_IF(!p->weight[k], ITERMVS_ERR_NULL);
        a.weight[i] = p->weight[k];
        a.bias[i] = p->bias[k];
        a.seg_end[i] = i < p->n_seg - 1 ? p->seg_end[i] : p->N;
    }
    a.N = p->N;
    return ITERMVS_OK;
}

// the base, then the sizes and epilogue fields that every argument block names alike
template <class Args>
static inline void fill_conv_args(Args& a, const ConvArgsBase& base, const itermvs_conv_params* p, const itermvs_conv_plan& pl) {
    static_cast<ConvArgsBase&>(a) = base;
    a.Cin = p->Cin; a.Hin = p->Hin; a.Win = p->Win; a.Cout = p->Cout; a.Hout = pl.Hout; a.Wout = pl.Wout;
    a.pad = p->pad; a.act = p->act;
}

// The ITERMVS_* overrides of a `make TUNING=1` library (tools/conv_bench.py --sweep / --sweep3); a constant in the product build.
struct ConvForce { int shape, mb; };                  // shape == INT_MIN: not forced
struct ConvTuning {
    int persist;              // persistent workgroups per CU wanted (ITERMVS_TILE_PERSIST, 4)
    ConvForce tile_force;     // ITERMVS_TILE_FORCE  "shape,mb"
    ConvForce tile3_force;    // ITERMVS_TILE3_FORCE "shape,mb"
    bool tuned;               // the measured tables of conv_tile apply (ITERMVS_TILE_TUNED)
    int min_work;             // work items the generic search of conv_tile wants (ITERMVS_TILE_MINWORK, 1024: 4 workgroups per CU)
    bool splitk;              // conv_mfma may split K (ITERMVS_CONV_SPLITK)
};
constexpr ConvTuning kConvTuningDefault = {4, {INT_MIN, 0}, {INT_MIN, 0}, true, 1024, true};
constexpr int kPairPersist = 4;           // the tap-pair form of conv_tile3 was measured at 4 only: it does not follow ITERMVS_TILE_PERSIST

// ---- LDS sizes: constexpr functions of the template arguments (the launch ladders static_assert them against the kernels' geometry) ----
constexpr int kLdsBudget = 64 * 1024;      // conv_tile, deconv: default dynamic-LDS limit; two workgroups fit a CU
constexpr int kLds3Budget = 80 * 1024;     // conv_tile3: two workgroups fit the CU's 160 KB

constexpr int tile_in_px(int stride, int dil, int th, int twt) {
    return ((th - 1) * stride + 2 * dil + 1) * ((16 * twt - 1) * stride + 2 * dil + 1);
}
constexpr int tile_plane_floats(int in_px, int s) { return (in_px * s + 63) / 64 * 64 + (s == 4 ? 0 : s == 2 ? 32 : 16); }
constexpr int tile_lds_bytes(int mb, int s, int stride, int dil, int th, int twt, int cps, int nchunk) {
    return (cps * 4 * tile_plane_floats(tile_in_px(stride, dil, th, twt), s) + nchunk * 36 * 16 * mb * s) * 4;
}
constexpr int deconv_lds_bytes(int mb, int s, int nch) { return (nch * 4 * tile_plane_floats((4 + 1) * 17, s) + nch * 36 * 16 * mb * s) * 4; }
constexpr int tile3_lds_bytes(int mb, int stride, int dil, int th, int twt, int cps, int nchunk, int taps = 9) {
    return cps * 6 * ((tile_in_px(stride, dil, th, twt) * 16 + 255) / 256 * 256) + nchunk * taps * 3 * 16 * mb * 32;
}

// tile counts of the persistent kernels (and of deconv, whose tiles are th x 16 INPUT positions)
static inline void plan_tiles(itermvs_conv_plan& pl, int n, int h, int w, int mt, int nchunk) {
    pl.tiles_x = (w + 16 * pl.TWT - 1) / (16 * pl.TWT);
    pl.tiles_y = (h + pl.TH - 1) / pl.TH;
    pl.ncb = mt / pl.MB;
    pl.nstage = pl.CPS ? (nchunk + pl.CPS - 1) / pl.CPS : 0;
    pl.total = n * pl.tiles_y * pl.tiles_x;
}

// Every plan_* returns false for "not covered" (itermvs_conv2d reports ITERMVS_ERR_DIMS: packed weights fit no other kernel).
// weight_format 0: largest channel tile that divides Cout and still leaves >= 1024 workgroups (all CT channels sit in one thread)
static inline bool plan_direct(const itermvs_conv_params* p, itermvs_conv_plan& pl) {
    int ct = 1;
    for (int c : {32, 16, 8, 4})
        if (p->Cout % c == 0) { ct = c; break; }
    while (ct > 4 && (int64_t)((pl.Hout * pl.Wout + 255) / 256) * (p->Cout / ct) * p->N < 1024) ct /= 2;
    pl.backend = ITERMVS_CONV_DIRECT;
    pl.CT = ct;
    return true;
}

// weight_format 1 (covers every 1x1 / 3x3 shape)
constexpr int kLatTH = 4, kLatTW = 64;                       // output tile of lateral_up2_kernel (rows = waves)
static inline bool plan_mfma(const itermvs_conv_params* p, const ConvTuning& t, itermvs_conv_plan& pl) {
    const int P = pl.Hout * pl.Wout;
    const int mt = (p->Cout + 15) / 16;
    // FeatureNet's lateral layers: 1x1 + bias + x2 bilinear up-sampled residual with the coarse patch staged in LDS
    if (p->ksize == 1 && p->add_mode == 1 && p->out_layout == 0 && !p->out2 && p->act == 0 && p->stride == 1 && p->pad == 0 &&
        p->n_seg == 1 && mt == 3 && !p->split_cout) {
        pl.backend = ITERMVS_CONV_LATERAL_UP2;
        pl.MB = 3;
        pl.tiles_x = (pl.Wout + kLatTW - 1) / kLatTW;
        pl.tiles_y = (pl.Hout + kLatTH - 1) / kLatTH;
        return true;
    }
    // too few tiles even at 16x16 and a k-loop long enough to split: four waves per tile (split-K)
    const int ksteps = p->ksize * p->ksize * ((p->Cin + 3) / 4);
    const int64_t tiles16 = (int64_t)p->N * ((P + 15) / 16) * mt;       // waves of the <1,1> configuration
    if (t.splitk && tiles16 < 8192 && ksteps >= 16) {
        pl.backend = ITERMVS_CONV_MFMA_SPLITK;
        pl.MB = (mt % 2 == 0 && tiles16 / 2 >= 2048) ? 2 : 1;
        return true;
    }
    // largest register blocking (MB x NB tiles of 16 channels x 16 pixels per wave) that still yields
    // >= 2048 waves (2 per SIMD): bigger tiles need fewer loads per MFMA, more waves hide latency
    struct Cfg { int mb, nb; };
    const Cfg cfgs[] = {{3, 4}, {2, 4}, {3, 2}, {2, 2}, {1, 4}, {1, 2}, {3, 1}, {2, 1}, {1, 1}};
    Cfg pick = {1, 1};
    int64_t best_waves = -1;
    for (const Cfg& c : cfgs) {
        if (mt % c.mb != 0) continue;
        const int64_t waves = (int64_t)p->N * ((P + 16 * c.nb - 1) / (16 * c.nb)) * (mt / c.mb);
        if (waves >= 2048) { pick = c; break; }
        if (waves > best_waves) { pick = c; best_waves = waves; }   // otherwise: the most waves available
    }
    pl.backend = ITERMVS_CONV_MFMA;
    pl.MB = pick.mb;
    pl.NB = pick.nb;
    return true;
}

// weight_format 2, transposed: ConvTranspose2d(3, stride 2, pad 1, output_padding 1); one tile of 4 x 16 input positions per workgroup
static inline bool plan_deconv(const itermvs_conv_params* p, itermvs_conv_plan& pl) {
    if (p->ksize != 3 || p->stride != 2 || p->pad != 1 || p->act > 1 || p->Cin <= 4 || p->Cin > 32) return false;
    const int S = p->Cin <= 8 ? 2 : 4;
    const int nchunk = (p->Cin + 4 * S - 1) / (4 * S);
    const int mt = (p->Cout + 15) / 16;
    if (mt > 2) return false;
    pl.backend = ITERMVS_CONV_DECONV;
    pl.MB = mt; pl.S = S; pl.TH = 4; pl.NCH = nchunk;         // all chunks staged at once: nchunk is 1 or 2 here
    pl.lds_bytes = deconv_lds_bytes(mt, S, nchunk);
    pl.tiles_x = (p->Win + 15) / 16;
    pl.tiles_y = (p->Hin + pl.TH - 1) / pl.TH;
    pl.ncb = 1;
    pl.total = p->N * pl.tiles_y * pl.tiles_x;
    return true;
}

// One candidate of conv_tile (t3 = false, pl.S set) / conv_tile3: tile shape 2 = 8 x 32 pixels (4 segments per wave; stride 1 only,
// conv_tile3: MB < 3 only), 1 = 4 x 32 (2), 0 = 4 x 16 (1); chunks per stage = all chunks of a 2..4-chunk layer at once when the
// stages + the block's weights fit the LDS budget, else one; LDS bytes; tile counts.  False when even that exceeds the budget.
constexpr bool conv_stride_dil_ok(int stride, int dil) { return (dil == 1 && (stride == 1 || stride == 2)) || (dil == 2 && stride == 1); }
static inline bool plan_fit(itermvs_conv_plan& pl, const itermvs_conv_params* p, bool t3, int shape, int mb, int nchunk, int mt) {
    pl.TH = shape == 2 && p->stride == 1 && !(t3 && mb == 3) ? 8 : 4;
    pl.TWT = shape == 0 ? 1 : 2;
    auto lds = [&](int cps) {
        return t3 ? tile3_lds_bytes(mb, p->stride, p->dilation, pl.TH, pl.TWT, cps, nchunk) : tile_lds_bytes(mb, pl.S, p->stride, p->dilation, pl.TH, pl.TWT, cps, nchunk);
    };
    const int budget = t3 ? kLds3Budget : kLdsBudget;
    const bool multi = t3 || pl.S == 4;
    pl.CPS = multi && nchunk == 3 && lds(3) <= budget ? 3 : multi && (nchunk == 2 || nchunk == 4) && lds(2) <= budget ? 2 : 1;
    pl.lds_bytes = lds(pl.CPS);
    pl.MB = mb; pl.STRIDE = p->stride; pl.DIL = p->dilation;
    plan_tiles(pl, p->N, pl.Hout, pl.Wout, mt, nchunk);
    return pl.lds_bytes <= budget;
}

// The (tile shape, channel blocking) a table or a search chose -> the plan: the force override, `dot` (the epilogue contracts over
// ALL output channels: one block per wave), then the first candidate whose stage + weights fit the LDS (stride-2 halos, many input
// channels): conv_tile3 tries smaller tiles first, both then narrower channel blocks.
static inline bool conv_mb_ok(const itermvs_conv_params* p, int m) { return (p->Cout + 15) / 16 % m == 0 && p->split_cout / 16 % m == 0; }
static inline bool plan_resolve(itermvs_conv_plan& pl, const itermvs_conv_params* p, bool t3, const ConvForce& f, int shape, int mb, int nchunk) {
    const int mt = (p->Cout + 15) / 16;
    const bool force = f.shape != INT_MIN, dot = p->act == 6 || p->act == 7;
    if (force) {
        shape = f.shape;
        mb = f.mb;
        if (shape < 0 || shape > 2 || mb < 1 || mb > 3 || mt % mb != 0 || (t3 && !conv_mb_ok(p, mb))) return false;
    }
    if (dot) {
        mb = mt;
        if (t3 && mb > 3) return false;
        if (!t3 && mt == 2) shape = 0;               // two blocks per wave run as 4x16 tiles
    }
    for (; mb >= 1; --mb) {
        if (dot && mb != mt) return false;
        if (!conv_mb_ok(p, mb)) continue;
        for (int sh = shape; sh >= 0; --sh) {
            if (plan_fit(pl, p, t3, sh, mb, nchunk, mt)) return true;
            if (force || !t3) break;                 // conv_tile keeps its tile shape
        }
    }
    return false;
}

// weight_format 2: exact fp32 tiles.
// Who chooses (tile shape, channel blocking) -- the measured tables speak first, the generic work-item search ("the largest tile /
// blocking that still gives min_work work items, else the most work items") only where they are silent.  With 16+ input channels
// (S = 4) that is: dilation 2 with other than three chunks and no split (the 32 -> 32 heads), and split layers at dilation 1
// whose split or total block count is odd.  Below that everything but the stride-2 layers of 5..8 input channels with even
// block counts: all of S = 1 (Cin <= 4) and the stride-1 S = 2 layers.  (And every layer when ITERMVS_TILE_TUNED=0.)
static inline bool plan_tile(const itermvs_conv_params* p, const ConvTuning& t, itermvs_conv_plan& pl) {
    if (p->ksize != 3 || !conv_stride_dil_ok(p->stride, p->dilation)) return false;
    const int hout = pl.Hout, wout = pl.Wout;
    const int S = p->Cin <= 4 ? 1 : p->Cin <= 8 ? 2 : 4;
    const int nchunk = (p->Cin + 4 * S - 1) / (4 * S);
    const int mt = (p->Cout + 15) / 16;
    int shape = -1, mb = 1;
    if (t.tuned && S == 4 && !p->split_cout) {
        // measured sweep over all (tile shape, channel blocking) pairs on the layers of the path (tools/conv_bench.py --sweep): the
        // 8x32 tile never wins there.  An even number of channel blocks runs best as 4x16 tiles with two blocks per wave (the
        // stride-2 stages, 32->32, 48->32, 32->64: -10..-25 %), an odd one as 4x32 tiles with one block (16->16, 48->48, 48->16);
        // the dilated ConvGRU convolutions as 4x32.
        if (p->dilation == 2) {
            if (nchunk == 3) { shape = 1; mb = 1; }
        } else if (mt % 2 == 0) {
            shape = 0; mb = 2;
        } else {
            shape = 1; mb = 1;
        }
    } else if (t.tuned && S == 2 && p->stride == 2 && conv_mb_ok(p, 2)) {
        shape = 0; mb = 2;                                                            // 8 -> 16+16, stride 2
    } else if (t.tuned && S == 4 && p->split_cout) {
        if (p->dilation == 2) { shape = 1; mb = 1; }                                  // z / r gates
        else if (conv_mb_ok(p, 2)) { shape = 0; mb = 2; }                                     // stride-2 conv + shortcut
    }
    if (shape < 0) {
        auto blocks = [&](int sh, int m) -> int64_t {
            const int th = sh == 2 && p->stride == 1 ? 8 : 4, tw = sh == 0 ? 16 : 32;
            return (int64_t)((hout + th - 1) / th) * ((wout + tw - 1) / tw) * (mt / m) * p->N;   // work items
        };
        // LDS bytes of a candidate when ALL chunks of a tile are staged together (the chunks-per-stage rule below picks that when it fits)
        auto full_stage_fits = [&](int sh, int m) {
            return tile_lds_bytes(m, S, p->stride, p->dilation, sh == 2 && p->stride == 1 ? 8 : 4, sh == 0 ? 1 : 2, nchunk == 4 ? 2 : nchunk, nchunk) <= kLdsBudget;
        };
        // multi-chunk layers of a few hundred tiles (the per-tile chain of barriers and weight copies bounds them; large layers
        // amortise it over big tiles): first among the candidates that stage a whole tile at once
        const bool deep = nchunk >= 2 && nchunk <= 4 && blocks(2, 1) < 1024;
        bool found = false;
        shape = 0;
        for (int pass = deep ? 0 : 1; pass < 2 && !found; ++pass) {
            int64_t best = -1;
            for (int sh = 2; sh >= 0 && !found; --sh)
                for (int m : {3, 2, 1}) {
                    if (!conv_mb_ok(p, m)) continue;
                    if (pass == 0 && !full_stage_fits(sh, m)) continue;
                    const int64_t b = blocks(sh, m);
                    if (b >= t.min_work) { shape = sh; mb = m; found = true; break; }
                    if (b > best) { best = b; shape = sh; mb = m; }
                }
            if (best >= 0) found = true;       // pass 0 found a full-stage candidate (the one with the most work items)
        }
    }
    if ((S == 1 && p->stride != 1) || (S < 4 && p->dilation != 1)) return false;      // S = 1: stride 1 only; no dilation below S = 4
    pl.backend = ITERMVS_CONV_TILE;
    pl.S = S;
    return plan_resolve(pl, p, false, t.tile_force, shape, mb, nchunk);
}

// weight_format 3: bf16x3 tiles, and the tap-pair form for 5..8 input channels
static inline bool plan_tile3(const itermvs_conv_params* p, const ConvTuning& t, itermvs_conv_plan& pl) {
    if (p->ksize != 3 || p->Cin <= 4 || !conv_stride_dil_ok(p->stride, p->dilation)) return false;
    const bool s1d1 = p->stride == 1 && p->dilation == 1;
    if (p->in_layout == 1 && !(p->Cin == 8 && s1d1)) return false;      // channels-last input: the tap-pair form only
    if (p->Cin <= 8 && !s1d1) return false;                             // the tap-pair form: stride 1, no dilation
    const int nchunk = (p->Cin + 15) / 16;
    const int mt = (p->Cout + 15) / 16;
    const bool dot = p->act == 6 || p->act == 7;
    if (p->Cin <= 8) {            // PAIR form (weights packed as five tap pairs: ops.MfmaWeight): 8 x 32 tiles, one chunk
        if (p->split_cout || (dot && mt > 2)) return false;
        pl.backend = ITERMVS_CONV_TILE3_PAIR;
        pl.MB = dot ? mt : 1;
        pl.STRIDE = 1; pl.DIL = 1; pl.TH = 8; pl.TWT = 2; pl.CPS = 1; pl.PAIR = 1;
        pl.INCL = p->in_layout;   // channels-last input: exactly 8 channels, 16-byte aligned pixels (checked in itermvs_conv2d)
        pl.lds_bytes = tile3_lds_bytes(pl.MB, 1, 1, 8, 2, 1, 1, 5);
        plan_tiles(pl, p->N, pl.Hout, pl.Wout, mt, 1);
        return true;
    }
    // Measured sweep over all (tile shape, channel blocking) pairs on the layers of the path (tools/conv_bench.py --sweep3,
    // profiles/r05/r05e_conv_tile3_sweep.txt).  A wave wants MB * NB >= 4 accumulator tiles (operand reads per MFMA, see the
    // header of conv_tile3.hip) but the split weights of a wide channel block crowd the LDS (48 -> 48 at MB = 3: 124 KB), and
    // every channel block of a tile stages and splits the tile again:
    //   dilated layers (ConvGRU, heads: 20 480 pixels, few tiles)      4x32 tiles, one block per wave
    //   48 input channels (three chunks)                               8x32 tiles, one block
    //   16 output channels                                             8x32 tiles
    //   32 output channels                                             4x16 tiles, two blocks per wave
    //   64+ output channels                                            4x16 tiles, one block
    int shape = 0, mb = 1;
    if (p->dilation == 2) shape = 1;
    else if (nchunk >= 3 || mt == 1) shape = p->stride == 1 ? 2 : 1;
    else if (mt == 2 && conv_mb_ok(p, 2)) mb = 2;
    pl.backend = ITERMVS_CONV_TILE3;
    return plan_resolve(pl, p, true, t.tile3_force, shape, mb, nchunk);
}

// The checks of itermvs_conv2d, the base of the argument block (with its weight-set check) and the plan.
static inline int conv_validate_plan(const itermvs_conv_params* p, const ConvTuning& t, ConvArgsBase* base, itermvs_conv_plan* plan) {
    ITERMVS_RETURN_IF(!p || !plan, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(!p->in || !p->out || !p->weight[0], ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(p->N < 1 || p->Cin < 1 || p->Cout < 1 || p->Hin < 1 || p->Win < 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(p->ksize != 1 && p->ksize != 3, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(p->n_seg < 1 || p->n_seg > 3 || p->act < 0 || p->act > 7, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF((p->act == 6 || p->act == 7) && (!p->aux1 || p->add || p->out2 || p->out_layout != 0 || (p->Cout != 16 && p->Cout != 32) || (p->weight_format != 2 && p->weight_format != 3) || p->ksize != 3 ||
                                      p->split_cout != 0 || p->transposed || p->n_seg != 1), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF((p->act == 4 || p->act == 5 || p->act == 6 || p->act == 7) && !p->aux1, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(p->act == 5 && !p->aux2, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(p->act >= 2 && p->add, ITERMVS_ERR_DIMS);   // residual add only with none / relu
    ITERMVS_RETURN_IF(p->add_mode < 0 || p->add_mode > 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(p->out_layout < 0 || p->out_layout > 3, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(p->in_layout != 0 && p->in_layout != 1, ITERMVS_ERR_LAYOUT);
    // channels-last input: the 8-channel tap-pair form of the bf16x3 kernel only (conv_tile3.hip)
    ITERMVS_RETURN_IF(p->in_layout == 1 && (p->weight_format != 3 || p->ksize != 3 || p->Cin != 8 || p->stride != 1 || p->dilation != 1 || p->transposed),
                      ITERMVS_ERR_LAYOUT);
    ITERMVS_RETURN_IF(p->in_layout == 1 && (((uintptr_t)p->in) % 16 || p->in_sn % 4), ITERMVS_ERR_ALIGN);
    if (p->split_cout != 0) {
        ITERMVS_RETURN_IF((p->weight_format != 2 && p->weight_format != 3) || p->transposed || p->out_layout != 0 || p->add || p->out2, ITERMVS_ERR_DIMS);
        ITERMVS_RETURN_IF(p->split_cout < 16 || p->split_cout >= p->Cout || (p->split_cout & 15), ITERMVS_ERR_DIMS);
        ITERMVS_RETURN_IF(!p->out_b || p->act_b < 0 || p->act_b > 4 || p->act > 4, ITERMVS_ERR_DIMS);
        ITERMVS_RETURN_IF(p->act_b == 4 && !p->aux1, ITERMVS_ERR_NULL);
    }
    ITERMVS_RETURN_IF(p->out_layout >= 1 && (p->weight_format == 0 || p->transposed || p->act != 0 || p->add || (p->Cout & 3)),
                      ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(p->add_mode == 1 && (!p->add || p->weight_format == 0 || p->transposed || p->act != 0), ITERMVS_ERR_DIMS);
    const int rc = fill_conv_base(*base, p);
    if (rc != ITERMVS_OK) return rc;
    itermvs_conv_plan pl = {};
    pl.KS = p->ksize;
    bool covered;
    if (p->transposed) {
        ITERMVS_RETURN_IF(p->weight_format != 2, ITERMVS_ERR_DIMS);   // transposed convolutions exist in weight_format 2 only
        pl.Hout = 2 * p->Hin; pl.Wout = 2 * p->Win;
        covered = plan_deconv(p, pl);
    } else {
        ITERMVS_RETURN_IF(p->stride < 1 || p->dilation < 1 || p->pad < 0, ITERMVS_ERR_DIMS);
        const int span = (p->ksize - 1) * p->dilation + 1;
        pl.Hout = (p->Hin + 2 * p->pad - span) / p->stride + 1;
        pl.Wout = (p->Win + 2 * p->pad - span) / p->stride + 1;
        ITERMVS_RETURN_IF(pl.Hout < 1 || pl.Wout < 1, ITERMVS_ERR_DIMS);
        ITERMVS_RETURN_IF(p->add_mode == 1 && ((pl.Hout | pl.Wout) & 1), ITERMVS_ERR_DIMS);
        covered = p->weight_format == 2   ? plan_tile(p, t, pl)      // LDS-tiled 3x3 kernels; the packed layout fits no other kernel
                  : p->weight_format == 3 ? plan_tile3(p, t, pl)     // bf16x3 split on the bf16 MFMA (3x3, more than 4 input channels)
                  : p->weight_format == 1 ? plan_mfma(p, t, pl)
                                          : plan_direct(p, pl);
    }
    ITERMVS_RETURN_IF(!covered, ITERMVS_ERR_DIMS);
    *plan = pl;
    return ITERMVS_OK;
}

}  // namespace itermvs
