// itermvs_down_conv: the stride-2 pair of a FeatureNet residual block (models/module.py:33-50: conv1 + ReLU and the down-sampling
// shortcut read the same input) as ONE cooperative launch:
//     y  = relu(conv3x3_s2(x; W1) + b1)      sc = conv3x3_s2(x; Wd) + bd            both [N,C,(H-1)/2+1,(W-1)/2+1]
// for the two shapes of the path, 16 -> 32+32 (layer2.0) and 32 -> 48+48 (layer3.0).
// As itermvs_conv2d launches every block of 16 (32) output channels was a workgroup column of its own: the halo tile of a
// stride-2 layer -- 9 x 33 input pixels for 4 x 16 outputs -- was fetched, written to LDS and synchronised two (six) times, and the
// layers stayed on the fp32 matrix instruction because the split form re-split the tile as often (ops.py, profiles/r06/r06l_*).
// Here -- the work split of gru.hip -- a persistent workgroup owns a TH x 16 tile of output pixels and ALL 2C/16 output blocks:
// wave w = (output block w % NOB, pixel part w / NOB) keeps the split weights of its block in registers (9 taps x 3 operands)
// and multiplies the tile's rows of its part; the tile is fetched, split and stored once.
// Arithmetic: the bf16x3 form of conv_tile3.hip (operands split exactly into three bf16 terms, the six largest cross products on
// v_mfma_f32_16x16x32_bf16, fp32 accumulation, small terms first):
//   16 input channels   K = 32 = two 16-channel terms side by side: A1 = [wh | wh], A2 = [wm | wm], A3 = [wl | wh],
//                       B1 = [xh | xm], B3 = [xh | xl]: three MFMAs per tap;
//   32 input channels   K = 32 = the 32 channels of ONE term: wl xh, wh xl, wm xm, wm xh, wh xm, wh xh: six MFMAs per tap.
// LDS image of a tile (input rows 2 oy0 - 1 .. 2 (oy0 + TH) - 1, columns 2 ox0 - 1 .. 2 ox0 + 31), space-to-depth:
//   [term h, m, l][group of 8 channels][class (row parity, column parity)][row / 2][column / 2][8 bf16]
// so that tap (ky, kx) of 16 consecutive output pixels is 16 consecutive 16-byte positions of class (ky & 1, kx & 1), displaced
// by (ky >> 1, kx >> 1): conflict-free ds_read_b128 at lane base + immediate.  (term, group) planes are multiples of 256 bytes
// (the 16-lane groups of a ds_read_b128 mix two lane quarters = two planes); a class is 64 mod 128 bytes, so that the 8-lane
// groups of a staging ds_write_b128 -- consecutive input columns, alternating column parity -- cover all 32 banks.
// Two such images: between two barriers a wave splits and stores tile i + 1 (fetched one iteration ago), multiplies tile i with
// the loads of tile i + 2 spread over the taps (never a burst: DESIGN.md section 4, lat_conv), and stores tile i's results.
#include "common.hpp"
#include "tile_walk.hpp"

namespace itermvs {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr uint32_t kDcOob = 0x7fffffffu;                    // byte offset past any input (Cin H W 4 <= 2^30)

struct DownConvArgs {
    const float* x;          // [N,CIN,H,W] planes
    int64_t x_sn;
    const void* w;           // bf16 [tap 9][chunk CIN/16][term 3][2C][16]  (weight_format 3 of itermvs_conv2d)
    const float* bias;       // [2C] or nullptr
    float* y;                // [N,C,Ho,Wo] planes: channels 0 .. C-1, ReLU
    int64_t y_sn;
    float* sc;               // [N,C,Ho,Wo] planes: channels C .. 2C-1
    int64_t sc_sn;
    int H, W, Ho, Wo, tiles_x, tiles_y;
    int run, run_extra;      // a workgroup's run of tiles: tiles / grid, the first tiles % grid workgroups one more
    int banded;
};

template <int CIN, int NOB, int PH, int TH>
struct DownGeom {
    static constexpr int KG = CIN / 8;                              // groups of 8 channels
    static constexpr int THREADS = 64 * NOB * PH;
    static constexpr int NB = TH / PH;                              // output rows (16-pixel segments) of a wave
    static constexpr int IN_H = 2 * TH + 1, IN_W = 33, IN_PX = IN_H * IN_W;
    static constexpr int CP = ((TH + 1) * 17 - 4 + 7) / 8 * 8 + 4;  // positions of a parity class: (TH + 1) x 17, rounded up to 4 mod 8
    static constexpr int CSB = CP * 16;                             // bytes per class
    static constexpr int PLB = 4 * CSB;                             // bytes per (term, channel group): a multiple of 256
    static constexpr int BUFB = 3 * KG * PLB;                       // one tile
    static constexpr int LDS = 2 * BUFB;
    static constexpr int ITEMS = KG * IN_PX;                        // staging items (channel group, input pixel)
    static constexpr int NIT = (ITEMS + THREADS - 1) / THREADS;     // ... per thread
    static_assert(TH % PH == 0 && PLB % 256 == 0 && CSB % 128 == 64 && LDS <= 160 * 1024, "tile geometry");
};

struct DownTile { int n, tx, ty; };

template <int CIN, int NOB, int PH, int TH>
__global__ void __launch_bounds__(64 * NOB * PH) down_conv_kernel(const DownConvArgs a) {
    using G = DownGeom<CIN, NOB, PH, TH>;
    constexpr int KG = G::KG, NB = G::NB, NIT = G::NIT, PLB = G::PLB, CSB = G::CSB;
    constexpr int NCH = CIN / 16, CPAD = 16 * NOB;            // input chunks and output channels of the packed weight
    constexpr int NA = 3;                                     // weight operands per tap
    constexpr int NBO = CIN == 16 ? 2 : 3;                    // pixel operands per (tap, segment)
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, l16 = lane & 15;
    const int half = q & 1, second = q >> 1;
    const int ob = wave % NOB, ph = wave / NOB;
    const uint32_t plane = (uint32_t)(a.H * a.W);
    const int P = a.Ho * a.Wo;

    // this workgroup's run of tiles, in the order (image, tile column, tile row): a run walks down a column.  Banded
    // (tile_walk.hpp), the runs of one XCD are neighbours in the tile list and share their halos in that XCD's L2
    const TileRun mine = tile_walk_run(a.run, a.run_extra, blockIdx.x, gridDim.x, a.banded);
    const int t0 = mine.t0;
    int left = mine.count;                                    // tiles not yet fetched
    auto advance = [&](DownTile t) {
        if (++t.ty == a.tiles_y) {
            t.ty = 0;
            if (++t.tx == a.tiles_x) { t.tx = 0; ++t.n; }
        }
        return t;
    };
    DownTile cur;
    {
        const int per = a.tiles_x * a.tiles_y;
        cur.n = t0 / per;
        const int r = t0 - cur.n * per;
        cur.tx = r / a.tiles_y;
        cur.ty = r - cur.tx * a.tiles_y;
    }

    // staging items of this thread: (channel group, pixel of the input tile): 8 channels = eight dword loads (consecutive lanes =
    // consecutive columns), split, three 16-byte LDS stores
    int rel[NIT], loff[NIT];
    uint32_t reloff[NIT];
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
        const int item = tid + j * G::THREADS;
        const bool live = item < G::ITEMS;
        const int kg = live ? item / G::IN_PX : 0;
        const int px = live ? item - kg * G::IN_PX : 0;
        const int y = px / G::IN_W, x = px - y * G::IN_W;
        rel[j] = live ? (y << 12) | x : -1;
        reloff[j] = live ? ((uint32_t)(kg * 8) * plane + (uint32_t)(y * a.W + x)) * 4u : kDcOob;
        loff[j] = kg * PLB + ((y & 1) * 2 + (x & 1)) * CSB + ((y >> 1) * 17 + (x >> 1)) * 16;
    }
    uint32_t goff[NIT];
    __amdgpu_buffer_rsrc_t ir;
    // padding = the buffer's bounds: an item outside the image gets an offset past the end and loads zeros
    auto setup = [&](const DownTile& t) {
        ir = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x + (int64_t)t.n * a.x_sn), 0, (int)((uint32_t)CIN * plane * 4u), 0x00020000);
        const int iy0 = t.ty * (2 * TH) - 1, ix0 = t.tx * 32 - 1;
        const int base = (iy0 * a.W + ix0) * 4;
        if (iy0 >= 0 && ix0 >= 0 && iy0 + G::IN_H <= a.H && ix0 + G::IN_W <= a.W) {
#pragma unroll
            for (int j = 0; j < NIT; ++j) goff[j] = rel[j] >= 0 ? reloff[j] + (uint32_t)base : kDcOob;
        } else {
#pragma unroll
            for (int j = 0; j < NIT; ++j) {
                const int gy = iy0 + (rel[j] >> 12), gx = ix0 + (rel[j] & 0xfff);
                const bool ok = rel[j] >= 0 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
                goff[j] = ok ? reloff[j] + (uint32_t)base : kDcOob;
            }
        }
    };
    float stage[NIT][8];
    constexpr int kLoads = NIT * 8, kParts = 9;
    auto fetch_part = [&](int part) {
#pragma unroll
        for (int e = 0; e < kLoads; ++e)
            if (e * kParts / kLoads == part) {
                const int j = e / 8, k = e % 8;
                stage[j][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ir, goff[j], (uint32_t)k * plane * 4u, 0));
            }
    };
    auto stash = [&](char* __restrict__ buf) {
#pragma unroll
        for (int j = 0; j < NIT; ++j)
            if (j < NIT - 1 || tid + j * G::THREADS < G::ITEMS) {
                u32x4 Hh, Mm, Ll;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t h, m, l;
                    split_pair(stage[j][2 * k], stage[j][2 * k + 1], h, m, l);
                    Hh[k] = h; Mm[k] = m; Ll[k] = l;
                }
                char* d = buf + loff[j];
                *reinterpret_cast<u32x4*>(d) = Hh;
                *reinterpret_cast<u32x4*>(d + KG * PLB) = Mm;
                *reinterpret_cast<u32x4*>(d + 2 * KG * PLB) = Ll;
            }
    };

    setup(cur);
#pragma unroll
    for (int part = 0; part < kParts; ++part) fetch_part(part);             // in flight together with the weights
    --left;

    // this wave's weights, all in registers.  16 channels: A1 = [wh | wh], A2 = [wm | wm], A3 = [wl | wh] (lane quarter q:
    // term by q >> 1, channels 8 (q & 1) ..); 32 channels: terms h, m, l of channels 8 q .. 8 q + 7
    bf8 wreg[9][NA];
    {
        const bf8* __restrict__ src = reinterpret_cast<const bf8*>(a.w);
        const int chunk = CIN == 16 ? 0 : second;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int o = 0; o < NA; ++o) {
                // operand o of the MFMA sequence below
                const int term = CIN == 16 ? (o == 0 ? (second ? 0 : 2) : o == 1 ? 1 : 0) : 2 - o;       // 16: A3, A2, A1;  32: l, m, h
                wreg[tap][o] = src[(((tap * NCH + chunk) * 3 + term) * CPAD + ob * 16 + l16) * 2 + half];
            }
    }
    float bsv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bsv[r] = a.bias ? a.bias[ob * 16 + q * 4 + r] : 0.0f;

    stash(dsm);
    DownTile nxt = cur;
    bool more1 = left > 0;                        // a tile after cur exists (and is in the staging registers)
    if (more1) {
        nxt = advance(cur);
        setup(nxt);
#pragma unroll
        for (int part = 0; part < kParts; ++part) fetch_part(part);
        --left;
    }

    // pixel operands of this lane: position (row ph * NB, column l16) of class 0 in its planes
    const int pos0 = ((ph * NB) * 17 + l16) * 16;
    int bo[NBO];
    if constexpr (CIN == 16) {
        bo[0] = ((second ? 2 : 0) * KG + half) * PLB + pos0;      // B3 = [xh | xl]
        bo[1] = ((second ? 1 : 0) * KG + half) * PLB + pos0;      // B1 = [xh | xm]
    } else {
#pragma unroll
        for (int t = 0; t < 3; ++t) bo[t] = (t * KG + q) * PLB + pos0;      // xh, xm, xl
    }

    for (int it = 0;; ++it) {
        __syncthreads();            // tile `it` is staged; the other image is free (its readers finished the previous iteration)
        const char* __restrict__ buf = dsm + (it & 1) * G::BUFB;
        const bool more = more1;
        DownTile nn = nxt;
        bool prefetch = false;
        if (more) {
            stash(dsm + ((it + 1) & 1) * G::BUFB);
            more1 = left > 0;
            if (more1) {
                nn = advance(nxt);
                setup(nn);
                --left;
                prefetch = true;
            }
        }
        f32x4 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{bsv[0], bsv[1], bsv[2], bsv[3]};
        __builtin_amdgcn_sched_barrier(0);
        // one step = (tap, segment); the operands of step v + 1 are read from LDS before the MFMAs of step v
        bf8 b[2][NBO];
        auto read_operands = [&](int v, int set) {
            const int u = v / NB, nb = v - u * NB;
            const int ky = u / 3, kx = u - ky * 3;
            const int o = ((ky & 1) * 2 + (kx & 1)) * CSB + ((nb + (ky >> 1)) * 17 + (kx >> 1)) * 16;
#pragma unroll
            for (int t = 0; t < NBO; ++t) b[set][t] = *reinterpret_cast<const bf8*>(buf + bo[t] + o);
        };
        read_operands(0, 0);
#pragma unroll
        for (int v = 0; v < 9 * NB; ++v) {
            const int u = v / NB, nb = v - u * NB, s = v & 1;
            if (v + 1 < 9 * NB) read_operands(v + 1, s ^ 1);
            if (prefetch && nb == 0) fetch_part(u);
            if constexpr (CIN == 16) {
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[u][0], b[s][0], acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[u][1], b[s][1], acc[nb], 0, 0, 0);
                acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[u][2], b[s][1], acc[nb], 0, 0, 0);
            } else {
                // (weight operand, pixel term): wl xh, wh xl, wm xm, wm xh, wh xm, wh xh
                constexpr int kW[6] = {0, 2, 1, 1, 2, 2}, kX[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int p = 0; p < 6; ++p) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[u][kW[p]], b[s][kX[p]], acc[nb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }

        // D: column (pixel) = lane & 15, row (output channel of the block) = 4 q + r
        {
            const bool first = ob * 16 < NOB * 8;           // block of conv1 (ReLU) or of the shortcut
            float* __restrict__ dst = first ? a.y + (int64_t)cur.n * a.y_sn + (size_t)(ob * 16 + q * 4) * P
                                            : a.sc + (int64_t)cur.n * a.sc_sn + (size_t)(ob * 16 - NOB * 8 + q * 4) * P;
            const int ox = cur.tx * 16 + l16;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int oy = cur.ty * TH + ph * NB + nb;
                if (oy < a.Ho && ox < a.Wo) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[(size_t)r * P + (size_t)oy * a.Wo + ox] = first ? fmaxf(acc[nb][r], 0.0f) : acc[nb][r];
                }
            }
        }
        if (!more) break;
        cur = nxt;
        nxt = nn;
    }
}

template <int CIN, int NOB, int PH, int TH>
static int launch_down(DownConvArgs& a, int N, hipStream_t stream) {
    using G = DownGeom<CIN, NOB, PH, TH>;
    a.tiles_x = (a.Wo + 15) / 16;
    a.tiles_y = (a.Ho + TH - 1) / TH;
    PersistentPlan plan;            // one workgroup per CU (the weights take 108 registers per lane)
    const int rc = persistent_plan_cus((int64_t)a.tiles_x * a.tiles_y * N, 1, true, ITERMVS_WALK_RUNS, &plan);
    if (rc != ITERMVS_OK) return rc;
    a.run = plan.run; a.run_extra = plan.run_extra; a.banded = plan.banded;
    return launch_fused<down_conv_kernel<CIN, NOB, PH, TH>, G::LDS>(dim3(plan.grid), G::THREADS, stream, true, a);
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_down_conv(const float* x, int64_t x_sn, int32_t N, int32_t Cin, int32_t H, int32_t W, const void* w_packed,
                                 const float* bias, int32_t C, float* y, int64_t y_sn, float* sc, int64_t sc_sn, void* stream) {
    ITERMVS_RETURN_IF(!x || !w_packed || !y || !sc, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(N < 1 || H < 1 || W < 1 || H > 4095 || W > 4095, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(!((Cin == 16 && C == 32) || (Cin == 32 && C == 48)), ITERMVS_ERR_CHANNELS);
    ITERMVS_RETURN_IF((int64_t)Cin * H * W * 4 > ((int64_t)1 << 30), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(((uintptr_t)w_packed) % 16, ITERMVS_ERR_ALIGN);
    DownConvArgs a;
    a.x = x; a.x_sn = x_sn; a.w = w_packed; a.bias = bias; a.y = y; a.y_sn = y_sn; a.sc = sc; a.sc_sn = sc_sn;
    a.H = H; a.W = W; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
    // (output blocks, pixel parts, tile rows) by measurement at the cfg-1 shapes (tools/down_conv_bench.py):
    // 16 -> 64: 8 waves on 4 x 16 tiles (8 x 16: the same; 2 x 16: +2.2 us; 4 waves: +1.2 us);
    // 32 -> 96: 12 waves on 2 x 16 tiles (6 waves on 4 x 16: +1.7 us, on 2 x 16: +1.1 us; 12 waves on 4 x 16 spill)
    if (Cin == 16) return launch_down<16, 4, 2, 4>(a, N, (hipStream_t)stream);
    return launch_down<32, 6, 2, 2>(a, N, (hipStream_t)stream);
}
