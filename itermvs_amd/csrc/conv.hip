// Direct 2-D convolutions for the SMALL-channel layers of the hot path (CorrNet 8..32 channels,
// PixelViewWeight, ConvGRU 43->32, heads, FeatureNet 3..48 channels) -- models/itermvs.py:333-381,
// models/module.py:6-66, models/net.py:7-66.
//
// Why not MIOpen: at these sizes (0.05-1 GFLOP per layer) the library kernels are launch/latency
// bound (15-60 us each, plus NCHW<->NHWC transposes it inserts and separate bias / ReLU / add
// kernels); a step of the reference network spends 94 % of its GPU time there (profiles/r01_*).
//
// Design (fp32, NCHW planes, wave64):
//   * thread = one output pixel (2x2 output pixels for the stride-2 transposed conv), lanes run
//     along x so every input tap is one coalesced 256-byte wave load;
//   * a block handles CT output channels held in CT accumulators per thread; the CT weights of a
//     (ci, ky, kx) are contiguous in the packed [Cin][k][k][Cout] layout and wave-uniform, so they
//     are fetched with scalar loads and enter v_fmac as SGPR operands: the inner loop is pure
//     VALU FMA, one vector load per CT FMAs;
//   * bias, residual add, ReLU / sigmoid / tanh and the ConvGRU gate formulas are fused in the
//     epilogue (module.py:59-66), so activations are written exactly once;
//   * up to three weight sets per launch: the three CorrNets of one iteration (levels 1..3, batch
//     items [0,4), [4,8), [8,10)) run as ONE launch per layer instead of three.
// Numerics: plain fp32 fma chains in (ci, ky, kx) order -- same class of rounding as any other
// convolution back-end; parity is checked against F.conv2d in tests/test_conv_gpu.py.
#include <stdlib.h>

#include "common.hpp"
#include "conv_plan.hpp"

namespace itermvs {

struct ConvArgs : ConvArgsBase {
    int Cin, Hin, Win, Cout, Hout, Wout;
    int stride, pad, dil, act;
};
static_assert(sizeof(ConvArgs) == 192, "kernel argument layout");

__device__ __forceinline__ float epilogue(float v, int act, float add, float a1, float a2) {
    v += add;
    switch (act) {
        case 1: return fmaxf(v, 0.0f);
        case 2: return sigmoidf_(v);
        case 3: return tanhf(v);
        case 4: return sigmoidf_(v) * a1;                       // r * h            (module.py:63-64)
        case 5: return (1.0f - a2) * a1 + a2 * tanhf(v);        // (1-z) h + z q    (module.py:64-65)
        default: return v;
    }
}

template <int CT, int KS>
__global__ void __launch_bounds__(256) conv_direct_kernel(const ConvArgs a) {
    const int P = a.Hout * a.Wout;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int co0 = blockIdx.y * CT;
    const int n = blockIdx.z;
    const int seg = (n >= a.seg_end[0]) + (n >= a.seg_end[1]);
    const float* __restrict__ w = a.weight[seg] + co0;
    const float* __restrict__ bias = a.bias[seg];
    if (p >= P) return;
    const int oy = p / a.Wout, ox = p - oy * a.Wout;

    int off[KS * KS];
    bool ok[KS * KS];
#pragma unroll
    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int iy = oy * a.stride - a.pad + ky * a.dil;
            const int ix = ox * a.stride - a.pad + kx * a.dil;
            const bool in = iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
            ok[ky * KS + kx] = in;
            off[ky * KS + kx] = in ? iy * a.Win + ix : 0;
        }
    float acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = bias ? bias[co0 + c] : 0.0f;

    const float* __restrict__ ip = a.in + (int64_t)n * a.in_sn;
    const int plane = a.Hin * a.Win;
    const int wstep = KS * KS * a.Cout;
    for (int ci = 0; ci < a.Cin; ++ci) {
#pragma unroll
        for (int t = 0; t < KS * KS; ++t) {
            const float v = ok[t] ? ip[off[t]] : 0.0f;
            const float* __restrict__ wt = w + t * a.Cout;
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = fmaf(v, wt[c], acc[c]);
        }
        ip += plane;
        w += wstep;
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int64_t ch = (int64_t)(co0 + c) * P + p;
        const float ad = a.add ? a.add[(int64_t)n * a.add_sn + ch] : 0.0f;
        const float a1 = a.aux1 ? a.aux1[(int64_t)n * a.aux1_sn + ch] : 0.0f;
        const float a2 = a.aux2 ? a.aux2[(int64_t)n * a.aux2_sn + ch] : 0.0f;
        const float r = epilogue(acc[c], a.act, ad, a1, a2);
        a.out[(int64_t)n * a.out_sn + ch] = r;
        if (a.out2) a.out2[((int64_t)n * a.Cout) * P + ch] = r;
    }
}

}  // namespace itermvs

using namespace itermvs;

// the back ends: fill their argument block from the base + the plan and launch the instantiation the plan names
using ConvBackend = int(const ConvArgsBase& base, const itermvs_conv_params* p, const itermvs_conv_plan& pl, int persist, hipStream_t stream);
ConvBackend itermvs_conv2d_mfma, itermvs_conv2d_tile, itermvs_deconv2d_tile, itermvs_conv2d_tile3;   // conv_mfma.hip, conv_tile.hip (two), conv_tile3.hip

static int conv2d_direct(const ConvArgsBase& base, const itermvs_conv_params* p, const itermvs_conv_plan& pl, int, hipStream_t stream) {
    ConvArgs a;
    fill_conv_args(a, base, p, pl);
    a.stride = p->stride; a.dil = p->dilation;
    const dim3 grid((pl.Hout * pl.Wout + 255) / 256, p->Cout / pl.CT, p->N);
#define ITERMVS_DIRECT(CT_, KS_) \
    if (pl.CT == CT_ && p->ksize == KS_) hipLaunchKernelGGL((conv_direct_kernel<CT_, KS_>), grid, dim3(256), 0, stream, a);
    ITERMVS_DIRECT(32, 3) ITERMVS_DIRECT(16, 3) ITERMVS_DIRECT(8, 3) ITERMVS_DIRECT(4, 3) ITERMVS_DIRECT(1, 3)
    ITERMVS_DIRECT(32, 1) ITERMVS_DIRECT(16, 1) ITERMVS_DIRECT(8, 1) ITERMVS_DIRECT(4, 1) ITERMVS_DIRECT(1, 1)
#undef ITERMVS_DIRECT
    return itermvs_launch_status();
}

// The tuning of this call: a constant in the product build (itermvs_tuning_env is nullptr there).  A `make TUNING=1` library reads
// the switches once, except the two FORCE overrides, which tools/conv_bench.py --sweep / --sweep3 change between calls.
static ConvTuning conv_tuning() {
    static const ConvTuning fixed = [] {
        ConvTuning t = kConvTuningDefault;
        if (const char* e = itermvs_tuning_env("ITERMVS_TILE_PERSIST")) t.persist = atoi(e) < 1 ? 4 : atoi(e);
        if (const char* e = itermvs_tuning_env("ITERMVS_TILE_TUNED")) t.tuned = e[0] != '0';
        if (const char* e = itermvs_tuning_env("ITERMVS_TILE_MINWORK")) t.min_work = atoi(e);
        if (const char* e = itermvs_tuning_env("ITERMVS_CONV_SPLITK")) t.splitk = e[0] != '0';
        return t;
    }();
    ConvTuning t = fixed;
    if (const char* e = itermvs_tuning_env("ITERMVS_TILE_FORCE")) t.tile_force = {e[0] - '0', e[2] - '0'};       // "shape,mb"
    if (const char* e = itermvs_tuning_env("ITERMVS_TILE3_FORCE")) t.tile3_force = {e[0] - '0', e[2] - '0'};
    return t;
}

extern "C" int itermvs_conv2d_plan(const itermvs_conv_params* p, itermvs_conv_plan* plan) {
    ConvArgsBase base;
    return conv_validate_plan(p, conv_tuning(), &base, plan);
}

// validate, plan, launch(plan)
static int conv2d_impl(const itermvs_conv_params* p, hipStream_t stream) {
    const ConvTuning t = conv_tuning();
    ConvArgsBase base;
    itermvs_conv_plan pl;
    const int rc = conv_validate_plan(p, t, &base, &pl);
    if (rc != ITERMVS_OK) return rc;
    static ConvBackend* const backend[] = {conv2d_direct, itermvs_conv2d_mfma, itermvs_conv2d_mfma, itermvs_conv2d_mfma, itermvs_conv2d_tile,
                                           itermvs_deconv2d_tile, itermvs_conv2d_tile3, itermvs_conv2d_tile3};      // by itermvs_conv_backend
    return backend[pl.backend](base, p, pl, t.persist, stream);
}

extern "C" int itermvs_conv2d(const itermvs_conv_params* p, void* stream) {
    itermvs_profile_begin(3, (hipStream_t)stream);
    const int rc = conv2d_impl(p, (hipStream_t)stream);
    itermvs_profile_end(3, (hipStream_t)stream);
    return rc;
}
