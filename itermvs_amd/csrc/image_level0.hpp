// Level-0 arithmetic of the image pyramid (image.hip), shared by itermvs_image_pyramid and the training input side
// (train_input.hip): one output pixel of cv2.resize(2 * src / 255. - 1, (W, H), INTER_LINEAR), with the normalised value
// of a source byte supplied by the caller (image.hip: normalise_u8; train_input.hip: a per-view ColorJitter table).
#pragma once
#include "common.hpp"

namespace itermvs {

__device__ __forceinline__ void resize_axis(int d, double scale, int n_src, int& s0, int& s1, float& a0, float& a1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.0f; s = 0; }
    if (s >= n_src - 1) { f = 0.0f; s = n_src - 1; }
    s0 = s;
    s1 = s + 1 < n_src ? s + 1 : n_src - 1;
    a0 = 1.0f - f;
    a1 = f;
}

__device__ __forceinline__ float normalise_u8(uint8_t v) {   // 2 * x / 255. - 1, float32 op by op
    return (2.0f * (float)v) / 255.0f - 1.0f;
}

// pixel (v, y, x) of level 0; src [V,Hs,Ws,3] uint8 interleaved RGB; out [V,3,H,W] float32 planes; value(byte) -> float
template <class Value>
__device__ __forceinline__ void level0_pixel(const uint8_t* __restrict__ src, int v, int Hs, int Ws, int H, int W, int x, int y,
                                             float* __restrict__ out, Value value) {
    int x0, x1, y0, y1;
    float ax0, ax1, ay0, ay1;
    resize_axis(x, (double)Ws / (double)W, Ws, x0, x1, ax0, ax1);
    resize_axis(y, (double)Hs / (double)H, Hs, y0, y1, ay0, ay1);
    const uint8_t* s = src + (int64_t)v * Hs * Ws * 3;
    const uint8_t* r0 = s + (int64_t)y0 * Ws * 3;
    const uint8_t* r1 = s + (int64_t)y1 * Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = value(r0[x0 * 3 + c]) * ax0 + value(r0[x1 * 3 + c]) * ax1;   // horizontal pass
        const float bot = value(r1[x0 * 3 + c]) * ax0 + value(r1[x1 * 3 + c]) * ax1;
        out[(((int64_t)v * 3 + c) * H + y) * W + x] = top * ay0 + bot * ay1;            // vertical pass
    }
}

// enqueue image.hip's level-l kernel (l = 1..3) over level 0 [M,H,W] -> out [M,H>>l,W>>l]; returns an ITERMVS_* status
int image_pyramid_down(const float* level0, int M, int H, int W, int lvl, float* out, hipStream_t stream);

}  // namespace itermvs
