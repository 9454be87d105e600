// itermvs_resize_rgb8: Pillow's Image.resize(size, Image.BILINEAR) of 8-bit RGB images on the GPU, bit for bit -- the vertex
// colours of the fusion (fusion.read_scan_image(as_uint8=True)) from the uint8 upload the input side already makes.
//
// Pillow's 8-bit resample (src/libImaging/Resample.c) is integer arithmetic on per-axis coefficient tables; only the tables
// involve floating point and the host computes them (itermvs_amd/resize.py).  Per axis and output index: the first input
// sample, a tap count and the taps as integers with 22 fractional bits.  A pass is
//     clip(((1 << 21) + sum(pixel[first + t] * k[t])) >> 22, 0, 255)
// horizontal first, its rounded uint8 result feeding the vertical pass.  An axis that keeps its size has the identity table
// (one tap of 1 << 22), which returns the pixel: Pillow skips that pass.  The sums fit int32 like Pillow's (255 * ~2^22).
//
// One launch, no intermediate image: a thread recomputes the horizontal results its vertical taps need (5 x 5 taps for DTU's
// 1600 x 1200 -> anything smaller, 1 x 3 for 1200 -> 1152 rows).  Four neighbouring pixels per thread make the store
// 12 contiguous bytes (three dwords) when the rows allow it; when the width is also kept, the 12 source bytes of each vertical
// tap are three dword loads.  Otherwise one pixel per thread with byte accesses.
#include "flat_launch.hpp"

namespace itermvs {

constexpr int kResizeBlock = 256;

__device__ __forceinline__ int resize_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct ResizeTables {
    const int32_t* xb;   // [W,2] first input column, tap count
    const int32_t* xk;   // [W,KX]
    const int32_t* yb;   // [H,2]
    const int32_t* yk;   // [H,KY]
    int KX, KY;
};

// the horizontal pass of one output pixel on one source row -> 3 channels (uint8 values)
__device__ __forceinline__ void resize_row(const uint8_t* __restrict__ row, int Ws, int first, int count,
                                           const int32_t* __restrict__ k, int& r, int& g, int& b) {
    int ar = 1 << 21, ag = 1 << 21, ab = 1 << 21;
    for (int t = 0; t < count; ++t) {
        const int sx = min(first + t, Ws - 1);          // tables from the host never leave the row; a bad table must not either
        const uint8_t* p = row + (int64_t)sx * 3;
        const int kt = k[t];
        ar += p[0] * kt;
        ag += p[1] * kt;
        ab += p[2] * kt;
    }
    r = resize_clip8(ar);
    g = resize_clip8(ag);
    b = resize_clip8(ab);
}

// PX output pixels of one row per thread.  PX = 4 needs W % 4 == 0 and a 4-byte aligned `out`; SAME_W (the width is kept:
// the horizontal pass is the identity) additionally needs a 4-byte aligned `src` and reads dwords.
template <int PX, bool SAME_W>
__global__ void __launch_bounds__(kResizeBlock) resize_rgb8_kernel(const uint8_t* __restrict__ src, int V, int Hs, int Ws, int H,
                                                                   int W, ResizeTables tb, uint8_t* __restrict__ out) {
    const int wq = W / PX;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)V * H * wq) return;
    const int x0 = (int)(t % wq) * PX, y = (int)((t / wq) % H), v = (int)(t / ((int64_t)wq * H));
    const int yfirst = max(tb.yb[2 * y], 0), ycount = min(tb.yb[2 * y + 1], tb.KY);
    const int32_t* ky = tb.yk + (int64_t)y * tb.KY;
    int acc[PX * 3];
#pragma unroll
    for (int i = 0; i < PX * 3; ++i) acc[i] = 1 << 21;
    for (int ty = 0; ty < ycount; ++ty) {
        const int sy = min(yfirst + ty, Hs - 1);
        const uint8_t* row = src + ((int64_t)v * Hs + sy) * Ws * 3;
        const int kv = ky[ty];
        if constexpr (SAME_W) {
            static_assert(PX == 4, "the dword path handles four pixels");
            const uint32_t* q = reinterpret_cast<const uint32_t*>(row + (int64_t)x0 * 3);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const uint32_t u = q[d];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * d + j] += (int)((u >> (8 * j)) & 0xffu) * kv;
            }
        } else {
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const int x = x0 + p;
                const int first = max(tb.xb[2 * x], 0), count = min(tb.xb[2 * x + 1], tb.KX);
                int r, g, b;
                resize_row(row, Ws, first, count, tb.xk + (int64_t)x * tb.KX, r, g, b);
                acc[3 * p + 0] += r * kv;
                acc[3 * p + 1] += g * kv;
                acc[3 * p + 2] += b * kv;
            }
        }
    }
    uint8_t* o = out + (((int64_t)v * H + y) * W + x0) * 3;
    if constexpr (PX == 4) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            uint32_t u = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) u |= (uint32_t)resize_clip8(acc[4 * d + j]) << (8 * j);
            o4[d] = u;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PX * 3; ++i) o[i] = (uint8_t)resize_clip8(acc[i]);
    }
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_resize_rgb8(const uint8_t* src, int32_t V, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                                   const int32_t* xbounds, const int32_t* xk, int32_t KX, const int32_t* ybounds,
                                   const int32_t* yk, int32_t KY, uint8_t* out, void* stream) {
    ITERMVS_RETURN_IF(!src || !out || !xbounds || !xk || !ybounds || !yk, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(V < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || KX < 1 || KY < 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(H > kFlatInt32 / 2 || W > kFlatInt32 / 2, ITERMVS_ERR_DIMS);      // the kernel forms 2 * y and 2 * x in an int
    const bool wide = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 4 == 0);
    const bool same_w = wide && Ws == W && KX == 1 && (reinterpret_cast<uintptr_t>(src) % 4 == 0);
    const FlatItems n{flat_items({V, H, wide ? W / 4 : W})};
    const ResizeTables tb{xbounds, xk, ybounds, yk, KX, KY};
    const hipStream_t s = (hipStream_t)stream;
    if (same_w) return flat_launch<resize_rgb8_kernel<4, true>, kResizeBlock>(n, s, src, V, Hs, Ws, H, W, tb, out);
    if (wide) return flat_launch<resize_rgb8_kernel<4, false>, kResizeBlock>(n, s, src, V, Hs, Ws, H, W, tb, out);
    return flat_launch<resize_rgb8_kernel<1, false>, kResizeBlock>(n, s, src, V, Hs, Ws, H, W, tb, out);
}
