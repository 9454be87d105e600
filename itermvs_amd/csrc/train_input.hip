// Training input side: the per-sample work of datasets/dtu_yao.py:64-119 and datasets/blendedmvs.py:62-101 on the GPU, from
// the decoded uint8 views and the raw PFM rows of the reference view.
//
// 1. ColorJitter(brightness=0.5, contrast=0.5) as torchvision applies it to a PIL image: ImageEnhance.Brightness and
//    ImageEnhance.Contrast, both Image.blend(degenerate, image, f) with f a C float:
//      blend(a, b, f) = (uint8)(a + f * (b - a))          float arithmetic, two roundings; clipped to 0..255 when f > 1
//      brightness: a = 0;  contrast: a = int(mean(L) + 0.5), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of the image
//      as it stands when contrast is applied (after brightness when brightness came first)
//    The jitter is a byte -> byte map per view, so it runs in front of image.hip's level-0 arithmetic (the same device code)
//    as a 256-entry table; pass A sums L per view in uint64 (order-independent integer atomics, one per workgroup).
// 2. Ground-truth depth / mask pyramids of the reference view: cv2.resize(INTER_NEAREST) index maps
//      src = min(floor(dst_index * (1.0 / ((double)dst / src))), src - 1)      per axis (OpenCV's published resizeNN)
//    composed per recipe, with the PFM's bottom-up row order absorbed into the map.  cv2 is not in this image: the map is
//    restated from OpenCV's source (unpinned, like image.hip's bilinear resize).
#include "flat_launch.hpp"
#include "image_level0.hpp"
#include "wave_ops.hpp"

namespace itermvs {

// Pillow's ImagingBlend for one 8-bit sample: im1 = degenerate (a), im2 = image (b)
__device__ __forceinline__ int pil_blend(int a, int b, float f) {
    const float t = (float)a + f * (float)(b - a);
    if (f >= 0.0f && f <= 1.0f) return (int)t;                 // interpolation: t lies in [min(a,b), max(a,b)]
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)t;
}

__device__ __forceinline__ int pil_l(int r, int g, int b) {     // Pillow's rgb2l (ITU-R 601-2, 16-bit fixed point)
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
}

// pass A: lsum[v] += sum of L over view v's pixels, the image taken as contrast sees it; grid (blocks, V), 256 threads
__global__ void __launch_bounds__(256) jitter_lsum_kernel(const uint8_t* __restrict__ src, int64_t npix,
                                                          const itermvs_jitter* __restrict__ jit, unsigned long long* __restrict__ lsum) {
    const int v = blockIdx.y;
    const itermvs_jitter j = jit[v];
    if (!j.enabled) return;                                   // uniform over the workgroup
    const bool bright_first = !j.contrast_first;
    const uint8_t* s = src + (int64_t)v * npix * 3;
    unsigned long long acc = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        int r = s[p * 3], g = s[p * 3 + 1], b = s[p * 3 + 2];
        if (bright_first) {
            r = pil_blend(0, r, j.brightness);
            g = pil_blend(0, g, j.brightness);
            b = pil_blend(0, b, j.brightness);
        }
        acc += (unsigned long long)pil_l(r, g, b);
    }
    acc = wave_sum_lane0(acc);
    __shared__ unsigned long long part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(lsum + v, part[0] + part[1] + part[2] + part[3]);    // vector global atomic
}

// pass B, level 0: image.hip's level-0 pixel with every source byte replaced by its jittered normalised value; grid
// (blocks, V) so that one workgroup serves one view and builds that view's 256-entry table in LDS
__global__ void __launch_bounds__(256) image_level0_jitter_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int H, int W,
                                                                  const itermvs_jitter* __restrict__ jit,
                                                                  const unsigned long long* __restrict__ lsum, float* __restrict__ out) {
    __shared__ float lut[256];
    const int v = blockIdx.y;
    const itermvs_jitter j = jit[v];
    {
        int x = threadIdx.x;                                  // blockDim.x == 256: one table entry per thread
        if (j.enabled) {
            const int mean = (int)((double)lsum[v] / (double)((int64_t)Hs * Ws) + 0.5);   // int(ImageStat mean + 0.5)
            if (j.contrast_first) {
                x = pil_blend(mean, x, j.contrast);
                x = pil_blend(0, x, j.brightness);
            } else {
                x = pil_blend(0, x, j.brightness);
                x = pil_blend(mean, x, j.contrast);
            }
        }
        lut[threadIdx.x] = normalise_u8((uint8_t)x);
    }
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)H * W) return;
    const int x = (int)(t % W), y = (int)(t / W);
    level0_pixel(src, v, Hs, Ws, H, W, x, y, out, [&](uint8_t b) { return lut[b]; });
}

__device__ __forceinline__ int nn_index(int d, int dst, int src) {      // cv2 resizeNN: x_ofs = min(cvFloor(d * ifx), src - 1)
    const double ifx = 1.0 / ((double)dst / (double)src);
    const int s = (int)floor((double)d * ifx);
    return s < src - 1 ? s : src - 1;
}

struct GtLevels {
    float* depth[4];
    float* mask[4];
};

// thread per (sample b, level l, y, x) of the four levels laid end to end; grid (blocks, B)
__global__ void __launch_bounds__(256) gt_pyramid_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ mask_src,
                                                         const float* __restrict__ params, int Hs, int Ws, int H, int W, int recipe,
                                                         GtLevels o) {
    const int b = blockIdx.y;
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int l = 0;
    for (; l < 4; ++l) {
        const int64_t n = (int64_t)(H >> l) * (W >> l);
        if (t < n) break;
        t -= n;
    }
    if (l == 4 || (!o.depth[l] && !o.mask[l])) return;
    const int h = H >> l, w = W >> l;
    const int x = (int)(t % w), y = (int)(t / w);
    const float m0 = params[b * 4 + 0], m1 = params[b * 4 + 1];
    const float* r = rows + (int64_t)b * Hs * Ws;
    int dy, dx, my, mx;
    if (recipe == ITERMVS_GT_DTU) {
        // dtu_yao.py:80-91 + 113-115: level map (W,H) -> (w,h), centre crop of the nearest x1/2 image, nearest x1/2 map
        const int hh = Hs / 2, wh = Ws / 2;
        dy = nn_index((hh - H) / 2 + nn_index(y, h, H), hh, Hs);
        dx = nn_index((wh - W) / 2 + nn_index(x, w, W), wh, Ws);
        my = dy;
        mx = dx;
    } else {
        // blendedmvs.py:69-78: depth resized to (W,H) and then to the level; the mask straight from the file size
        dy = nn_index(nn_index(y, h, H), H, Hs);
        dx = nn_index(nn_index(x, w, W), W, Ws);
        my = nn_index(y, h, Hs);
        mx = nn_index(x, w, Ws);
    }
    const int64_t o_idx = (int64_t)b * h * w + t;
    if (o.depth[l]) o.depth[l][o_idx] = (r[(int64_t)(Hs - 1 - dy) * Ws + dx] * m0) * m1;      // PFM rows are bottom-up
    if (o.mask[l]) {
        float m;
        if (recipe == ITERMVS_GT_DTU) {
            m = mask_src[((int64_t)b * Hs + my) * Ws + mx] > 10 ? 1.0f : 0.0f;                  // dtu_yao.py:93-97
        } else {
            const float d = (r[(int64_t)(Hs - 1 - my) * Ws + mx] * m0) * m1;
            m = (d >= params[b * 4 + 2] && d <= params[b * 4 + 3]) ? 1.0f : 0.0f;             // blendedmvs.py:67
        }
        o.mask[l][o_idx] = m;
    }
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_image_pyramid_jitter(const uint8_t* src, int32_t V, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                                            const itermvs_jitter* jitter, uint64_t* lsum, float* level0, float* level1,
                                            float* level2, float* level3, void* stream) {
    ITERMVS_RETURN_IF(!src || !jitter || !lsum || !level0, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(V < 1 || V > 65535 || Hs < 1 || Ws < 1 || H < 1 || W < 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF((level1 || level2 || level3) && ((H | W) & 7), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(Ws > kFlatInt32 / 3, ITERMVS_ERR_DIMS);            // level0_pixel forms x * 3 + c of a source row in an int
    // both grids before the first HIP call: level 0 with the view in grid.y, the levels below (fewer items than V * H * W) without
    const FlatItems n0{flat_items({H, W}), kFlatMaxWork, V};
    dim3 unused;
    ITERMVS_RETURN_IF(flat_grid(n0, 256, &unused) || flat_grid({flat_items({V, H, W})}, 256, &unused), ITERMVS_ERR_DIMS);
    const hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)Hs * Ws;
    if (hipMemsetAsync(lsum, 0, sizeof(uint64_t) * (size_t)V, st) != hipSuccess) return ITERMVS_ERR_LAUNCH;
    const int64_t lb = (npix + 255) / 256;
    hipLaunchKernelGGL(jitter_lsum_kernel, dim3((unsigned)(lb < 64 ? lb : 64), (unsigned)V), dim3(256), 0, st, src, npix, jitter,
                       (unsigned long long*)lsum);
    int rc = flat_launch<image_level0_jitter_kernel, 256>(n0, st, src, Hs, Ws, H, W, jitter, (const unsigned long long*)lsum, level0);
    float* lv[3] = {level1, level2, level3};
    for (int l = 1; l <= 3 && rc == ITERMVS_OK; ++l)
        if (lv[l - 1]) rc = image_pyramid_down(level0, V * 3, H, W, l, lv[l - 1], st);
    return rc;
}

extern "C" int itermvs_gt_pyramid(const float* depth_rows, const uint8_t* mask_src, const float* params, int32_t B, int32_t Hs,
                                  int32_t Ws, int32_t H, int32_t W, int32_t recipe, float* depth0, float* depth1, float* depth2,
                                  float* depth3, float* mask0, float* mask1, float* mask2, float* mask3, void* stream) {
    ITERMVS_RETURN_IF(!depth_rows || !params, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(recipe != ITERMVS_GT_DTU && recipe != ITERMVS_GT_BLENDEDMVS, ITERMVS_ERR_DIMS);
    const bool any_mask = mask0 || mask1 || mask2 || mask3;
    ITERMVS_RETURN_IF(recipe == ITERMVS_GT_DTU && any_mask && !mask_src, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(B < 1 || B > 65535 || Hs < 1 || Ws < 1 || H < 8 || W < 8 || ((H | W) & 7), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF((int64_t)Hs * Ws > 0x7fffffffLL, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(recipe == ITERMVS_GT_DTU && (Hs / 2 < H || Ws / 2 < W), ITERMVS_ERR_DIMS);   // the crop lies inside
    GtLevels o = {{depth0, depth1, depth2, depth3}, {mask0, mask1, mask2, mask3}};
    int64_t n = 0;
    for (int l = 0; l < 4; ++l) n += (int64_t)(H >> l) * (W >> l);
    return flat_launch<gt_pyramid_kernel, 256>({n, kFlatMaxWork, B}, (hipStream_t)stream, depth_rows, mask_src, params, Hs, Ws, H, W, recipe, o);
}
