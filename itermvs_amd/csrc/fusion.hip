// itermvs_fuse_depth: geometric + photometric filter of one reference view against its source views --
// reproject_with_depth (eval.py:154-194), check_geometric_consistency (eval.py:197-212) and the per-reference
// arithmetic of filter_depth (eval.py:238-269) in ONE pass: a thread owns a reference pixel, walks the S source
// views and keeps the consistency count and the depth sum in registers; no per-view reprojection maps or masks
// ever reach memory (the reference materialises six [H,W] float64/float32 arrays per pair).
// Arithmetic mirrors numpy's promotion rules in the reference: pixel grid int64, depths float32, camera matrices
// float32 (inverted / composed on the host exactly like eval.py does), every product with a point in float64 (cam_math.hpp);
// cv2.remap(INTER_LINEAR) as published (1/32-pixel coordinates, float32 weights, zero border).  oracle/fusion_oracle.py
// is the CPU restatement the tests compare against, bit for bit.
// itermvs_fuse_depth_claim is the same per-pixel body (fuse_pixel<true>) with the claim step of include/itermvs_hip.h behind it:
// a pixel that another view's emitted point was verified against is marked and never emits a copy of that point.
// itermvs_fuse_depth_dynamic is that body once more (fuse_pixel<true, true>) with the level rule of include/itermvs_hip.h in
// place of the count against geo_mask_thres: the per-source errors are in registers already, so the rule costs no memory traffic.
#include <math.h>

#include "cam_math.hpp"

namespace itermvs {

struct FuseArgs {
    const float* depth_ref;
    const float* conf_ref;
    const float* depth_src[ITERMVS_MAX_SRC];
    const float* mats;      // [S][60]: a_ref(9) t_rs(12, rows 0..2) k_src(9) a_src(9) t_sr(12) k_ref(9), float32
    double* depth_avg;
    uint8_t* photo_mask;
    uint8_t* geo_mask;
    uint8_t* final_mask;
    int32_t* geo_sum;
    int S, H, W, geo_mask_thres;
    double geo_pixel_thres;
    float geo_depth_thres, photo_thres;
};

__device__ __forceinline__ long long remap_fixed(float c) {   // cvRound(c * 32) with saturate_cast<int>
    const double v = (double)c * 32.0;
    if (!isfinite(v)) return -2147483648LL;
    const double r = rint(v);
    return r > 2147483647.0 ? 2147483647LL : (r < -2147483648.0 ? -2147483648LL : (long long)r);
}

__device__ __forceinline__ float remap_bilinear(const float* __restrict__ src, int H, int W, float mx, float my) {
    const long long sx = remap_fixed(mx), sy = remap_fixed(my);
    const long long ix = sx >> 5, iy = sy >> 5;
    const float fx = (float)(sx & 31) * (1.0f / 32.0f), fy = (float)(sy & 31) * (1.0f / 32.0f);
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    auto tap = [&](long long yy, long long xx) {
        return (xx >= 0 && xx < W && yy >= 0 && yy < H) ? src[yy * W + xx] : 0.0f;
    };
    float out = tap(iy, ix) * (wy0 * wx0);
    out = out + tap(iy, ix + 1) * (wy0 * fx);
    out = out + tap(iy + 1, ix) * (fy * wx0);
    out = out + tap(iy + 1, ix + 1) * (fy * fx);
    return out;
}

struct FuseClaimArgs {
    FuseArgs f;
    const uint8_t* claimed_ref;                  // [H,W] of the reference view, or null: nothing is claimed yet
    uint8_t* claimed_src[ITERMVS_MAX_SRC];       // [H,W] per source view; claimed_src[0] null: the claim step is skipped
};

struct FuseDynArgs {
    double pixel_step;                           // a: a source passes level n iff dist < (double)n * a && rel < (float)n * b
    float depth_step;                            // b
    int n_min, n_max;
    uint8_t* geo_level;                          // [H,W] or null
};

// reference pixel (px, py, d) = (x * d, y * d, d) -> its position in the source view of `m`, float64   (eval.py:162-169)
__device__ __forceinline__ void project_to_source(const float* __restrict__ m, double px, double py, double d, double& xs,
                                                  double& ys) {
    double rx, ry, rz, sx, sy, sz, kx, ky, kz;
    mat3(m, px, py, d, rx, ry, rz);                    // reference 3-D space      (eval.py:162-163)
    mat34(m + 9, rx, ry, rz, sx, sy, sz);              // source 3-D space         (eval.py:165-166)
    mat3(m + 21, sx, sy, sz, kx, ky, kz);              // source pixel             (eval.py:168-169)
    xs = kx / kz;
    ys = ky / kz;
}

// One reference pixel.  Claim = false is itermvs_fuse_depth; Claim = true adds the two places where the claim maps enter: the
// pixel's own mark gates `final`, and an emitting pixel marks the source pixel nearest to each consistent reprojection.
// Dynamic = true replaces `geo`: a source's first passing level (thresholds grow with n, so it passes every level from there on)
// is found by comparison in the source loop and counted in an 8-bit field of hist0 / hist1 (field i: level n_min + i, 16 fields
// for at most ITERMVS_MAX_SRC levels); the running sum of the fields is c_n.  The average, the count and the claims stay those
// of the base decision `ok`.
template <bool Claim, bool Dynamic>
__device__ __forceinline__ void fuse_pixel(const FuseArgs& a, const uint8_t* __restrict__ claimed_ref,
                                           uint8_t* const* claimed_src, const FuseDynArgs* dyn) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.W || y >= a.H) return;
    const int p = y * a.W + x;
    const float dref = a.depth_ref[p];
    const double d = (double)dref;
    const double px = (double)x * d, py = (double)y * d;
    int geo = 0;
    uint32_t ok_bits = 0;
    float acc = 0.0f;
    uint64_t hist0 = 0, hist1 = 0;
    const int n_top = Dynamic ? (dyn->n_max < a.S ? dyn->n_max : a.S) : 0;                  // min(n_max, S)
    for (int s = 0; s < a.S; ++s) {
        const float* __restrict__ m = a.mats + s * 60;
        double xs, ys;
        project_to_source(m, px, py, d, xs, ys);
        const float xs32 = (float)xs, ys32 = (float)ys;
        const double smp = (double)remap_bilinear(a.depth_src[s], a.H, a.W, xs32, ys32);   // eval.py:176
        double qx, qy, qz, wx, wy, wz, jx, jy, jz;
        mat3(m + 30, xs * smp, ys * smp, smp, qx, qy, qz);  // back to source 3-D space (eval.py:181-182)
        mat34(m + 39, qx, qy, qz, wx, wy, wz);             // reference 3-D space      (eval.py:184-185)
        const float drep = (float)wz;
        mat3(m + 51, wx, wy, wz, jx, jy, jz);
        const float xr = (float)(jx / (jz + 1e-6)), yr = (float)(jy / (jz + 1e-6));        // eval.py:189
        const double ddx = (double)xr - (double)x, ddy = (double)yr - (double)y;
        const double dist = sqrt(ddx * ddx + ddy * ddy);                                    // eval.py:203
        const float rel = fabsf(drep - dref) / dref;                                        // eval.py:205-206
        const bool ok = dist < a.geo_pixel_thres && rel < a.geo_depth_thres;
        geo += ok ? 1 : 0;
        if (Claim) ok_bits |= (ok ? 1u : 0u) << s;
        acc = acc + (ok ? drep : 0.0f);                                                     // eval.py:209,262
        if (Dynamic) {
            for (int n = dyn->n_min; n <= n_top; ++n) {
                if (dist < (double)n * dyn->pixel_step && rel < (float)n * dyn->depth_step) {   // NaN fails every level
                    const int i = n - dyn->n_min;
                    if (i < 8) hist0 += 1ull << (8 * i); else hist1 += 1ull << (8 * (i - 8));
                    break;
                }
            }
        }
    }
    int level = 0;
    if (Dynamic) {
        int c = 0;
        for (int n = dyn->n_min; n <= n_top; ++n) {
            const int i = n - dyn->n_min;
            c += (int)((i < 8 ? hist0 >> (8 * i) : hist1 >> (8 * (i - 8))) & 0xffu);
            if (c >= n) { level = n; break; }
        }
    }
    const float total = acc + dref;
    a.depth_avg[p] = (double)total / (double)(geo + 1);                                    // eval.py:264
    const bool photo = a.conf_ref[p] > a.photo_thres, g = Dynamic ? level != 0 : geo >= a.geo_mask_thres;
    bool final = photo && g;
    if (Claim) final = final && !(claimed_ref && claimed_ref[p] != 0);
    if (a.photo_mask) a.photo_mask[p] = photo;
    if (a.geo_mask) a.geo_mask[p] = g;
    if (a.final_mask) a.final_mask[p] = final;
    if (a.geo_sum) a.geo_sum[p] = geo;
    if (Dynamic && dyn->geo_level) dyn->geo_level[p] = (uint8_t)level;
    if (!Claim || !final || !claimed_src[0]) return;
    // The claim step, for the few pixels that emit: the projection and the sample of each consistent source are computed again
    // by the expressions above (same operations, same bits) instead of being held in registers for all S sources.
    const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);
    for (int s = 0; s < a.S; ++s) {
        if (!((ok_bits >> s) & 1u)) continue;
        double xs, ys;
        project_to_source(a.mats + s * 60, px, py, d, xs, ys);
        const float xs32 = (float)xs, ys32 = (float)ys;
        const float smp32 = remap_bilinear(a.depth_src[s], a.H, a.W, xs32, ys32);
        const float qx = rintf(xs32), qy = rintf(ys32);
        if (!(qx >= 0.0f && qx <= wmax && qy >= 0.0f && qy <= hmax)) continue;             // NaN and inf fail: q is inside [H,W]
        const size_t q = (size_t)(int)qy * (size_t)a.W + (size_t)(int)qx;
        if (fabsf(a.depth_src[s][q] - smp32) / smp32 < a.geo_depth_thres) claimed_src[s][q] = 1;   // not across a depth edge
    }
}

__global__ void __launch_bounds__(256) fuse_depth_kernel(const FuseArgs a) {
    fuse_pixel<false, false>(a, nullptr, nullptr, nullptr);
}

// Reads claimed_ref, writes claimed_src[s] (never the same map: checked on the host) with plain byte stores of the constant 1:
// whichever threads reach a byte, in whatever order, it ends as 1, so the maps do not depend on scheduling and need no atomics.
__global__ void __launch_bounds__(256) fuse_depth_claim_kernel(const FuseClaimArgs c) {
    fuse_pixel<true, false>(c.f, c.claimed_ref, c.claimed_src, nullptr);
}

// claimed_ref and claimed_src[0] null: the no-dedupe form (nothing gates `final`, the claim step is skipped)
__global__ void __launch_bounds__(256) fuse_depth_dynamic_kernel(const FuseClaimArgs c, const FuseDynArgs d) {
    fuse_pixel<true, true>(c.f, c.claimed_ref, c.claimed_src, &d);
}

}  // namespace itermvs

using namespace itermvs;

// the checks and the argument block both entry points share
static int fill_fuse_args(FuseArgs& a, const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                          const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres, float geo_depth_thres,
                          float photo_thres, int32_t geo_mask_thres, double* depth_avg, uint8_t* photo_mask, uint8_t* geo_mask,
                          uint8_t* final_mask, int32_t* geo_sum) {
    ITERMVS_RETURN_IF(!depth_ref || !conf_ref || !depth_src || !mats || !depth_avg, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(H < 1 || W < 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(S < 1 || S > ITERMVS_MAX_SRC, ITERMVS_ERR_VIEWS);
    a.depth_ref = depth_ref; a.conf_ref = conf_ref; a.mats = mats;
    for (int s = 0; s < ITERMVS_MAX_SRC; ++s) {
        a.depth_src[s] = s < S ? depth_src[s] : nullptr;
        ITERMVS_RETURN_IF(s < S && !depth_src[s], ITERMVS_ERR_NULL);
    }
    a.depth_avg = depth_avg; a.photo_mask = photo_mask; a.geo_mask = geo_mask; a.final_mask = final_mask;
    a.geo_sum = geo_sum;
    a.S = S; a.H = H; a.W = W; a.geo_mask_thres = geo_mask_thres;
    a.geo_pixel_thres = geo_pixel_thres; a.geo_depth_thres = geo_depth_thres; a.photo_thres = photo_thres;
    return ITERMVS_OK;
}

// the claim maps of both entry points that take them, behind fill_fuse_args
static int fill_claim_args(FuseClaimArgs& c, const uint8_t* claimed_ref, uint8_t* const* claimed_src, int32_t S) {
    c.claimed_ref = claimed_ref;
    for (int s = 0; s < ITERMVS_MAX_SRC; ++s) {
        c.claimed_src[s] = claimed_src && s < S ? claimed_src[s] : nullptr;
        ITERMVS_RETURN_IF(claimed_src && s < S && !claimed_src[s], ITERMVS_ERR_NULL);
        // a map that is read as claimed_ref and written as claimed_src in one launch would race with itself
        ITERMVS_RETURN_IF(claimed_src && s < S && claimed_src[s] == claimed_ref, ITERMVS_ERR_DIMS);
    }
    return ITERMVS_OK;
}

extern "C" int itermvs_fuse_depth(const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                                  const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres,
                                  float geo_depth_thres, float photo_thres, int32_t geo_mask_thres, double* depth_avg,
                                  uint8_t* photo_mask, uint8_t* geo_mask, uint8_t* final_mask, int32_t* geo_sum,
                                  void* stream) {
    FuseArgs a;
    const int status = fill_fuse_args(a, depth_ref, conf_ref, depth_src, mats, S, H, W, geo_pixel_thres, geo_depth_thres,
                                      photo_thres, geo_mask_thres, depth_avg, photo_mask, geo_mask, final_mask, geo_sum);
    if (status != ITERMVS_OK) return status;
    hipLaunchKernelGGL(fuse_depth_kernel, dim3((W + 31) / 32, (H + 7) / 8), dim3(256), 0, (hipStream_t)stream, a);
    return itermvs_launch_status();
}

extern "C" int itermvs_fuse_depth_claim(const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                                        const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres,
                                        float geo_depth_thres, float photo_thres, int32_t geo_mask_thres, double* depth_avg,
                                        uint8_t* photo_mask, uint8_t* geo_mask, uint8_t* final_mask, int32_t* geo_sum,
                                        const uint8_t* claimed_ref, uint8_t* const* claimed_src, void* stream) {
    FuseClaimArgs c;
    const int status = fill_fuse_args(c.f, depth_ref, conf_ref, depth_src, mats, S, H, W, geo_pixel_thres, geo_depth_thres,
                                      photo_thres, geo_mask_thres, depth_avg, photo_mask, geo_mask, final_mask, geo_sum);
    if (status != ITERMVS_OK) return status;
    const int claim_status = fill_claim_args(c, claimed_ref, claimed_src, S);
    if (claim_status != ITERMVS_OK) return claim_status;
    hipLaunchKernelGGL(fuse_depth_claim_kernel, dim3((W + 31) / 32, (H + 7) / 8), dim3(256), 0, (hipStream_t)stream, c);
    return itermvs_launch_status();
}

extern "C" int itermvs_fuse_depth_dynamic(const float* depth_ref, const float* conf_ref, const float* const* depth_src,
                                          const float* mats, int32_t S, int32_t H, int32_t W, double geo_pixel_thres,
                                          float geo_depth_thres, float photo_thres, double* depth_avg, uint8_t* photo_mask,
                                          uint8_t* geo_mask, uint8_t* final_mask, int32_t* geo_sum, const uint8_t* claimed_ref,
                                          uint8_t* const* claimed_src, double dyn_pixel_step, float dyn_depth_step,
                                          int32_t n_min, int32_t n_max, uint8_t* geo_level, void* stream) {
    FuseClaimArgs c;
    const int status = fill_fuse_args(c.f, depth_ref, conf_ref, depth_src, mats, S, H, W, geo_pixel_thres, geo_depth_thres,
                                      photo_thres, 0, depth_avg, photo_mask, geo_mask, final_mask, geo_sum);
    if (status != ITERMVS_OK) return status;
    const int claim_status = fill_claim_args(c, claimed_ref, claimed_src, S);
    if (claim_status != ITERMVS_OK) return claim_status;
    ITERMVS_RETURN_IF(!(isfinite(dyn_pixel_step) && dyn_pixel_step > 0.0 && isfinite(dyn_depth_step) && dyn_depth_step > 0.0f),
                      ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(n_min < 1 || n_min > n_max || n_max > ITERMVS_MAX_SRC, ITERMVS_ERR_DIMS);
    FuseDynArgs d;
    d.pixel_step = dyn_pixel_step; d.depth_step = dyn_depth_step; d.n_min = n_min; d.n_max = n_max; d.geo_level = geo_level;
    hipLaunchKernelGGL(fuse_depth_dynamic_kernel, dim3((W + 31) / 32, (H + 7) / 8), dim3(256), 0, (hipStream_t)stream, c, d);
    return itermvs_launch_status();
}
