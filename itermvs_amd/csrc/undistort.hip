// itermvs_undistort_rgb8: an image of a COLMAP camera with lens distortion resampled to a pinhole camera -- the warp of COLMAP's
// image_undistorter, which colmap_input.py leaves to the user.  The arithmetic, operation by operation, is in
// include/itermvs_hip.h; itermvs_amd/undistort.py chooses the output camera.
//
// A gather: per output pixel a few dozen fp64 operations (one atan for the fisheye models), four taps of three bytes, three
// bytes out.  Neighbouring lanes read neighbouring source pixels, so the byte loads of a wave fall into a handful of cache lines
// per tap row; nothing is staged.  Four neighbouring pixels per thread make the store 12 contiguous bytes (three dwords) when
// the width allows it, as in resize_rgb8.hip; otherwise one pixel per thread with byte stores.  The model is a launch-uniform
// switch: every lane of a launch takes the same case.
//
// Safety: the integer tap indices are formed only after `sx >= 0 && sx <= Ws - 1 && sy >= 0 && sy <= Hs - 1` held, which NaN
// and +-Inf fail, so no parameter set makes the kernel read outside src.
#include "flat_launch.hpp"

namespace itermvs {

constexpr int kUndistortBlock = 256;
constexpr int kUndistortMaxParams = 12;

enum : int {
    kSimplePinhole = 0, kPinhole = 1, kSimpleRadial = 2, kRadial = 3, kOpenCV = 4, kOpenCVFisheye = 5, kFullOpenCV = 6, kFov = 7,
    kSimpleRadialFisheye = 8, kRadialFisheye = 9, kThinPrismFisheye = 10
};

// number of parameters of a supported model, -1 otherwise (COLMAP src/colmap/sensor/models.h)
static int undistort_param_count(int model) {
    switch (model) {
        case kSimplePinhole: return 3;
        case kPinhole: return 4;
        case kSimpleRadial: return 4;
        case kRadial: return 5;
        case kOpenCV: return 8;
        case kOpenCVFisheye: return 8;
        case kFullOpenCV: return 12;
        case kSimpleRadialFisheye: return 4;
        case kRadialFisheye: return 5;
        default: return -1;
    }
}

struct UndistortArgs {
    const uint8_t* src;
    uint8_t* out;
    double* map;                       // [Ho,Wo,2] or nullptr
    double fx, fy, cx, cy;             // the distorted camera
    double k[8];                       // its distortion parameters, in COLMAP's order
    double fxo, fyo, cxo, cyo;         // the output pinhole
    int model, Hs, Ws, Ho, Wo;
};

// (u, v) -> (du, dv); the written order of operations is the contract (include/itermvs_hip.h)
__device__ __forceinline__ void undistort_distortion(int model, const double* __restrict__ k, double u, double v, double& du,
                                                     double& dv) {
    const double u2 = u * u, v2 = v * v, r2 = u2 + v2;
    du = 0.0;
    dv = 0.0;
    switch (model) {
        case kSimpleRadial: {
            const double radial = k[0] * r2;
            du = u * radial;
            dv = v * radial;
        } break;
        case kRadial: {
            const double r4 = r2 * r2, radial = k[0] * r2 + k[1] * r4;
            du = u * radial;
            dv = v * radial;
        } break;
        case kOpenCV: {
            const double r4 = r2 * r2, uv = u * v, radial = k[0] * r2 + k[1] * r4;
            du = (u * radial + (2.0 * k[2]) * uv) + k[3] * (r2 + 2.0 * u2);
            dv = (v * radial + (2.0 * k[3]) * uv) + k[2] * (r2 + 2.0 * v2);
        } break;
        case kFullOpenCV: {
            const double r4 = r2 * r2, r6 = r4 * r2, uv = u * v;
            const double radial = (((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6) / (((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6);
            du = ((u * radial + (2.0 * k[2]) * uv) + k[3] * (r2 + 2.0 * u2)) - u;
            dv = ((v * radial + (2.0 * k[3]) * uv) + k[2] * (r2 + 2.0 * v2)) - v;
        } break;
        case kSimpleRadialFisheye:
        case kRadialFisheye:
        case kOpenCVFisheye: {
            const double r = sqrt(r2);
            if (r > 2.220446049250313e-16) {
                const double t = atan(r), t2 = t * t;
                double poly = 1.0 + k[0] * t2;
                if (model != kSimpleRadialFisheye) {
                    const double t4 = t2 * t2;
                    poly = poly + k[1] * t4;
                    if (model == kOpenCVFisheye) {
                        const double t6 = t4 * t2, t8 = t4 * t4;
                        poly = (poly + k[2] * t6) + k[3] * t8;
                    }
                }
                const double td = t * poly;
                du = (u * td) / r - u;
                dv = (v * td) / r - v;
            }
        } break;
        default: break;                                   // the pinhole models
    }
}

__device__ __forceinline__ int undistort_round8(double value) {
    const double f = floor(value + 0.5);
    return f < 0.0 ? 0 : (f > 255.0 ? 255 : (int)f);
}

// one output pixel -> its three bytes (0 when not filled) and its source coordinates
__device__ __forceinline__ void undistort_pixel(const UndistortArgs& a, int x, int y, int rgb[3], double& sx, double& sy) {
    const double u = (((double)x + 0.5) - a.cxo) / a.fxo, v = (((double)y + 0.5) - a.cyo) / a.fyo;
    double du, dv;
    undistort_distortion(a.model, a.k, u, v, du, dv);
    sx = (a.fx * (u + du) + a.cx) - 0.5;
    sy = (a.fy * (v + dv) + a.cy) - 0.5;
    rgb[0] = rgb[1] = rgb[2] = 0;
    if (!(sx >= 0.0 && sx <= (double)(a.Ws - 1) && sy >= 0.0 && sy <= (double)(a.Hs - 1))) return;   // NaN, +-Inf: not filled
    const double fx0 = floor(sx), fy0 = floor(sy);
    const int x0 = (int)fx0, y0 = (int)fy0;               // in [0, Ws - 1] x [0, Hs - 1] by the test above
    const int x1 = min(x0 + 1, a.Ws - 1), y1 = min(y0 + 1, a.Hs - 1);
    const double wx = sx - fx0, wy = sy - fy0;
    const uint8_t* r0 = a.src + (int64_t)y0 * a.Ws * 3;
    const uint8_t* r1 = a.src + (int64_t)y1 * a.Ws * 3;
    const uint8_t *p00 = r0 + (int64_t)x0 * 3, *p01 = r0 + (int64_t)x1 * 3, *p10 = r1 + (int64_t)x0 * 3, *p11 = r1 + (int64_t)x1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double top = (1.0 - wx) * (double)p00[c] + wx * (double)p01[c];
        const double bot = (1.0 - wx) * (double)p10[c] + wx * (double)p11[c];
        rgb[c] = undistort_round8((1.0 - wy) * top + wy * bot);
    }
}

// PX output pixels of one row per thread.  PX = 4 needs Wo % 4 == 0 and a 4-byte aligned `out`.
template <int PX>
__global__ void __launch_bounds__(kUndistortBlock) undistort_rgb8_kernel(const UndistortArgs a) {
    const int wq = a.Wo / PX;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)a.Ho * wq) return;
    const int x0 = (int)(t % wq) * PX, y = (int)(t / wq);
    int rgb[PX * 3];
    const int64_t pixel = (int64_t)y * a.Wo + x0;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
        double sx, sy;
        undistort_pixel(a, x0 + p, y, rgb + 3 * p, sx, sy);
        if (a.map) {
            a.map[(pixel + p) * 2 + 0] = sx;
            a.map[(pixel + p) * 2 + 1] = sy;
        }
    }
    uint8_t* o = a.out + pixel * 3;
    if constexpr (PX == 4) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= (uint32_t)rgb[4 * d + j] << (8 * j);
            o4[d] = w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PX * 3; ++i) o[i] = (uint8_t)rgb[i];
    }
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_undistort_rgb8(const uint8_t* src, int32_t Hs, int32_t Ws, int32_t model, const double* params,
                                      int32_t n_params, double fx_o, double fy_o, double cx_o, double cy_o, int32_t Ho, int32_t Wo,
                                      uint8_t* out, double* map, void* stream) {
    ITERMVS_RETURN_IF(!src || !out || !params, ITERMVS_ERR_NULL);
    const int count = undistort_param_count(model);
    ITERMVS_RETURN_IF(count < 0, ITERMVS_ERR_MODEL);
    ITERMVS_RETURN_IF(Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || n_params != count, ITERMVS_ERR_DIMS);
    const bool wide = (Wo % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 4 == 0);
    const FlatItems n{flat_items({Ho, wide ? Wo / 4 : Wo})};
    UndistortArgs a{};
    a.src = src;
    a.out = out;
    a.map = map;
    const bool one_focal = count == 3 || model == kSimpleRadial || model == kRadial || model == kSimpleRadialFisheye ||
                           model == kRadialFisheye;
    const int first = one_focal ? 3 : 4;               // f cx cy | fx fy cx cy, then the distortion parameters
    a.fx = params[0];
    a.fy = one_focal ? params[0] : params[1];
    a.cx = params[first - 2];
    a.cy = params[first - 1];
    static_assert(kUndistortMaxParams - 4 == 8, "k[] holds the parameters after fx fy cx cy of the longest model");
    for (int i = first; i < count; ++i) a.k[i - first] = params[i];
    a.fxo = fx_o;
    a.fyo = fy_o;
    a.cxo = cx_o;
    a.cyo = cy_o;
    a.model = model;
    a.Hs = Hs;
    a.Ws = Ws;
    a.Ho = Ho;
    a.Wo = Wo;
    if (wide) return flat_launch<undistort_rgb8_kernel<4>, kUndistortBlock>(n, (hipStream_t)stream, a);
    return flat_launch<undistort_rgb8_kernel<1>, kUndistortBlock>(n, (hipStream_t)stream, a);
}
