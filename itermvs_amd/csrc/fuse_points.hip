// itermvs_fuse_points: the tail of filter_depth (eval.py:287-308) for one reference view -- the pixels that survive the final
// mask are unprojected to world space, coloured and compacted into the PLY vertex records (x, y, z float32, red, green, blue
// uint8: 15 bytes, not padded) in row-major pixel order behind the vertices of the views emitted before.
// Three launches on the stream, 256 consecutive pixels (flat row-major index) per workgroup:
//   count : per-workgroup population of the final mask (64-bit ballot + popcount) and of the photo / geo masks -> workspace;
//   scan  : ONE workgroup turns the final counts into exclusive offsets in place, reads `cursor` as the view's first vertex
//           index, fills the view's row of view_counts and advances `cursor`;
//   emit  : every workgroup recomputes its lanes' ranks and stores the records whose vertex index is below `capacity`.
// Ordering comes from the stream alone: no workgroup waits on another, no atomics, so the bytes do not depend on scheduling.
// Arithmetic: oracle/fusion_oracle.py:unproject_points -- pixel indices as float64, float32 matrices upcast, k-ascending products
// and sums, each rounded once (cam_math.hpp), one round-to-nearest conversion to float32 at the end.
// itermvs_fuse_points_normals: the same three launches with an emit kernel that writes 27-byte records (x, y, z, nx, ny, nz
// float32, red, green, blue uint8).  Count, scan, the vertex index, the coordinates and the colour are the code of the 15-byte
// path; the normal is the cross product of depth_avg's camera-space differences along the row and the column, turned towards
// the camera and rotated to world space (definition: include/itermvs_hip.h; numpy restatement: tests/fuse_normals_reference.py).
#include <cmath>

#include "cam_math.hpp"
#include "flat_launch.hpp"
#include "wave_ops.hpp"

namespace itermvs {

constexpr int kPtsBlock = 256;                 // pixels per workgroup = 4 waves
constexpr int kPtsWaves = kPtsBlock / 64;
constexpr int kScanBlock = 1024;
constexpr int kRecordBytes = 15;
constexpr int kNormalRecordBytes = 27;         // x y z | nx ny nz | red green blue

// workspace: uint32 [3][nblocks] = final | photo | geo populations per workgroup
__global__ void __launch_bounds__(kPtsBlock) fuse_points_count_kernel(const uint8_t* __restrict__ final_mask,
                                                                      const uint8_t* __restrict__ photo_mask,
                                                                      const uint8_t* __restrict__ geo_mask, uint32_t n,
                                                                      uint32_t* __restrict__ ws) {
    __shared__ uint32_t part[3][kPtsWaves];
    const uint32_t p = blockIdx.x * kPtsBlock + threadIdx.x;
    const bool in = p < n;
    const bool f = in && final_mask[p] != 0;
    const bool ph = in && photo_mask && photo_mask[p] != 0;
    const bool g = in && geo_mask && geo_mask[p] != 0;
    const uint32_t cf = (uint32_t)__popcll(__ballot(f)), cp = (uint32_t)__popcll(__ballot(ph)),
                   cg = (uint32_t)__popcll(__ballot(g));
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        part[0][wv] = cf; part[1][wv] = cp; part[2][wv] = cg;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t s = 0;
        for (int wv = 0; wv < kPtsWaves; ++wv) s += part[threadIdx.x][wv];
        ws[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// one workgroup: ws[0][*] counts -> exclusive offsets (relative to the view's first vertex; < 2^31 by the H*W limit)
__global__ void __launch_bounds__(kScanBlock) fuse_points_scan_kernel(uint32_t* __restrict__ ws, uint32_t nblocks, int has_photo,
                                                                      int has_geo, unsigned long long* __restrict__ cursor,
                                                                      long long* __restrict__ view_row) {
    __shared__ unsigned long long red[2][kScanBlock / 64];
    unsigned long long sp = 0, sg = 0;                     // the photo / geo rows are only summed, beside the scan's own loads
    const uint32_t total = block_scan_exclusive_chunked<uint32_t, kScanBlock>(ws, nblocks, [&](uint32_t i) {
        sp += ws[(size_t)nblocks + i];
        sg += ws[(size_t)2 * nblocks + i];
    });
    sp = wave_sum_lane0(sp);
    sg = wave_sum_lane0(sg);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tp = 0, tg = 0;
        for (int k = 0; k < kScanBlock / 64; ++k) { tp += red[0][k]; tg += red[1][k]; }
        const unsigned long long first = *cursor;
        view_row[0] = has_photo ? (long long)tp : -1;
        view_row[1] = has_geo ? (long long)tg : -1;
        view_row[2] = (long long)total;
        view_row[3] = (long long)first;
        *cursor = first + total;
    }
}

// the vertex index of this lane's pixel: the view's first vertex + the workgroups before it (scan) + the waves and lanes before it
__device__ __forceinline__ unsigned long long pts_vertex_index(bool on, const uint32_t* __restrict__ ws,
                                                               const long long* __restrict__ view_row) {
    uint32_t total;
    const uint32_t own = on ? 1u : 0u, rank = wave_rank(on, total);
    return (unsigned long long)view_row[3] + ws[blockIdx.x] + block_exclusive<kPtsWaves>(rank + own, own);
}

// camera-space point of pixel (x, y) at depth d (eval.py:291-292)
__device__ __forceinline__ void pts_camera(const float* __restrict__ cam, uint32_t x, uint32_t y, double d, double& rx, double& ry,
                                           double& rz) {
    mat3(cam, (double)x * d, (double)y * d, d, rx, ry, rz);
}

// the part of a vertex record that both emit kernels write: world coordinates of the camera-space point (eval.py:293-294)
// -> xyz[0..11], colour of pixel p -> colour[0..2] ((uint8 / 255. * 255).astype(uint8) is the identity)
__device__ __forceinline__ void pts_put_vertex(const float* __restrict__ cam, double rx, double ry, double rz,
                                                 const uint8_t* __restrict__ rgb, uint32_t p, uint8_t* __restrict__ xyz,
                                                 uint8_t* __restrict__ colour) {
    double wx, wy, wz;
    mat34(cam + 9, rx, ry, rz, wx, wy, wz);
    put_f32_bytes(xyz, (float)wx); put_f32_bytes(xyz + 4, (float)wy); put_f32_bytes(xyz + 8, (float)wz);
    const uint8_t* c = rgb + (size_t)p * 3;
    colour[0] = c[0]; colour[1] = c[1]; colour[2] = c[2];
}

__global__ void __launch_bounds__(kPtsBlock) fuse_points_emit_kernel(const double* __restrict__ depth_avg,
                                                                     const uint8_t* __restrict__ final_mask,
                                                                     const float* __restrict__ cam, const uint8_t* __restrict__ rgb,
                                                                     uint32_t n, uint32_t W, const uint32_t* __restrict__ ws,
                                                                     const long long* __restrict__ view_row,
                                                                     uint8_t* __restrict__ records, unsigned long long capacity) {
    const uint32_t p = blockIdx.x * kPtsBlock + threadIdx.x;
    const bool on = p < n && final_mask[p] != 0;
    const unsigned long long idx = pts_vertex_index(on, ws, view_row);
    if (!on || idx >= capacity) return;                    // the ONLY stores below are guarded by idx < capacity
    const uint32_t y = p / W, x = p - y * W;
    double rx, ry, rz;
    pts_camera(cam, x, y, depth_avg[p], rx, ry, rz);
    uint8_t* o = records + idx * kRecordBytes;
    pts_put_vertex(cam, rx, ry, rz, rgb, p, o, o + 12);
}

// the neighbour's depth dq lies on the surface of the pixel at depth d (finite, > 0); a comparison with NaN is false
__device__ __forceinline__ bool pts_same_surface(double dq, double d, double edge_thres) {
    return std::isfinite(dq) && dq > 0.0 && fabs(dq - d) < edge_thres * d;
}

// the tangent along one axis from the camera-space points of the neighbours lo (x-1 | y-1) and hi (x+1 | y+1): hi - lo when both
// are usable, one-sided against the pixel's own point c when one is, false when neither is.  in_lo / in_hi: inside the image; the
// depth of a neighbour outside it is never loaded.
__device__ __forceinline__ bool pts_tangent(const double* __restrict__ depth_avg, const float* __restrict__ cam, bool in_lo,
                                            uint32_t p_lo, uint32_t x_lo, uint32_t y_lo, bool in_hi, uint32_t p_hi, uint32_t x_hi,
                                            uint32_t y_hi, double d, double edge_thres, const double (&c)[3], double (&t)[3]) {
    const double d_lo = in_lo ? depth_avg[p_lo] : 0.0, d_hi = in_hi ? depth_avg[p_hi] : 0.0;      // 0 is never usable
    const bool lo = pts_same_surface(d_lo, d, edge_thres), hi = pts_same_surface(d_hi, d, edge_thres);
    if (!lo && !hi) return false;
    double a[3] = {c[0], c[1], c[2]}, b[3] = {c[0], c[1], c[2]};
    if (hi) pts_camera(cam, x_hi, y_hi, d_hi, a[0], a[1], a[2]);
    if (lo) pts_camera(cam, x_lo, y_lo, d_lo, b[0], b[1], b[2]);
    t[0] = a[0] - b[0]; t[1] = a[1] - b[1]; t[2] = a[2] - b[2];
    return true;
}

// the unit normal of pixel p = (x, y) with depth d and camera-space point c, in world space and facing the reference camera;
// (0, 0, 0) where it is not defined.  p + W < 2^32 by kPtsMaxPixels.
__device__ __forceinline__ void pts_normal(const double* __restrict__ depth_avg, const float* __restrict__ cam, uint32_t p,
                                           uint32_t x, uint32_t y, uint32_t W, uint32_t n, double d, double edge_thres,
                                           const double (&c)[3], float (&out)[3]) {
    out[0] = out[1] = out[2] = 0.0f;
    if (!(std::isfinite(d) && d > 0.0)) return;
    double tx[3], ty[3];
    if (!pts_tangent(depth_avg, cam, x > 0, p - 1, x - 1, y, x + 1 < W, p + 1, x + 1, y, d, edge_thres, c, tx)) return;
    if (!pts_tangent(depth_avg, cam, y > 0, p - W, x, y - 1, p + W < n, p + W, x, y + 1, d, edge_thres, c, ty)) return;
    double nc[3] = {tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]};
    const double s = (nc[0] * c[0] + nc[1] * c[1]) + nc[2] * c[2];
    if (s > 0.0) { nc[0] = -nc[0]; nc[1] = -nc[1]; nc[2] = -nc[2]; }       // towards the camera, the origin of camera space
    double nx, ny, nz;
    rot34(cam + 9, nc[0], nc[1], nc[2], nx, ny, nz);                          // rows 0..2 of inv(E_ref); its 3x3 part rotates
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(std::isfinite(len) && len > 0.0)) return;
    out[0] = (float)(nx / len); out[1] = (float)(ny / len); out[2] = (float)(nz / len);
}

// fuse_points_emit_kernel with the normal between the coordinates and the colour
__global__ void __launch_bounds__(kPtsBlock) fuse_points_normals_emit_kernel(
    const double* __restrict__ depth_avg, const uint8_t* __restrict__ final_mask, const float* __restrict__ cam,
    const uint8_t* __restrict__ rgb, uint32_t n, uint32_t W, double edge_thres, const uint32_t* __restrict__ ws,
    const long long* __restrict__ view_row, uint8_t* __restrict__ records, unsigned long long capacity) {
    const uint32_t p = blockIdx.x * kPtsBlock + threadIdx.x;
    const bool on = p < n && final_mask[p] != 0;
    const unsigned long long idx = pts_vertex_index(on, ws, view_row);
    if (!on || idx >= capacity) return;                    // the ONLY stores below are guarded by idx < capacity
    const uint32_t y = p / W, x = p - y * W;
    const double d = depth_avg[p];
    double c[3];
    pts_camera(cam, x, y, d, c[0], c[1], c[2]);
    float nrm[3];
    pts_normal(depth_avg, cam, p, x, y, W, n, d, edge_thres, c, nrm);
    uint8_t* o = records + idx * kNormalRecordBytes;
    pts_put_vertex(cam, c[0], c[1], c[2], rgb, p, o, o + 24);
    put_f32_bytes(o + 12, nrm[0]); put_f32_bytes(o + 16, nrm[1]); put_f32_bytes(o + 20, nrm[2]);
}

// H*W <= this keeps every 32-bit pixel index, workgroup count and relative offset in range
constexpr long long kPtsMaxPixels = 0x7fffff00LL;

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_fuse_points_workspace_bytes(int32_t H, int32_t W) {
    ITERMVS_RETURN_IF(H < 1 || W < 1 || (long long)H * W > kPtsMaxPixels, ITERMVS_ERR_DIMS);
    const long long nblocks = ((long long)H * W + kPtsBlock - 1) / kPtsBlock;
    return (int)(3 * nblocks * (long long)sizeof(uint32_t));
}

// both entry points: the argument checks, in this order, before anything is launched, then count, scan and the emit kernel of the
// record format -- normals false: 15-byte records, edge_thres not used; true: 27-byte records
static int fuse_points_run(const double* depth_avg, const uint8_t* final_mask, const uint8_t* photo_mask, const uint8_t* geo_mask,
                           const float* cam, const uint8_t* rgb, int32_t H, int32_t W, bool normals, double edge_thres, uint8_t* records,
                           int64_t capacity, uint64_t* cursor, int64_t* view_counts, int32_t view, uint32_t* workspace, void* stream) {
    ITERMVS_RETURN_IF(!depth_avg || !final_mask || !cam || !rgb || !cursor || !view_counts || !workspace, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(!records && capacity != 0, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(H < 1 || W < 1 || (long long)H * W > kPtsMaxPixels || capacity < 0 || view < 0, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(normals && (!std::isfinite(edge_thres) || !(edge_thres > 0.0)), ITERMVS_ERR_DIMS);
    const FlatItems items{(int64_t)H * W, kPtsMaxPixels};
    const uint32_t n = (uint32_t)items.total, nblocks = (n + kPtsBlock - 1) / kPtsBlock;
    hipStream_t s = (hipStream_t)stream;
    long long* row = (long long*)view_counts + (size_t)view * 4;     // the scan fills it, the emit kernel reads it
    const int bad = flat_launch<fuse_points_count_kernel, kPtsBlock>(items, s, final_mask, photo_mask, geo_mask, n, workspace);
    if (bad != ITERMVS_OK) return bad;
    hipLaunchKernelGGL(fuse_points_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, workspace, nblocks, photo_mask ? 1 : 0,
                       geo_mask ? 1 : 0, (unsigned long long*)cursor, row);
    if (!normals)
        return flat_launch<fuse_points_emit_kernel, kPtsBlock>(items, s, depth_avg, final_mask, cam, rgb, n, (uint32_t)W, workspace,
                                                               (const long long*)row, records, (unsigned long long)capacity);
    return flat_launch<fuse_points_normals_emit_kernel, kPtsBlock>(items, s, depth_avg, final_mask, cam, rgb, n, (uint32_t)W,
                                                                   edge_thres, workspace, (const long long*)row, records,
                                                                   (unsigned long long)capacity);
}

extern "C" int itermvs_fuse_points(const double* depth_avg, const uint8_t* final_mask, const uint8_t* photo_mask,
                                   const uint8_t* geo_mask, const float* cam, const uint8_t* rgb, int32_t H, int32_t W,
                                   uint8_t* records, int64_t capacity, uint64_t* cursor, int64_t* view_counts, int32_t view,
                                   uint32_t* workspace, void* stream) {
    return fuse_points_run(depth_avg, final_mask, photo_mask, geo_mask, cam, rgb, H, W, false, 0.0, records, capacity, cursor,
                           view_counts, view, workspace, stream);
}

extern "C" int itermvs_fuse_points_normals(const double* depth_avg, const uint8_t* final_mask, const uint8_t* photo_mask,
                                           const uint8_t* geo_mask, const float* cam, const uint8_t* rgb, int32_t H, int32_t W,
                                           double edge_thres, uint8_t* records, int64_t capacity, uint64_t* cursor,
                                           int64_t* view_counts, int32_t view, uint32_t* workspace, void* stream) {
    return fuse_points_run(depth_avg, final_mask, photo_mask, geo_mask, cam, rgb, H, W, true, edge_thres, records, capacity, cursor,
                           view_counts, view, workspace, stream);
}
