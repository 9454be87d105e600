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
// and sums, each rounded once (-ffp-contract=off), one round-to-nearest conversion to float32 at the end.
#include "common.hpp"

namespace itermvs {

constexpr int kPtsBlock = 256;                 // pixels per workgroup = 4 waves
constexpr int kPtsWaves = kPtsBlock / 64;
constexpr int kScanBlock = 1024;
constexpr int kRecordBytes = 15;

// the same two products as fusion.hip (kept there untouched): (3x3 | rows 0..2 of 4x4, float32 upcast) @ float64 point
__device__ __forceinline__ void pts_mat3(const float* __restrict__ m, double x, double y, double z, double& ox, double& oy,
                                         double& oz) {
    ox = ((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z;
    oy = ((double)m[3] * x + (double)m[4] * y) + (double)m[5] * z;
    oz = ((double)m[6] * x + (double)m[7] * y) + (double)m[8] * z;
}
__device__ __forceinline__ void pts_mat34(const float* __restrict__ m, double x, double y, double z, double& ox, double& oy,
                                          double& oz) {
    ox = (((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z) + (double)m[3] * 1.0;
    oy = (((double)m[4] * x + (double)m[5] * y) + (double)m[6] * z) + (double)m[7] * 1.0;
    oz = (((double)m[8] * x + (double)m[9] * y) + (double)m[10] * z) + (double)m[11] * 1.0;
}

// lanes of this wave below the caller with `on` set, and the wave's total
__device__ __forceinline__ uint32_t wave_rank(bool on, uint32_t& total) {
    const unsigned long long b = __ballot(on);
    total = (uint32_t)__popcll(b);
    const int lane = threadIdx.x & 63;
    return (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
}

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
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    __shared__ unsigned long long red[2][kScanBlock / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t carry = 0;                                    // uniform: vertices of the chunks before this one
    unsigned long long sp = 0, sg = 0;
    for (uint32_t base = 0; base < nblocks; base += kScanBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? ws[i] : 0u;
        if (i < nblocks) {
            sp += ws[(size_t)nblocks + i];
            sg += ws[(size_t)2 * nblocks + i];
        }
        uint32_t inc = v;                                  // inclusive scan inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wv] = inc;
        __syncthreads();
        uint32_t before = 0, chunk = 0;
        for (int k = 0; k < kScanBlock / 64; ++k) {
            const uint32_t s = wave_sum[k];
            before += k < wv ? s : 0u;
            chunk += s;
        }
        if (i < nblocks) ws[i] = carry + before + (inc - v);
        carry += chunk;
        __syncthreads();                                   // wave_sum is rewritten by the next chunk
    }
    for (int d = 32; d > 0; d >>= 1) {
        sp += __shfl_down(sp, d, 64);
        sg += __shfl_down(sg, d, 64);
    }
    if (lane == 0) { red[0][wv] = sp; red[1][wv] = sg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tp = 0, tg = 0;
        for (int k = 0; k < kScanBlock / 64; ++k) { tp += red[0][k]; tg += red[1][k]; }
        const unsigned long long first = *cursor;
        view_row[0] = has_photo ? (long long)tp : -1;
        view_row[1] = has_geo ? (long long)tg : -1;
        view_row[2] = (long long)carry;
        view_row[3] = (long long)first;
        *cursor = first + carry;
    }
}

__global__ void __launch_bounds__(kPtsBlock) fuse_points_emit_kernel(const double* __restrict__ depth_avg,
                                                                     const uint8_t* __restrict__ final_mask,
                                                                     const float* __restrict__ cam, const uint8_t* __restrict__ rgb,
                                                                     uint32_t n, uint32_t W, const uint32_t* __restrict__ ws,
                                                                     const long long* __restrict__ view_row,
                                                                     uint8_t* __restrict__ records, unsigned long long capacity) {
    __shared__ uint32_t part[kPtsWaves];
    const uint32_t p = blockIdx.x * kPtsBlock + threadIdx.x;
    const bool on = p < n && final_mask[p] != 0;
    uint32_t total;
    const uint32_t rank = wave_rank(on, total);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) part[wv] = total;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < kPtsWaves; ++k) before += k < wv ? part[k] : 0u;
    const unsigned long long idx = (unsigned long long)view_row[3] + ws[blockIdx.x] + before + rank;
    if (!on || idx >= capacity) return;                    // the ONLY store below is guarded by idx < capacity
    const uint32_t y = p / W, x = p - y * W;
    const double d = depth_avg[p];
    double rx, ry, rz, wx, wy, wz;
    pts_mat3(cam, (double)x * d, (double)y * d, d, rx, ry, rz);        // eval.py:291-292
    pts_mat34(cam + 9, rx, ry, rz, wx, wy, wz);                        // eval.py:293-294
    const uint32_t bx = __float_as_uint((float)wx), by = __float_as_uint((float)wy), bz = __float_as_uint((float)wz);
    const uint8_t* c = rgb + (size_t)p * 3;                             // (uint8 / 255. * 255).astype(uint8) is the identity
    uint8_t* o = records + idx * kRecordBytes;                          // 15-byte records: no alignment to rely on
    o[0] = (uint8_t)bx; o[1] = (uint8_t)(bx >> 8); o[2] = (uint8_t)(bx >> 16); o[3] = (uint8_t)(bx >> 24);
    o[4] = (uint8_t)by; o[5] = (uint8_t)(by >> 8); o[6] = (uint8_t)(by >> 16); o[7] = (uint8_t)(by >> 24);
    o[8] = (uint8_t)bz; o[9] = (uint8_t)(bz >> 8); o[10] = (uint8_t)(bz >> 16); o[11] = (uint8_t)(bz >> 24);
    o[12] = c[0]; o[13] = c[1]; o[14] = c[2];
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

extern "C" int itermvs_fuse_points(const double* depth_avg, const uint8_t* final_mask, const uint8_t* photo_mask,
                                   const uint8_t* geo_mask, const float* cam, const uint8_t* rgb, int32_t H, int32_t W,
                                   uint8_t* records, int64_t capacity, uint64_t* cursor, int64_t* view_counts, int32_t view,
                                   uint32_t* workspace, void* stream) {
    ITERMVS_RETURN_IF(!depth_avg || !final_mask || !cam || !rgb || !cursor || !view_counts || !workspace, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(!records && capacity != 0, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(H < 1 || W < 1 || (long long)H * W > kPtsMaxPixels || capacity < 0 || view < 0, ITERMVS_ERR_DIMS);
    const uint32_t n = (uint32_t)((long long)H * W);
    const uint32_t nblocks = (n + kPtsBlock - 1) / kPtsBlock;
    long long* row = (long long*)view_counts + (size_t)view * 4;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fuse_points_count_kernel, dim3(nblocks), dim3(kPtsBlock), 0, s, final_mask, photo_mask, geo_mask, n,
                       workspace);
    hipLaunchKernelGGL(fuse_points_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, workspace, nblocks, photo_mask ? 1 : 0,
                       geo_mask ? 1 : 0, (unsigned long long*)cursor, row);
    hipLaunchKernelGGL(fuse_points_emit_kernel, dim3(nblocks), dim3(kPtsBlock), 0, s, depth_avg, final_mask, cam, rgb, n,
                       (uint32_t)W, workspace, (const long long*)row, records, (unsigned long long)capacity);
    return itermvs_launch_status();
}
