// The point-cloud passes of the Tanks and Temples evaluation (host side: itermvs_amd/cloud_register.py): the crop to a scene's
// polygon prism, the per-voxel mean, the nearest-neighbour index of transformed queries and the sums of the similarity fit.
// They stand in for Open3D's SelectionPolygonVolume.crop_point_cloud, voxel_down_sample, the correspondence search of
// registration_icp and TransformationEstimationPointToPoint(with_scaling = true), which the official scoring script calls.
//
// All arithmetic is fp64 on float32 coordinates, written operation for operation and built without contraction, so a numpy
// restatement gives the same bits.  A transform T (4x4 row-major, rows 0..2 used) is applied as ((m0*x + m1*y) + m2*z) + m3.
// No float atomics anywhere: every sum has one fixed order, so two runs give the same bytes.  No value read from memory is used
// as an address without a bounds check: idx[] entries are compared against [0, nt), ranks against [0, n_out), and the
// positions of the grid search come from the binary search of cloud_grid.hpp.
//
// cloud_crop_kernel: the polygon (at most 1024 (u, v) pairs) is staged in LDS once per workgroup; every lane reads the same
// vertex at the same time (an LDS broadcast).  Edge (a, b) toggles iff (a_v > c_v) != (b_v > c_v) and
// c_u < (((b_u - a_u) * (c_v - a_v)) / (b_v - a_v)) + a_u; b is the vertex after a, the last edge closes the polygon.
//
// cloud_voxel_mean_kernel: one lane per point of the key-sorted cloud.  A lane whose key differs from its predecessor's is a
// segment head; it finds the end of its run with one binary search.  Runs of at most kLongRun points are summed by the head
// lane itself.  Longer runs are handed to the whole wave: 64 points are loaded at once (coalesced) and added one after the
// other in lane order from broadcasts, so the order of the additions -- and with it every bit -- is the sequential one,
// whatever the run length; what the wave saves is the chain of dependent global loads of a single lane.
//
// cloud_umeyama_partial_kernel / cloud_umeyama_final_kernel: workgroup g owns the contiguous slice [g * slice, (g + 1) * slice);
// thread t adds the elements t, t + 256, ... of the slice in that order, the 64 lanes of a wave combine by xor-butterfly
// (offsets 32, 16, ..., 1: every lane ends with the same bits), the 4 waves are added in wave order, and a single workgroup adds
// the partials in ascending g.  umeyama_groups(n) below is the grid size.
#include "cloud_grid.hpp"
#include "wave_ops.hpp"

namespace itermvs {

constexpr int kMaxPoly = 1024;
constexpr int kPolyChunk = 128;                            // vertices per upload launch: 2 KiB of kernel arguments
constexpr int kLongRun = 64;                               // voxel runs longer than this are summed by the whole wave
constexpr int kSumsPerGroup = 2048;                        // correspondences per workgroup before a second workgroup is used
constexpr int kMaxSumGroups = 1024;
constexpr int kSums = 18;

struct Transform {
    double m[12];                                          // rows 0..2 of the 4x4
};

struct PolyChunk {
    double uv[kPolyChunk][2];
};

__device__ __forceinline__ void apply(const Transform& T, const float* __restrict__ p, double& x, double& y, double& z) {
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    x = ((T.m[0] * px + T.m[1] * py) + T.m[2] * pz) + T.m[3];
    y = ((T.m[4] * px + T.m[5] * py) + T.m[6] * pz) + T.m[7];
    z = ((T.m[8] * px + T.m[9] * py) + T.m[10] * pz) + T.m[11];
}

// kernel arguments are the transport of the host polygon: no copy from host memory that could outlive the caller's buffer
__global__ void __launch_bounds__(kPolyChunk) cloud_poly_upload_kernel(PolyChunk c, int first, int count, double* __restrict__ poly) {
    const int k = threadIdx.x;
    if (k >= count) return;
    poly[(first + k) * 2 + 0] = c.uv[k][0];
    poly[(first + k) * 2 + 1] = c.uv[k][1];
}

__global__ void __launch_bounds__(kCloudBlock) cloud_crop_kernel(const float* __restrict__ xyz, long long n, Transform T, int w,
                                                                 int u, int v, double axis_min, double axis_max,
                                                                 const double* __restrict__ poly, int n_poly,
                                                                 uint8_t* __restrict__ out) {
    __shared__ double s_poly[kMaxPoly * 2];
    for (int k = threadIdx.x; k < n_poly * 2; k += kCloudBlock) s_poly[k] = poly[k];
    __syncthreads();
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (i >= n) return;
    double c[3];
    apply(T, xyz + i * 3, c[0], c[1], c[2]);
    const double cu = u == 0 ? c[0] : c[1], cv = v == 1 ? c[1] : c[2], cw = w == 0 ? c[0] : (w == 1 ? c[1] : c[2]);
    uint8_t in = 0;
    if (isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && cw >= axis_min && cw <= axis_max) {
        bool inside = false;
        for (int k = 0; k < n_poly; ++k) {
            const int k1 = k + 1 < n_poly ? k + 1 : 0;
            const double au = s_poly[k * 2], av = s_poly[k * 2 + 1], bu = s_poly[k1 * 2], bv = s_poly[k1 * 2 + 1];
            if ((av > cv) != (bv > cv) && cu < (((bu - au) * (cv - av)) / (bv - av)) + au) inside = !inside;
        }
        in = inside ? 1 : 0;
    }
    out[i] = in;
}

__global__ void __launch_bounds__(kCloudBlock) cloud_voxel_heads_kernel(const long long* __restrict__ keys, long long n,
                                                                        int* __restrict__ head) {
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (i >= n) return;
    const long long key = keys[i];
    head[i] = key != kNoKey && (i == 0 || keys[i - 1] != key) ? 1 : 0;
}

__device__ __forceinline__ double lane_value(double x, int lane) {
    return __shfl(x, lane, 64);
}

// rank[i] = (inclusive count of heads up to i) - 1: the segment's position in the output
__global__ void __launch_bounds__(kCloudBlock) cloud_voxel_mean_kernel(const float* __restrict__ xyz,
                                                                       const long long* __restrict__ keys,
                                                                       const long long* __restrict__ rank, long long n,
                                                                       long long n_out, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    long long len = 0, slot = -1;
    if (i < n) {
        const long long key = keys[i];
        if (key != kNoKey && (i == 0 || keys[i - 1] != key)) {
            const long long r = rank[i];
            if (r >= 0 && r < n_out) {                     // a rank outside the output writes nothing
                slot = r;
                len = lower_bound(keys, n, key + 1) - i;   // key < kNoKey, so key + 1 does not overflow; the run ends inside [i + 1, n]
            }
        }
    }
    if (slot >= 0 && len <= kLongRun) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (long long j = i; j < i + len; ++j) {
            sx += (double)xyz[j * 3 + 0];
            sy += (double)xyz[j * 3 + 1];
            sz += (double)xyz[j * 3 + 2];
        }
        const double cnt = (double)len;
        out[slot * 3 + 0] = (float)(sx / cnt);
        out[slot * 3 + 1] = (float)(sy / cnt);
        out[slot * 3 + 2] = (float)(sz / cnt);
    }
    // a run of more than 64 points puts the next head at least 65 positions later, so a wave holds at most one long-run head;
    // every lane of the wave takes part in its sum (none has returned)
    const unsigned long long todo = __ballot(slot >= 0 && len > kLongRun);
    if (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        const long long first = __shfl(i, owner, 64), count = __shfl(len, owner, 64);
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (long long base = 0; base < count; base += 64) {
            const long long j = first + base + lane;
            const bool have = base + lane < count;         // first + count <= n by the binary search
            const double x = have ? (double)xyz[j * 3 + 0] : 0.0, y = have ? (double)xyz[j * 3 + 1] : 0.0,
                         z = have ? (double)xyz[j * 3 + 2] : 0.0;
            const int m = count - base < 64 ? (int)(count - base) : 64;
            for (int k = 0; k < m; ++k) {                  // wave-uniform trip count; every lane keeps the same sums
                sx += lane_value(x, k);
                sy += lane_value(y, k);
                sz += lane_value(z, k);
            }
        }
        if (lane == owner) {
            const double cnt = (double)len;
            out[slot * 3 + 0] = (float)(sx / cnt);
            out[slot * 3 + 1] = (float)(sy / cnt);
            out[slot * 3 + 2] = (float)(sz / cnt);
        }
    }
}

// the best of a search that keeps the target: ties on d2 go to the lowest original index
struct NearestIndex {
    double d2;
    long long idx;
    const long long* perm;
    __device__ __forceinline__ NearestIndex take(long long j, double c) const {
        if (!(c <= d2)) return *this;                      // NaN never wins
        const long long o = perm[j];
        return (c < d2 || o < idx) ? NearestIndex{c, o, perm} : *this;
    }
};

__global__ void __launch_bounds__(kCloudBlock) cloud_nn_index_kernel(const float* __restrict__ q, long long nq, Transform T,
                                                                     const float* __restrict__ t,
                                                                     const long long* __restrict__ keys,
                                                                     const long long* __restrict__ perm, long long nt,
                                                                     CloudGrid g, double max_dist, double max_d2, int rings,
                                                                     long long* __restrict__ idx, double* __restrict__ d2) {
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (i >= nq) return;
    double qx, qy, qz;
    apply(T, q + i * 3, qx, qy, qz);
    NearestIndex best{INFINITY, 0x7fffffffffffffffLL, perm};
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
        const int cx = clamped_cell(qx, g.ox, g.edge), cy = clamped_cell(qy, g.oy, g.edge), cz = clamped_cell(qz, g.oz, g.edge);
        ring_walk(t, keys, nt, g, cx, cy, cz, qx, qy, qz, max_dist, rings, best);
    }
    const bool hit = best.d2 < max_d2;                     // exclusive: a target exactly max_dist away is no match
    idx[i] = hit ? best.idx : -1;
    d2[i] = hit ? best.d2 : INFINITY;
}

__global__ void __launch_bounds__(kCloudBlock) cloud_umeyama_partial_kernel(const float* __restrict__ q, long long n, Transform T,
                                                                            const long long* __restrict__ idx,
                                                                            const double* __restrict__ d2,
                                                                            const float* __restrict__ target, long long nt,
                                                                            long long slice, double* __restrict__ partials) {
    __shared__ double s_part[kCloudBlock / 64][kSums];
    const long long lo = (long long)blockIdx.x * slice, hi = lo + slice < n ? lo + slice : n;
    double s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += kCloudBlock) {
        const long long j = idx[i];
        if (j < 0 || j >= nt) continue;                    // unmatched, or not an index into the targets
        double p[3];
        apply(T, q + i * 3, p[0], p[1], p[2]);
        const double t[3] = {(double)target[j * 3 + 0], (double)target[j * 3 + 1], (double)target[j * 3 + 2]};
        s[0] += 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[1 + a] += p[a];
            s[4 + a] += t[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s[7 + a * 3 + b] += t[a] * p[b];
        }
        s[16] += ((p[0] * p[0]) + (p[1] * p[1])) + (p[2] * p[2]);
        s[17] += d2[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const double w = wave_sum_all(s[k]);
        if (lane == 0) s_part[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        double a = s_part[0][threadIdx.x];
        for (int w = 1; w < kCloudBlock / 64; ++w) a += s_part[w][threadIdx.x];
        partials[(long long)blockIdx.x * kSums + threadIdx.x] = a;
    }
}

__global__ void __launch_bounds__(64) cloud_umeyama_final_kernel(const double* __restrict__ partials, int groups,
                                                                 double* __restrict__ sums) {
    if (threadIdx.x >= kSums) return;
    double a = 0.0;
    for (int g = 0; g < groups; ++g) a += partials[(long long)g * kSums + threadIdx.x];
    sums[threadIdx.x] = a;
}

static inline int umeyama_groups(long long n) {
    const long long g = (n + kSumsPerGroup - 1) / kSumsPerGroup;
    return (int)(g < 1 ? 1 : (g > kMaxSumGroups ? kMaxSumGroups : g));
}

// rows 0..2 of a finite host 4x4; false when an entry is not finite
static inline bool read_transform(const double* T, Transform& out) {
    for (int k = 0; k < 12; ++k) {
        if (!isfinite(T[k])) return false;
        out.m[k] = T[k];
    }
    return true;
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_cloud_crop(const float* xyz, int64_t n, const double* T, int32_t axis, double axis_min, double axis_max,
                                  const double* polygon, int32_t n_poly, double* poly_ws, uint8_t* out, void* stream) {
    ITERMVS_RETURN_IF(!xyz || !T || !polygon || !poly_ws || !out, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints || axis < 0 || axis > 2 || n_poly < 3 || n_poly > kMaxPoly, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(isnan(axis_min) || isnan(axis_max), ITERMVS_ERR_DIMS);
    Transform tr;
    ITERMVS_RETURN_IF(!read_transform(T, tr), ITERMVS_ERR_DIMS);
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    for (int k = 0; k < n_poly; ++k)
        ITERMVS_RETURN_IF(!isfinite(polygon[k * 3 + u]) || !isfinite(polygon[k * 3 + v]), ITERMVS_ERR_DIMS);
    for (int first = 0; first < n_poly; first += kPolyChunk) {
        PolyChunk c;
        const int count = n_poly - first < kPolyChunk ? n_poly - first : kPolyChunk;
        for (int k = 0; k < kPolyChunk; ++k) {
            c.uv[k][0] = k < count ? polygon[(first + k) * 3 + u] : 0.0;
            c.uv[k][1] = k < count ? polygon[(first + k) * 3 + v] : 0.0;
        }
        hipLaunchKernelGGL(cloud_poly_upload_kernel, dim3(1), dim3(kPolyChunk), 0, (hipStream_t)stream, c, first, count, poly_ws);
    }
    return flat_launch<cloud_crop_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, xyz, (long long)n, tr, (int)axis, u, v,
        axis_min, axis_max, (const double*)poly_ws, (int)n_poly, out);
}

extern "C" int itermvs_cloud_voxel_heads(const int64_t* keys_sorted, int64_t n, int32_t* head, void* stream) {
    ITERMVS_RETURN_IF(!keys_sorted || !head, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints, ITERMVS_ERR_DIMS);
    return flat_launch<cloud_voxel_heads_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, (const long long*)keys_sorted,
        (long long)n, (int*)head);
}

extern "C" int itermvs_cloud_voxel_mean(const float* xyz_sorted, const int64_t* keys_sorted, const int64_t* rank, int64_t n,
                                        int64_t n_out, float* out, void* stream) {
    ITERMVS_RETURN_IF(!xyz_sorted || !keys_sorted || !rank || !out, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints || n_out < 1 || n_out > n, ITERMVS_ERR_DIMS);
    return flat_launch<cloud_voxel_mean_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, xyz_sorted, (const long long*)keys_sorted,
        (const long long*)rank, (long long)n, (long long)n_out, out);
}

extern "C" int itermvs_cloud_nn_index(const float* q, int64_t nq, const double* T, const float* to_sorted,
                                      const int64_t* keys_sorted, const int64_t* perm, int64_t nt, double ox, double oy, double oz,
                                      int32_t nx, int32_t ny, int32_t nz, double edge, double max_dist, int32_t rings,
                                      int64_t* idx, double* d2, void* stream) {
    ITERMVS_RETURN_IF(!q || !T || !idx || !d2 || (nt > 0 && (!to_sorted || !keys_sorted || !perm)), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(nq < 1 || nq > kCloudMaxPoints || nt < 0, ITERMVS_ERR_DIMS);
    CloudGrid g;
    const int bad = check_grid(nt > 0 ? nt : 1, ox, oy, oz, nx, ny, nz, edge, &g);
    ITERMVS_RETURN_IF(bad, bad);
    ITERMVS_RETURN_IF(check_walk(max_dist, rings), ITERMVS_ERR_DIMS);
    Transform tr;
    ITERMVS_RETURN_IF(!read_transform(T, tr), ITERMVS_ERR_DIMS);
    return flat_launch<cloud_nn_index_kernel, kCloudBlock>({nq, kCloudMaxPoints}, (hipStream_t)stream, q, (long long)nq, tr, to_sorted,
        (const long long*)keys_sorted, (const long long*)perm, (long long)nt, g, max_dist, max_dist * max_dist, (int)rings, (long long*)idx, d2);
}

extern "C" int itermvs_cloud_umeyama_groups(int64_t n) {
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints, ITERMVS_ERR_DIMS);
    return umeyama_groups(n);
}

extern "C" int itermvs_cloud_umeyama_sums(const float* q, int64_t n, const double* T, const int64_t* idx, const double* d2,
                                          const float* target, int64_t nt, double* partials, double* sums, void* stream) {
    ITERMVS_RETURN_IF(!q || !T || !idx || !d2 || !partials || !sums || (nt > 0 && !target), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints || nt < 0 || nt > kCloudMaxPoints, ITERMVS_ERR_DIMS);
    Transform tr;
    ITERMVS_RETURN_IF(!read_transform(T, tr), ITERMVS_ERR_DIMS);
    const int groups = umeyama_groups(n);
    const long long slice = (n + groups - 1) / groups;
    hipLaunchKernelGGL(cloud_umeyama_partial_kernel, dim3(groups), dim3(kCloudBlock), 0, (hipStream_t)stream, q, (long long)n, tr,
                       (const long long*)idx, d2, target, (long long)nt, slice, partials);
    hipLaunchKernelGGL(cloud_umeyama_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, groups, sums);
    return itermvs_launch_status();
}
