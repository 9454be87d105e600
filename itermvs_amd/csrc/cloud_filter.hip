// Outlier removal of a fused cloud (host side: itermvs_amd/cloud_filter.py): the mean distance to the k nearest neighbours
// (Open3D's remove_statistical_outlier, PCL's StatisticalOutlierRemoval) and the neighbour count inside a radius (PCL's
// RadiusOutlierRemoval), both over the sorted uniform grid and the ring walk of cloud_grid.hpp.
//
// The queries are the targets: one lane per position of the key-sorted cloud, so the lanes of a wave share cells and read the same
// runs.  A query skips its own sorted position; every other target counts, at distance 0 too.  All arithmetic is fp64 on the float32
// coordinates, dist2 of cloud_grid.hpp, no contraction.  A point with key INT64_MAX (not finite, or outside the grid) is no
// neighbour of anybody -- no search reaches its key -- and as a query it is flagged isolated (count 0).
//
// KNearest<K>: v[0 .. K) ascending; the first K - k slots hold -Inf and never move (c < -Inf is false), the last k slots hold the
// k smallest squared distances seen so far (+Inf until found), so the k-th smallest is always v[K - 1] -- a constant index -- and
// d2, the value the ring walk's stop bound looks at, is a copy of it.  One insert is a chain of K compare-exchanges on constant
// indices: the array lives in registers (no scratch; `make resource-usage`).  A candidate that is not below v[K - 1] (NaN included)
// leaves before the chain.  The result is a function of the SET of distances, whatever the order the walk meets them in.
//
// The walk ends on a stop bound when d2 <= lb^2 (every unvisited target is farther than lb: the k smallest are final and, since
// lb < cap, not isolated) or lb >= cap (every target with d2 <= cap * cap has been visited).  Either way
//     isolated  <=>  fewer than k other points with d2 <= cap * cap  <=>  !(v[K - 1] <= cap * cap),
// independent of the grid.  Otherwise m = (sqrt(v[K - k]) + ... + sqrt(v[K - 1])) / k, added in ascending order from 0.0.
//
// RadiusCount: d2 is the constant r * r until `limit` neighbours are counted and -1 afterwards, which stops the walk at the next
// ring (nothing more can change min(count, limit)); the walk's cap is r, so it ends when the ring bound reaches r.
#include "cloud_grid.hpp"

namespace itermvs {

constexpr int kKnnMaxK = 32;
constexpr int kRadiusMaxRings = 64;                    // itermvs_cloud_radius_count: r may span at most this many rings of cells
constexpr uint8_t kKnnSettled = 0, kKnnIsolated = 1, kKnnRingsUsedUp = 2;

template <int K>
struct KNearest {
    double d2;
    double v[K];
    long long self;
    __device__ __forceinline__ KNearest take(long long j, double c) const {
        KNearest o = *this;
        if (j == self || !(c < v[K - 1])) return o;        // NaN never enters
        double x = c;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const double lo = x < o.v[t] ? x : o.v[t], hi = x < o.v[t] ? o.v[t] : x;
            o.v[t] = lo;
            x = hi;
        }
        o.d2 = o.v[K - 1];
        return o;
    }
};

struct RadiusCount {
    double d2, r2;
    long long self;
    int count, limit;
    __device__ __forceinline__ RadiusCount take(long long j, double c) const {
        RadiusCount o = *this;
        if (j != self && c <= r2 && count < limit) {        // NaN: false
            o.count = count + 1;
            if (o.count >= limit) o.d2 = -1.0;
        }
        return o;
    }
};

// the sorted position a lane works on, or -1
__device__ __forceinline__ long long filter_position(const long long* __restrict__ index, long long n_index, long long n) {
    const long long lane = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (lane >= (index ? n_index : n)) return -1;
    const long long i = index ? index[lane] : lane;
    return i < 0 || i >= n ? -1 : i;
}

template <int K>
__global__ void __launch_bounds__(kCloudBlock) cloud_knn_mean_kernel(const float* __restrict__ xyz, const long long* __restrict__ keys,
                                                                     const long long* __restrict__ perm, long long n,
                                                                     const long long* __restrict__ index, long long n_index,
                                                                     CloudGrid g, int k, double cap, int rings,
                                                                     double* __restrict__ mean, uint8_t* __restrict__ flag) {
    const long long i = filter_position(index, n_index, n);
    if (i < 0) return;
    const long long o = perm[i];
    if (o < 0 || o >= n) return;
    const long long key = keys[i];
    if (key == kNoKey) {
        mean[o] = INFINITY;
        flag[o] = kKnnIsolated;
        return;
    }
    int cx, cy, cz;
    cell_from_key(key, g, cx, cy, cz);
    const CloudPoint q = load_point(xyz, i);
    KNearest<K> best;
#pragma unroll
    for (int t = 0; t < K; ++t) best.v[t] = t < K - k ? -INFINITY : INFINITY;
    best.d2 = INFINITY;
    best.self = i;
    const bool found = ring_walk(xyz, keys, n, g, cx, cy, cz, q.x, q.y, q.z, cap, rings, best);
    double m = INFINITY;
    uint8_t f = kKnnRingsUsedUp;
    if (found) {
        f = best.v[K - 1] <= cap * cap ? kKnnSettled : kKnnIsolated;
        if (f == kKnnSettled) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t >= K - k) s += sqrt(best.v[t]);
            m = s / (double)k;
        }
    }
    mean[o] = m;
    flag[o] = f;
}

__global__ void __launch_bounds__(kCloudBlock) cloud_radius_count_kernel(const float* __restrict__ xyz,
                                                                         const long long* __restrict__ keys,
                                                                         const long long* __restrict__ perm, long long n, CloudGrid g,
                                                                         double r, int limit, int rings, int* __restrict__ count) {
    const long long i = filter_position(nullptr, 0, n);
    if (i < 0) return;
    const long long o = perm[i];
    if (o < 0 || o >= n) return;
    const long long key = keys[i];
    if (key == kNoKey) {
        count[o] = 0;
        return;
    }
    int cx, cy, cz;
    cell_from_key(key, g, cx, cy, cz);
    const CloudPoint q = load_point(xyz, i);
    RadiusCount best{r * r, r * r, i, 0, limit};
    ring_walk(xyz, keys, n, g, cx, cy, cz, q.x, q.y, q.z, r, rings, best);       // rings reach r: the walk always ends on a bound
    count[o] = best.count;
}

// the first ring whose lower bound reaches `reach`, or 0 when it lies past `most`
static inline int rings_to_reach(double reach, double edge, int most) {
    for (int r = 1; r <= most; ++r)
        if ((double)(r - 1) * edge * kRingShrink >= reach) return r;
    return 0;
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_cloud_knn_mean(const float* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n,
                                      const int64_t* index, int64_t n_index, double ox, double oy, double oz, int32_t nx,
                                      int32_t ny, int32_t nz, double edge, int32_t k, double cap, int32_t rings, double* mean,
                                      uint8_t* flag, void* stream) {
    ITERMVS_RETURN_IF(!xyz_sorted || !keys_sorted || !perm || !mean || !flag, ITERMVS_ERR_NULL);
    CloudGrid g;
    const int bad = check_grid(n, ox, oy, oz, nx, ny, nz, edge, &g);
    ITERMVS_RETURN_IF(bad, bad);
    ITERMVS_RETURN_IF(k < 1 || k > kKnnMaxK || n <= k || (index && (n_index < 1 || n_index > n)), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(check_walk(cap, rings), ITERMVS_ERR_DIMS);
    const FlatItems items{index ? n_index : n, kCloudMaxPoints};
    const hipStream_t s = (hipStream_t)stream;
#define ITERMVS_KNN_LAUNCH(K)                                                                                                     \
    return flat_launch<cloud_knn_mean_kernel<K>, kCloudBlock>(items, s, xyz_sorted, (const long long*)keys_sorted,                \
        (const long long*)perm, (long long)n, (const long long*)index, (long long)n_index, g, (int)k, cap, (int)rings, mean, flag)
    if (k <= 8) ITERMVS_KNN_LAUNCH(8);
    if (k <= 16) ITERMVS_KNN_LAUNCH(16);
    ITERMVS_KNN_LAUNCH(32);
#undef ITERMVS_KNN_LAUNCH
}

extern "C" int itermvs_cloud_radius_count(const float* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n,
                                          double ox, double oy, double oz, int32_t nx, int32_t ny, int32_t nz, double edge,
                                          double r, int32_t limit, int32_t* count, void* stream) {
    ITERMVS_RETURN_IF(!xyz_sorted || !keys_sorted || !perm || !count, ITERMVS_ERR_NULL);
    CloudGrid g;
    const int bad = check_grid(n, ox, oy, oz, nx, ny, nz, edge, &g);
    ITERMVS_RETURN_IF(bad, bad);
    ITERMVS_RETURN_IF(!isfinite(r) || !(r > 0.0) || limit < 1, ITERMVS_ERR_DIMS);
    const int rings = rings_to_reach(r, edge, kRadiusMaxRings);
    ITERMVS_RETURN_IF(rings < 1, ITERMVS_ERR_DIMS);            // cells far smaller than r: a bad grid for this search
    return flat_launch<cloud_radius_count_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, xyz_sorted,
        (const long long*)keys_sorted, (const long long*)perm, (long long)n, g, r, (int)limit, rings, (int*)count);
}
