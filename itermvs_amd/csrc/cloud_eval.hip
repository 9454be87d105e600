// The searches of the DTU point-cloud evaluation (the .m scripts under evaluations/dtu of the reference; host side: itermvs_amd/cloud_eval.py).
//
// All arithmetic is fp64 on float32 coordinates (MATLAB converts to double first).  The squared distance is
// ((dx*dx) + (dy*dy)) + (dz*dz) in that order without contraction (the library is built with -ffp-contract=off), the distance
// its IEEE sqrt, so a numpy restatement gives the same bits.
//
// The neighbour structure is a uniform grid: cell = floor((p - origin) / edge) per axis, key = (cx * ny + cy) * nz + cz
// (int64; every dimension <= 2^21, so the key fits 63 bits).  The host sorts the points by key (torch.sort: plumbing); the
// kernels find a run of cells cz0..cz1 of one (cx, cy) row -- contiguous in key order -- with one binary search over the sorted
// keys and walk it.  Every position they read is the result of that search (inside [0, n)) or a counter below n; no value read
// from a table is used as an address.  A point that is not finite or lies outside the grid gets key INT64_MAX: it sorts last
// and no search reaches it.
//
// itermvs_cloud_reduce_round (reducePts_haa.m:24-30).  The sequential loop visits the points in a given order; a point still
// kept removes every other point within dst (d2 <= dst*dst, inclusive like rangesearch).  Its result is the unique fixed point
// of "kept <=> every neighbour earlier in the order is removed; removed <=> some earlier neighbour is kept".  One round: one lane
// per undecided point scans the 27 cells around it (edge >= dst); an earlier kept neighbour decides "removed", no earlier
// undecided neighbour decides "kept", otherwise the point waits for the next round.  States only move undecided -> decided and
// a decision reads decided neighbours only, so updating in place is benign: whatever a lane sees of a concurrent store, it
// decides what the sequential loop decides, or nothing yet.  No workgroup waits on another; the host launches rounds until the
// round's count of undecided points is zero (every round decides at least the earliest undecided point).
//
// itermvs_cloud_nn_distance (MaxDistCP.m).  For a query inside the region the script's blocks cover, rings of cells around the
// query's cell are searched outwards (ring r = the cells at Chebyshev cell distance r) until the best squared distance is at
// most the lower bound of the next ring, ((r - 1) * edge)^2 shrunk by 2^-20 for the rounding of the cell assignment, or that
// bound reaches the cap.  Result: min(distance to the nearest target, cap); cap for queries outside the region.
// Deliberate difference from MaxDistCP.m: inside a block MATLAB returns the distance to the nearest point of the ENLARGED BLOCK
// (the block grown by cap on every side), which can exceed cap; every consumer discards distances >= 20 and every target closer
// than cap lies inside the enlarged block, so all distances below cap are the same numbers.  The one-ulp seams between
// neighbouring blocks' Low / High (Low + cap of one block against BB + (x + 1) * cap of the next) are not reproduced either: the
// region is the union lo <= x < hi with hi = (BB(1) + Range * cap) + cap.
//
// itermvs_cloud_in_mask (PointCompareMain.m:32-41): v = round(((p - BB(1)) / Res) + 1) with C round() = MATLAB's round (half away
// from zero), inside 1..size on all three axes, and ObsMask(v) set.
#include "cloud_grid.hpp"

namespace itermvs {

__global__ void __launch_bounds__(kCloudBlock) cloud_cell_keys_kernel(const float* __restrict__ xyz, long long n, CloudGrid g,
                                                                      long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (i >= n) return;
    const double cx = cell_of((double)xyz[i * 3 + 0], g.ox, g.edge), cy = cell_of((double)xyz[i * 3 + 1], g.oy, g.edge),
                 cz = cell_of((double)xyz[i * 3 + 2], g.oz, g.edge);
    const bool in = cx >= 0.0 && cx < (double)g.nx && cy >= 0.0 && cy < (double)g.ny && cz >= 0.0 && cz < (double)g.nz;   // NaN: false
    keys[i] = in ? ((long long)cx * g.ny + (long long)cy) * g.nz + (long long)cz : kNoKey;
}

constexpr int kUndecided = 0, kKept = 1, kRemoved = 2;

// one lane per point of the key-sorted cloud; rank = the point's position in the visiting order
__global__ void __launch_bounds__(kCloudBlock) cloud_reduce_round_kernel(const float* __restrict__ xyz,
                                                                         const long long* __restrict__ keys,
                                                                         const int* __restrict__ rank, long long n, CloudGrid g,
                                                                         double dst2, int* state, int* __restrict__ undecided) {
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (i >= n) return;
    if (__hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kUndecided) return;
    const long long key = keys[i];
    if (key == kNoKey) {                                   // not finite / outside the grid: never kept, removes nobody
        __hip_atomic_store(&state[i], kRemoved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    int cx, cy, cz;
    cell_from_key(key, g, cx, cy, cz);
    const CloudPoint q = load_point(xyz, i);
    const int my = rank[i];
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < g.nx - 1 ? cx + 1 : g.nx - 1;
    const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < g.ny - 1 ? cy + 1 : g.ny - 1;
    const int z0 = cz > 0 ? cz - 1 : 0, z1 = cz < g.nz - 1 ? cz + 1 : g.nz - 1;
    bool blocked = false;
    for (int x = x0; x <= x1; ++x) {
        for (int y = y0; y <= y1; ++y) {
            const long long row = ((long long)x * g.ny + y) * g.nz, last = row + z1;
            for (long long j = lower_bound(keys, n, row + z0); j < n && keys[j] <= last; ++j) {
                if (j == i || rank[j] >= my || dist2(q.x, q.y, q.z, xyz + j * 3) > dst2) continue;
                const int s = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (s == kKept) {                          // reducePts_haa.m:27: an earlier kept point removes this one
                    __hip_atomic_store(&state[i], kRemoved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return;
                }
                blocked = blocked || s == kUndecided;
            }
        }
    }
    if (blocked)
        atomicAdd(undecided, 1);
    else
        __hip_atomic_store(&state[i], kKept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct CloudRegion {
    double lo[3], hi[3];
};

// one lane per query (index[i] when an index list is given).  best_d2 / done carry the search from one grid to the next
__global__ void __launch_bounds__(kCloudBlock) cloud_nn_distance_kernel(const float* __restrict__ q, long long nq,
                                                                        const long long* __restrict__ index, long long n_index,
                                                                        const float* __restrict__ t,
                                                                        const long long* __restrict__ keys, long long nt,
                                                                        CloudGrid g, CloudRegion reg, double cap, int rings,
                                                                        double* __restrict__ best_d2, uint8_t* __restrict__ done,
                                                                        double* __restrict__ dist) {
    const long long lane = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (lane >= (index ? n_index : nq)) return;
    const long long i = index ? index[lane] : lane;
    if (i < 0 || i >= nq || done[i]) return;
    const double qx = (double)q[i * 3 + 0], qy = (double)q[i * 3 + 1], qz = (double)q[i * 3 + 2];
    if (!(qx >= reg.lo[0] && qx < reg.hi[0] && qy >= reg.lo[1] && qy < reg.hi[1] && qz >= reg.lo[2] && qz < reg.hi[2])) {
        done[i] = 1;                                       // MaxDistCP.m:3: no block looks at it (NaN included)
        dist[i] = cap;
        return;
    }
    const int cx = clamped_cell(qx, g.ox, g.edge), cy = clamped_cell(qy, g.oy, g.edge), cz = clamped_cell(qz, g.oz, g.edge);
    NearestDistance nearest{best_d2[i]};
    const bool found = ring_walk(t, keys, nt, g, cx, cy, cz, qx, qy, qz, cap, rings, nearest);
    const double best = nearest.d2;
    const double d = sqrt(best);
    best_d2[i] = best;
    done[i] = found ? 1 : 0;
    dist[i] = d < cap ? d : cap;
}

__global__ void __launch_bounds__(kCloudBlock) cloud_in_mask_kernel(const float* __restrict__ xyz, long long n,
                                                                    const uint8_t* __restrict__ mask, int sx, int sy, int sz,
                                                                    double bx, double by, double bz, double res,
                                                                    uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kCloudBlock + threadIdx.x;
    if (i >= n) return;
    const double vx = round((((double)xyz[i * 3 + 0] - bx) / res) + 1.0), vy = round((((double)xyz[i * 3 + 1] - by) / res) + 1.0),
                 vz = round((((double)xyz[i * 3 + 2] - bz) / res) + 1.0);
    uint8_t in = 0;
    if (vx > 0.0 && vx <= (double)sx && vy > 0.0 && vy <= (double)sy && vz > 0.0 && vz <= (double)sz)          // NaN: false
        in = mask[(((long long)vx - 1) * sy + ((long long)vy - 1)) * sz + ((long long)vz - 1)] != 0;
    out[i] = in;
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_cloud_cell_keys(const float* xyz, int64_t n, double ox, double oy, double oz, int32_t nx, int32_t ny,
                                       int32_t nz, double edge, int64_t* keys, void* stream) {
    ITERMVS_RETURN_IF(!xyz || !keys, ITERMVS_ERR_NULL);
    CloudGrid g;
    const int bad = check_grid(n, ox, oy, oz, nx, ny, nz, edge, &g);
    ITERMVS_RETURN_IF(bad, bad);
    return flat_launch<cloud_cell_keys_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, xyz, (long long)n, g, (long long*)keys);
}

extern "C" int itermvs_cloud_reduce_round(const float* xyz_sorted, const int64_t* keys_sorted, const int32_t* rank_sorted,
                                          int64_t n, double ox, double oy, double oz, int32_t nx, int32_t ny, int32_t nz,
                                          double edge, double dst, int32_t* state, int32_t* undecided, void* stream) {
    ITERMVS_RETURN_IF(!xyz_sorted || !keys_sorted || !rank_sorted || !state || !undecided, ITERMVS_ERR_NULL);
    CloudGrid g;
    const int bad = check_grid(n, ox, oy, oz, nx, ny, nz, edge, &g);
    ITERMVS_RETURN_IF(bad, bad);
    ITERMVS_RETURN_IF(!isfinite(dst) || !(dst > 0.0) || edge < dst, ITERMVS_ERR_DIMS);      // 27 cells must hold the radius
    return flat_launch<cloud_reduce_round_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, xyz_sorted,
        (const long long*)keys_sorted, (const int*)rank_sorted, (long long)n, g, dst * dst, (int*)state, (int*)undecided);
}

extern "C" int itermvs_cloud_nn_distance(const float* q_from, int64_t nq, const int64_t* index, int64_t n_index,
                                         const float* to_sorted, const int64_t* keys_sorted, int64_t nt, double ox, double oy,
                                         double oz, int32_t nx, int32_t ny, int32_t nz, double edge, const double* region,
                                         double cap, int32_t rings, double* best_d2, uint8_t* done, double* dist, void* stream) {
    ITERMVS_RETURN_IF(!q_from || !to_sorted || !keys_sorted || !region || !best_d2 || !done || !dist, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(nq < 1 || nq > kCloudMaxPoints || (index && (n_index < 1 || n_index > nq)), ITERMVS_ERR_DIMS);
    CloudGrid g;
    const int bad = check_grid(nt, ox, oy, oz, nx, ny, nz, edge, &g);
    ITERMVS_RETURN_IF(bad, bad);
    ITERMVS_RETURN_IF(check_walk(cap, rings), ITERMVS_ERR_DIMS);
    CloudRegion reg;
    for (int a = 0; a < 3; ++a) {
        reg.lo[a] = region[a];                             // host memory: BB(1,:) and (BB(1,:) + Range * cap) + cap
        reg.hi[a] = region[3 + a];
    }
    return flat_launch<cloud_nn_distance_kernel, kCloudBlock>({index ? n_index : nq, kCloudMaxPoints}, (hipStream_t)stream, q_from, (long long)nq,
        (const long long*)index, (long long)n_index, to_sorted, (const long long*)keys_sorted, (long long)nt, g, reg, cap, rings, best_d2, done,
        dist);
}

extern "C" int itermvs_cloud_in_mask(const float* xyz, int64_t n, const uint8_t* mask, int32_t sx, int32_t sy, int32_t sz,
                                     double bx, double by, double bz, double res, uint8_t* out, void* stream) {
    ITERMVS_RETURN_IF(!xyz || !mask || !out, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints || sx < 1 || sy < 1 || sz < 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(!finite_all(bx, by, bz, res) || !(res > 0.0), ITERMVS_ERR_DIMS);
    return flat_launch<cloud_in_mask_kernel, kCloudBlock>({n, kCloudMaxPoints}, (hipStream_t)stream, xyz, (long long)n, mask, sx, sy, sz, bx, by,
        bz, res, out);
}
