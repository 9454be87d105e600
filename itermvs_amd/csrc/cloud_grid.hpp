// The uniform grid of the cloud searches, shared by cloud_eval.hip (DTU), cloud_register.hip (Tanks and Temples) and
// cloud_filter.hip (outlier removal): the cell key, the binary search over the sorted keys, the squared distance, the ring walk
// with its stop bounds, and the entry points' checks of a grid and a walk.  Host counterpart: itermvs_amd/cloud_grid.py.
//
// cell = floor((p - origin) / edge) per axis, key = (cx * ny + cy) * nz + cz (int64; every dimension <= 2^21, so the key fits
// 63 bits).  The targets are sorted by key; the cells z0..z1 of one (cx, cy) row are contiguous in key order, so one binary
// search finds a row's run.  Every position read is the result of that search (inside [0, n)) or a counter below n.
//
// ring_walk: rings of cells around the query's cell are searched outwards (ring r = the cells at Chebyshev cell distance r)
// until the best squared distance is at most the lower bound of the next ring, ((r - 1) * edge)^2 shrunk by 2^-20 for
// the rounding of the cell assignment, or that bound reaches the cap.  The shrink also makes the bound strict: a target of ring
// r or beyond is farther than the bound, so none of them can tie with a best that stopped the walk.  ``Best`` is the search's
// running result: best.d2 is the squared distance the stop bounds look at, best.take(j, d2) the result after target position j.
#pragma once
#include <math.h>

#include "flat_launch.hpp"

namespace itermvs {

constexpr int kCloudBlock = 256;
constexpr int64_t kCloudMaxPoints = 0x7fffff00LL;      // points of one launch (tighter than flat_launch.hpp's own limit)
constexpr int kMaxCellDim = 1 << 21;                    // per axis: three axes fit a 63-bit key
constexpr double kCellClamp = 4194304.0;                // 2^22: a query's cell far outside the grid, still safe in int arithmetic
constexpr double kRingShrink = 1.0 - 1.0 / 1048576.0;   // ring lower bounds give way 2^-20 to the rounding of (p - origin) / edge
constexpr long long kNoKey = 0x7fffffffffffffffLL;

struct CloudGrid {
    double ox, oy, oz, edge;
    int nx, ny, nz;
};

struct CloudPoint {
    double x, y, z;
};

__device__ __forceinline__ double cell_of(double p, double o, double edge) {
    return floor((p - o) / edge);
}

// the cell a key (not kNoKey) names
__device__ __forceinline__ void cell_from_key(long long key, const CloudGrid& g, int& cx, int& cy, int& cz) {
    cz = (int)(key % g.nz);
    cy = (int)((key / g.nz) % g.ny);
    cx = (int)(key / g.nz / g.ny);
}

__device__ __forceinline__ CloudPoint load_point(const float* __restrict__ xyz, long long i) {
    return CloudPoint{(double)xyz[i * 3 + 0], (double)xyz[i * 3 + 1], (double)xyz[i * 3 + 2]};
}

// first position in keys[0 : n) whose key is >= want; n < 2^31, so 32 halvings always finish
__device__ __forceinline__ long long lower_bound(const long long* __restrict__ keys, long long n, long long want) {
    long long lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double dist2(double qx, double qy, double qz, const float* __restrict__ p) {
    const double dx = qx - (double)p[0], dy = qy - (double)p[1], dz = qz - (double)p[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// the query's cell on one axis, clamped so that cell +- ring stays in int range
__device__ __forceinline__ int clamped_cell(double p, double o, double edge) {
    return (int)fmin(fmax(cell_of(p, o, edge), -kCellClamp), kCellClamp);
}

// the targets of the cells z0..z1 (clipped to the grid) of row (x, y)
template <class Best>
__device__ __forceinline__ Best scan_cells(const float* __restrict__ t, const long long* __restrict__ keys, long long nt,
                                           const CloudGrid& g, int x, int y, int z0, int z1, double qx, double qy, double qz,
                                           Best best) {
    z0 = z0 < 0 ? 0 : z0;
    z1 = z1 > g.nz - 1 ? g.nz - 1 : z1;
    if (z0 > z1) return best;
    const long long row = ((long long)x * g.ny + y) * g.nz, last = row + z1;
    for (long long j = lower_bound(keys, nt, row + z0); j < nt && keys[j] <= last; ++j) {
        const double d2 = dist2(qx, qy, qz, t + j * 3);
        best = best.take(j, d2);
    }
    return best;
}

// rings 0 .. rings - 1 around cell (cx, cy, cz), updating ``best``; true when a stop bound ended the walk (the result is final
// on this grid), false when the rings were used up first
template <class Best>
__device__ __forceinline__ bool ring_walk(const float* __restrict__ t, const long long* __restrict__ keys, long long nt,
                                          const CloudGrid& g, int cx, int cy, int cz, double qx, double qy, double qz, double cap,
                                          int rings, Best& out) {
    Best best = out;
    bool found = false;
    for (int r = 0; r <= rings; ++r) {
        if (r >= 1) {                                      // every target of ring r or beyond is at least (r - 1) * edge away
            const double lb = (double)(r - 1) * g.edge * kRingShrink;
            if (best.d2 <= lb * lb || lb >= cap) {
                found = true;
                break;
            }
        }
        if (r == rings) break;                             // this grid's rings are used up: the next grid goes on
        const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < g.nx - 1 ? cx + r : g.nx - 1;
        const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < g.ny - 1 ? cy + r : g.ny - 1;
        for (int x = x0; x <= x1; ++x) {
            for (int y = y0; y <= y1; ++y) {
                if (x - cx == r || cx - x == r || y - cy == r || cy - y == r) {
                    best = scan_cells(t, keys, nt, g, x, y, cz - r, cz + r, qx, qy, qz, best);
                } else {                                   // inside the ring's square: its bottom and its lid
                    best = scan_cells(t, keys, nt, g, x, y, cz - r, cz - r, qx, qy, qz, best);
                    best = scan_cells(t, keys, nt, g, x, y, cz + r, cz + r, qx, qy, qz, best);
                }
            }
        }
    }
    out = best;
    return found;
}

// the best of a distance-only search
struct NearestDistance {
    double d2;
    __device__ __forceinline__ NearestDistance take(long long, double c) const { return NearestDistance{c < d2 ? c : d2}; }   // NaN never wins
};

static inline bool finite_all(double a, double b, double c, double d) {
    return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d);
}

// ITERMVS_OK and the grid in *g, or the error of a grid description; n is the number of points of the launch
static inline int check_grid(long long n, double ox, double oy, double oz, int nx, int ny, int nz, double edge, CloudGrid* g) {
    ITERMVS_RETURN_IF(n < 1 || n > kCloudMaxPoints, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(!finite_all(ox, oy, oz, edge) || !(edge > 0.0), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(nx < 1 || ny < 1 || nz < 1 || nx > kMaxCellDim || ny > kMaxCellDim || nz > kMaxCellDim, ITERMVS_ERR_DIMS);
    *g = CloudGrid{ox, oy, oz, edge, nx, ny, nz};
    return ITERMVS_OK;
}

// ITERMVS_OK or the error of a ring walk's cap and number of rings
static inline int check_walk(double cap, int rings) {
    ITERMVS_RETURN_IF(!isfinite(cap) || !(cap > 0.0) || rings < 1 || rings > kMaxCellDim, ITERMVS_ERR_DIMS);
    return ITERMVS_OK;
}

}  // namespace itermvs
