// Volumetric fusion of the fused depth maps into a triangle mesh (eval.py --mesh; no counterpart in the reference).  The definition of
// both entry points, every step of the arithmetic, is in include/itermvs_hip.h; the numpy restatement is tests/tsdf_reference.py.
// itermvs_tsdf_integrate: one launch, one thread per voxel.  The thread loads its 12-byte state once, walks the batch's views in the given
//   order and stores the state once: the volume is read and written once per BATCH, which is what bounds the kernel.
// itermvs_tsdf_mesh: marching tetrahedra (tsdf_tets.hpp) in a memset and five launches on the stream, 256 consecutive voxels per workgroup:
//   mark   : a thread owns the cell whose corner 0 is its voxel; a valid cell stores the constant 1 into the mark byte of each of its 19
//            edges whose ends differ in sign (plain byte stores, several cells may store the same 1) and its triangle count into a byte;
//   count  : per workgroup the number of marks of its voxels' 7 edges and of its cells' triangles -> workspace;
//   scan   : ONE workgroup turns both count arrays into exclusive offsets in place and writes the two totals;
//   vertex : every thread ranks its voxel's marks (offset + ranks inside the workgroup), keeps its first vertex index and stores the
//            vertex records whose index is below the capacity;
//   face   : every thread ranks its cell's triangles the same way and stores the index triples below the capacity; a corner's vertex
//            index is its voxel's first index + the marks of that voxel below the edge's direction.
// Ordering comes from the stream alone: no workgroup waits on another, no atomics, so the bytes do not depend on scheduling.
#include <cmath>

#include "cam_math.hpp"
#include "flat_launch.hpp"
#include "tsdf_tets.hpp"
#include "wave_ops.hpp"

namespace itermvs {

constexpr int kTsdfBlock = 256;
constexpr int kTsdfWaves = kTsdfBlock / 64;
constexpr int kTsdfScanBlock = 1024;
constexpr uint32_t kTsdfMaxCount = 257;        // 257 * 255 = 65535: the largest colour sum a uint16 holds
constexpr int kMeshVertexBytes = 15;           // x y z float32 | red green blue uint8

// n = nx * ny * nz voxels, x fastest; nxy = nx * ny (both < 2^32 by the flat bound)
struct TsdfGrid {
    uint32_t n, nx, ny, nxy;
    double ox, oy, oz, voxel;
};

// voxel state, 12 bytes: fp32 sum_t | uint16 count | uint16 red, green, blue sums = three little-endian 32-bit words
struct TsdfVoxel {
    float sum;
    uint32_t count, r, g, b;
};
__device__ __forceinline__ TsdfVoxel tsdf_load(const uint32_t* __restrict__ state, uint32_t idx) {
    const uint32_t* s = state + (size_t)idx * 3;
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
    return {__uint_as_float(w0), w1 & 0xffffu, w1 >> 16, w2 & 0xffffu, w2 >> 16};
}

__device__ __forceinline__ void tsdf_split(const TsdfGrid& g, uint32_t idx, uint32_t& ix, uint32_t& iy, uint32_t& iz) {
    const uint32_t row = idx / g.nx;
    ix = idx - row * g.nx;
    iz = row / g.ny;
    iy = row - iz * g.ny;
}
__device__ __forceinline__ double tsdf_centre(double o, uint32_t i, double voxel) { return o + ((double)i + 0.5) * voxel; }

__global__ void __launch_bounds__(kTsdfBlock) tsdf_integrate_kernel(uint32_t* __restrict__ state, TsdfGrid g, double trunc,
                                                                    const double* __restrict__ depth, const uint8_t* __restrict__ mask,
                                                                    const float* __restrict__ cams, const uint8_t* __restrict__ rgb,
                                                                    int V, uint32_t H, uint32_t W) {
    const uint32_t idx = blockIdx.x * kTsdfBlock + threadIdx.x;
    if (idx >= g.n) return;
    uint32_t ix, iy, iz;
    tsdf_split(g, idx, ix, iy, iz);
    const double cx = tsdf_centre(g.ox, ix, g.voxel), cy = tsdf_centre(g.oy, iy, g.voxel), cz = tsdf_centre(g.oz, iz, g.voxel);
    TsdfVoxel s = tsdf_load(state, idx);
    const size_t hw = (size_t)H * W;
    const double xmax = (double)(W - 1), ymax = (double)(H - 1);
    for (int v = 0; v < V && s.count < kTsdfMaxCount; ++v) {
        const float* __restrict__ k = cams + (size_t)v * 21;
        const float* __restrict__ e = k + 9;
        // mat34(e, ...) of cam_math.hpp spelled out: profiles/wave_ops/README.md has what the inlined call cost this kernel
        const double px = (((double)e[0] * cx + (double)e[1] * cy) + (double)e[2] * cz) + (double)e[3] * 1.0;
        const double py = (((double)e[4] * cx + (double)e[5] * cy) + (double)e[6] * cz) + (double)e[7] * 1.0;
        const double pz = (((double)e[8] * cx + (double)e[9] * cy) + (double)e[10] * cz) + (double)e[11] * 1.0;
        if (!(std::isfinite(pz) && pz > 0.0)) continue;
        const double ux = (((double)k[0] * px + (double)k[1] * py) + (double)k[2] * pz) / pz;
        const double uy = (((double)k[3] * px + (double)k[4] * py) + (double)k[5] * pz) / pz;
        const double rx = rint(ux), ry = rint(uy);
        if (!(rx >= 0.0 && rx <= xmax && ry >= 0.0 && ry <= ymax)) continue;          // NaN and inf fail
        const size_t q = (size_t)v * hw + ((size_t)(uint32_t)ry * W + (uint32_t)rx);
        if (mask[q] == 0) continue;
        const double d = depth[q];
        if (!(std::isfinite(d) && d > 0.0)) continue;
        const double sdf = d - pz;
        if (sdf < -trunc) continue;
        s.sum += (float)fmin(1.0, sdf / trunc);
        const uint8_t* c = rgb + q * 3;
        s.r += c[0]; s.g += c[1]; s.b += c[2];
        ++s.count;
    }
    uint32_t* o = state + (size_t)idx * 3;
    o[0] = __float_as_uint(s.sum);
    o[1] = s.count | (s.r << 16);
    o[2] = s.g | (s.b << 16);
}

// ---- marching tetrahedra ----

// value of a valid voxel
__device__ __forceinline__ bool tsdf_value(const TsdfVoxel& s, uint32_t min_count, float& f) {
    if (s.count < min_count) return false;
    f = s.sum / (float)s.count;
    return true;
}
__device__ __forceinline__ uint32_t tsdf_corner(const TsdfGrid& g, uint32_t idx, int c) {
    return idx + (uint32_t)(c & 1) + (uint32_t)((c >> 1) & 1) * g.nx + (uint32_t)(c >> 2) * g.nxy;
}

// the 8-bit inside mask of the cell whose corner 0 is voxel idx (< n); -1: no such cell (last layer of an axis) or a corner is not valid
__device__ __forceinline__ int tsdf_cell(const uint32_t* __restrict__ state, const TsdfGrid& g, uint32_t idx, uint32_t min_count) {
    uint32_t ix, iy, iz;
    tsdf_split(g, idx, ix, iy, iz);
    if (ix + 1 >= g.nx || iy + 1 >= g.ny || (uint64_t)idx + g.nxy >= g.n) return -1;
    int m = 0;
    for (int c = 0; c < 8; ++c) {
        float f;
        if (!tsdf_value(tsdf_load(state, tsdf_corner(g, idx, c)), min_count, f)) return -1;
        m |= (f < 0.0f ? 1 : 0) << c;
    }
    return m;
}

__global__ void __launch_bounds__(kTsdfBlock) tsdf_mark_kernel(const uint32_t* __restrict__ state, TsdfGrid g, uint32_t min_count,
                                                               uint8_t* __restrict__ marks, uint8_t* __restrict__ cell_faces) {
    const uint32_t idx = blockIdx.x * kTsdfBlock + threadIdx.x;
    if (idx >= g.n) return;
    const int m = tsdf_cell(state, g, idx, min_count);
    int faces = 0;
    if (m > 0 && m < 255) {
        for (int t = 0; t < 6; ++t) faces += tsdf_tet_triangles(tsdf_tet_mask(t, m));
        for (int lo = 0; lo < 7; ++lo)
            for (int d = 1; d < 8; ++d)
                if ((lo & d) == 0 && (((m >> lo) ^ (m >> (lo | d))) & 1))
                    marks[(size_t)tsdf_corner(g, idx, lo) * kTsdfDirs + tsdf_dir_of_bits(d)] = 1;
    }
    cell_faces[idx] = (uint8_t)faces;
}

__device__ __forceinline__ uint32_t tsdf_marks_of(const uint8_t* __restrict__ marks, uint32_t idx, int dirs) {
    const uint8_t* m = marks + (size_t)idx * kTsdfDirs;
    uint32_t n = 0;
    for (int d = 0; d < dirs; ++d) n += m[d] != 0;
    return n;
}

// counts: uint64 [2][nblocks] = vertices | triangles per workgroup
__global__ void __launch_bounds__(kTsdfBlock) tsdf_count_kernel(const uint8_t* __restrict__ marks, const uint8_t* __restrict__ cell_faces,
                                                                uint32_t n, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t part[2][kTsdfWaves];
    const uint32_t idx = blockIdx.x * kTsdfBlock + threadIdx.x;
    const uint32_t nv = wave_sum_lane0(idx < n ? tsdf_marks_of(marks, idx, kTsdfDirs) : 0u);
    const uint32_t nf = wave_sum_lane0(idx < n ? (uint32_t)cell_faces[idx] : 0u);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = nv; part[1][threadIdx.x >> 6] = nf; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (int wv = 0; wv < kTsdfWaves; ++wv) s += part[threadIdx.x][wv];
        counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// one workgroup: both rows of counts -> exclusive offsets in place; totals[0] = vertices, totals[1] = triangles
__global__ void __launch_bounds__(kTsdfScanBlock) tsdf_scan_kernel(unsigned long long* __restrict__ counts, uint32_t nblocks,
                                                                   unsigned long long* __restrict__ totals) {
    for (int row = 0; row < 2; ++row) {
        const auto total = block_scan_exclusive_chunked<unsigned long long, kTsdfScanBlock>(counts + (size_t)row * nblocks, nblocks, [](uint32_t) {});
        if (threadIdx.x == 0) totals[row] = total;
    }
}

// v items of this thread -> the items of the workgroup's threads before it; every thread of the workgroup calls it, once per kernel
__device__ __forceinline__ uint32_t tsdf_block_rank(uint32_t v) {
    return block_exclusive<kTsdfWaves>(wave_inclusive_scan(v), v);
}

__device__ __forceinline__ uint8_t tsdf_colour(uint32_t sa, uint32_t na, uint32_t sb, uint32_t nb, double s) {
    const double a = (double)sa / (double)na, b = (double)sb / (double)nb;
    return (uint8_t)fmin(255.0, fmax(0.0, rint(a + s * (b - a))));
}

__global__ void __launch_bounds__(kTsdfBlock) tsdf_vertex_kernel(const uint32_t* __restrict__ state, TsdfGrid g,
                                                                 const uint8_t* __restrict__ marks,
                                                                 const unsigned long long* __restrict__ offsets,
                                                                 uint32_t* __restrict__ first_vertex, uint8_t* __restrict__ vertices,
                                                                 unsigned long long capacity) {
    const uint32_t idx = blockIdx.x * kTsdfBlock + threadIdx.x;
    const bool in = idx < g.n;
    const uint32_t nv = in ? tsdf_marks_of(marks, idx, kTsdfDirs) : 0u;
    unsigned long long vi = offsets[blockIdx.x] + tsdf_block_rank(nv);
    if (!in) return;
    first_vertex[idx] = (uint32_t)vi;
    if (nv == 0) return;
    uint32_t ix, iy, iz;
    tsdf_split(g, idx, ix, iy, iz);
    const TsdfVoxel a = tsdf_load(state, idx);
    const float fa = a.sum / (float)a.count;
    const uint8_t* m = marks + (size_t)idx * kTsdfDirs;
    for (int dir = 0; dir < kTsdfDirs; ++dir) {
        if (m[dir] == 0) continue;
        const unsigned long long at = vi++;
        if (at >= capacity) continue;                      // the ONLY stores to vertices are guarded by at < capacity
        const int bits = tsdf_bits_of_dir(dir);
        const TsdfVoxel b = tsdf_load(state, tsdf_corner(g, idx, bits));
        const float fb = b.sum / (float)b.count;
        const double s = (double)fa / ((double)fa - (double)fb);
        const double xa = tsdf_centre(g.ox, ix, g.voxel), xb = tsdf_centre(g.ox, ix + (bits & 1), g.voxel);
        const double ya = tsdf_centre(g.oy, iy, g.voxel), yb = tsdf_centre(g.oy, iy + ((bits >> 1) & 1), g.voxel);
        const double za = tsdf_centre(g.oz, iz, g.voxel), zb = tsdf_centre(g.oz, iz + (bits >> 2), g.voxel);
        uint8_t* o = vertices + at * kMeshVertexBytes;
        put_f32_bytes(o, (float)(xa + s * (xb - xa)));
        put_f32_bytes(o + 4, (float)(ya + s * (yb - ya)));
        put_f32_bytes(o + 8, (float)(za + s * (zb - za)));
        o[12] = tsdf_colour(a.r, a.count, b.r, b.count, s);
        o[13] = tsdf_colour(a.g, a.count, b.g, b.count, s);
        o[14] = tsdf_colour(a.b, a.count, b.b, b.count, s);
    }
}

__global__ void __launch_bounds__(kTsdfBlock) tsdf_face_kernel(const uint32_t* __restrict__ state, TsdfGrid g, uint32_t min_count,
                                                               const uint8_t* __restrict__ marks, const uint8_t* __restrict__ cell_faces,
                                                               const unsigned long long* __restrict__ offsets,
                                                               const uint32_t* __restrict__ first_vertex, int32_t* __restrict__ faces,
                                                               unsigned long long capacity) {
    const uint32_t idx = blockIdx.x * kTsdfBlock + threadIdx.x;
    const uint32_t nf = idx < g.n ? cell_faces[idx] : 0u;
    unsigned long long fi = offsets[blockIdx.x] + tsdf_block_rank(nf);
    if (nf == 0) return;
    const int m = tsdf_cell(state, g, idx, min_count);     // nf > 0: the cell is valid
    for (int t = 0; t < 6; ++t) {
        const TetCase tc = tsdf_tet_case(tsdf_tet_mask(t, m));
        for (int k = 0; k < tc.n; ++k) {
            const unsigned long long at = fi++;
            if (at >= capacity) continue;                  // the ONLY stores to faces are guarded by at < capacity
            for (int v = 0; v < 3; ++v) {
                const int lo = tsdf_tet_corner(t, tc.edge[6 * k + 2 * v]), hi = tsdf_tet_corner(t, tc.edge[6 * k + 2 * v + 1]);
                const int from = lo & hi;                  // the corners of a tetrahedron are nested: the lower one
                const uint32_t owner = tsdf_corner(g, idx, from);
                faces[at * 3 + v] = (int32_t)(first_vertex[owner] + tsdf_marks_of(marks, owner, tsdf_dir_of_bits(lo ^ hi)));
            }
        }
    }
}

// workspace: counts uint64 [2][nblocks] | first_vertex uint32 [n] | marks uint8 [n][7] | cell_faces uint8 [n]
struct TsdfWorkspace {
    int64_t nblocks, first_vertex, marks, cell_faces, bytes;
};
static inline TsdfWorkspace tsdf_workspace(int64_t n) {
    TsdfWorkspace w;
    w.nblocks = (n - 1) / kTsdfBlock + 1;
    w.first_vertex = 2 * w.nblocks * 8;
    w.marks = w.first_vertex + 4 * n;
    w.cell_faces = w.marks + kTsdfDirs * n;
    w.bytes = w.cell_faces + n;
    return w;
}

// the volume's description, checked in this order by both entry points: dimensions, the flat bound, then voxel and the origin
static inline int tsdf_grid(int32_t nx, int32_t ny, int32_t nz, double ox, double oy, double oz, double voxel, TsdfGrid* g, dim3* grid) {
    ITERMVS_RETURN_IF(nx < 1 || ny < 1 || nz < 1, ITERMVS_ERR_DIMS);
    const int64_t n = flat_items({nx, ny, nz});
    ITERMVS_RETURN_IF(flat_grid({n}, kTsdfBlock, grid) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(!std::isfinite(voxel) || !(voxel > 0.0) || !std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oz),
                      ITERMVS_ERR_DIMS);
    *g = {(uint32_t)n, (uint32_t)nx, (uint32_t)ny, (uint32_t)((int64_t)nx * ny), ox, oy, oz, voxel};
    return ITERMVS_OK;
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_tsdf_tet_corners(int32_t tet, int32_t* corners) {
    ITERMVS_RETURN_IF(!corners, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(tet < 0 || tet > 5, ITERMVS_ERR_DIMS);
    for (int p = 0; p < 4; ++p) corners[p] = tsdf_tet_corner(tet, p);
    return ITERMVS_OK;
}

extern "C" int itermvs_tsdf_tet_case(int32_t mask, int32_t* edges) {
    ITERMVS_RETURN_IF(!edges, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(mask < 0 || mask > 15, ITERMVS_ERR_DIMS);
    const TetCase tc = tsdf_tet_case(mask);
    for (int i = 0; i < 12; ++i) edges[i] = i < 6 * tc.n ? tc.edge[i] : -1;
    return tc.n;
}

extern "C" int itermvs_tsdf_integrate(uint32_t* state, int32_t nx, int32_t ny, int32_t nz, double ox, double oy, double oz, double voxel,
                                      double trunc, const double* depth, const uint8_t* mask, const float* cams, const uint8_t* rgb,
                                      int32_t V, int32_t H, int32_t W, void* stream) {
    ITERMVS_RETURN_IF(!state || !depth || !mask || !cams || !rgb, ITERMVS_ERR_NULL);
    TsdfGrid g;
    dim3 grid;
    ITERMVS_RETURN_IF(tsdf_grid(nx, ny, nz, ox, oy, oz, voxel, &g, &grid) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(!std::isfinite(trunc) || !(trunc > 0.0), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(V < 1 || H < 1 || W < 1 || flat_items({H, W}) > kFlatInt32, ITERMVS_ERR_DIMS);
    return flat_launch<tsdf_integrate_kernel, kTsdfBlock>({(int64_t)g.n}, (hipStream_t)stream, state, g, trunc, depth, mask, cams, rgb,
                                                          (int)V, (uint32_t)H, (uint32_t)W);
}

extern "C" int itermvs_tsdf_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t* bytes) {
    ITERMVS_RETURN_IF(!bytes, ITERMVS_ERR_NULL);
    TsdfGrid g;
    dim3 grid;
    ITERMVS_RETURN_IF(tsdf_grid(nx, ny, nz, 0.0, 0.0, 0.0, 1.0, &g, &grid) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    *bytes = tsdf_workspace(g.n).bytes;
    return ITERMVS_OK;
}

extern "C" int itermvs_tsdf_mesh(const uint32_t* state, int32_t nx, int32_t ny, int32_t nz, double ox, double oy, double oz, double voxel,
                                 int32_t min_count, uint8_t* vertices, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity,
                                 uint64_t* totals, uint8_t* workspace, void* stream) {
    ITERMVS_RETURN_IF(!state || !totals || !workspace, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF((!vertices && vertex_capacity != 0) || (!faces && face_capacity != 0), ITERMVS_ERR_NULL);
    TsdfGrid g;
    dim3 grid;
    ITERMVS_RETURN_IF(tsdf_grid(nx, ny, nz, ox, oy, oz, voxel, &g, &grid) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(min_count < 1 || vertex_capacity < 0 || vertex_capacity > kFlatInt32 || face_capacity < 0, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(((uintptr_t)workspace & 7) != 0, ITERMVS_ERR_ALIGN);
    const TsdfWorkspace w = tsdf_workspace(g.n);
    unsigned long long* counts = (unsigned long long*)workspace;
    uint32_t* first_vertex = (uint32_t*)(workspace + w.first_vertex);
    uint8_t *marks = workspace + w.marks, *cell_faces = workspace + w.cell_faces;
    hipStream_t s = (hipStream_t)stream;
    const FlatItems items{(int64_t)g.n};
    ITERMVS_RETURN_IF(hipMemsetAsync(marks, 0, (size_t)kTsdfDirs * g.n, s) != hipSuccess, ITERMVS_ERR_LAUNCH);
    int bad = flat_launch<tsdf_mark_kernel, kTsdfBlock>(items, s, state, g, (uint32_t)min_count, marks, cell_faces);
    if (bad == ITERMVS_OK)
        bad = flat_launch<tsdf_count_kernel, kTsdfBlock>(items, s, (const uint8_t*)marks, (const uint8_t*)cell_faces, g.n, counts);
    if (bad != ITERMVS_OK) return bad;
    hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(kTsdfScanBlock), 0, s, counts, (uint32_t)w.nblocks,
                       (unsigned long long*)totals);
    bad = flat_launch<tsdf_vertex_kernel, kTsdfBlock>(items, s, state, g, (const uint8_t*)marks, (const unsigned long long*)counts,
                                                      first_vertex, vertices, (unsigned long long)vertex_capacity);
    if (bad != ITERMVS_OK) return bad;
    return flat_launch<tsdf_face_kernel, kTsdfBlock>(items, s, state, g, (uint32_t)min_count, (const uint8_t*)marks,
                                                     (const uint8_t*)cell_faces, (const unsigned long long*)(counts + w.nblocks),
                                                     (const uint32_t*)first_vertex, faces, (unsigned long long)face_capacity);
}
