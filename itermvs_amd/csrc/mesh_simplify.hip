// Simplification of an indexed triangle mesh by vertex clustering with quadric placement (eval.py --mesh_simplify, simplify_mesh.py;
// Lindstrom 2000; no counterpart in the reference).  The definition of the three entry points, with the order of every floating-point
// operation, is in include/itermvs_hip.h; the numpy restatement is tests/mesh_simplify_reference.py; the host side that sorts between
// them is itermvs_amd/fusion.py: simplify_mesh.
// itermvs_mesh_simplify_corners: one launch, one thread per face: the cluster of each corner (the pairs the host sorts by cluster)
//   and the canonical triple of a face that is neither invalid nor degenerate (the keys the host sorts for the duplicate rule).
// itermvs_mesh_simplify_clusters: one launch, one thread per position of the key-sorted vertices; the thread at the head of a run
//   of equal cluster numbers walks the run's members and then the cluster's segment of the sorted (cluster, face) pairs, serially
//   and in the written order, solves the 3x3 system and writes the representative's record.  Serial on purpose: the order of the
//   sums IS the result, a cell of a few voxels has tens of members, and no thread waits for another.
// itermvs_mesh_simplify_emit: the pattern of tsdf.hip and mesh_components.hip from wave_ops.hpp, no atomics: a memset of the marks,
//   mark (the head of every run of equal sorted triples survives and marks its three clusters with plain byte stores of 1), per-256
//   count of the clusters, per-256 count of the faces, ONE workgroup scans both count rows and writes the totals, vertex scatter
//   (keeps every referenced cluster's new index), face scatter.
// Every index that comes out of a buffer (a face's vertex, a sorted position's vertex, cluster, face) is compared with its range
// before it is used as an address: arrays that do not describe this mesh give a wrong mesh, never an access outside the buffers.
#include "cloud_grid.hpp"
#include "wave_ops.hpp"

namespace itermvs {

constexpr int kSimBlock = 256;
constexpr int kSimWaves = kSimBlock / 64;
constexpr int kSimScanBlock = 1024;
constexpr int kSimMinRecord = 12, kSimMaxRecord = 64, kSimColourRecord = 15;
constexpr int32_t kNoCluster = 0x7fffffff;
constexpr int64_t kSimMaxFaces = kFlatInt32 / 3;             // the 3 * NF pairs are indexed in an int32

__device__ __forceinline__ bool sim_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t nv, int32_t& a, int32_t& b, int32_t& c) {
    const int32_t* t = faces + (size_t)f * 3;
    a = t[0]; b = t[1]; c = t[2];
    return (uint32_t)a < nv && (uint32_t)b < nv && (uint32_t)c < nv;
}

// records are unpadded: a coordinate is read and written byte by byte
__device__ __forceinline__ double sim_coord(const uint8_t* __restrict__ p) {
    const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return (double)__uint_as_float(u);
}

__device__ __forceinline__ void sim_store(uint8_t* __restrict__ p, float v) {
    const uint32_t u = __float_as_uint(v);
    p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); p[2] = (uint8_t)(u >> 16); p[3] = (uint8_t)(u >> 24);
}

// ---- corners ----

__global__ void __launch_bounds__(kSimBlock) sim_corners_kernel(const int32_t* __restrict__ faces, uint32_t nf, uint32_t nv,
                                                                const int32_t* __restrict__ cluster, int32_t* __restrict__ pair,
                                                                long long* __restrict__ key_hi, int32_t* __restrict__ key_lo) {
    const uint32_t f = blockIdx.x * kSimBlock + threadIdx.x;
    if (f >= nf) return;
    int32_t a, b, c;
    bool ok = sim_face(faces, f, nv, a, b, c);
    const int32_t ca = ok ? cluster[a] : -1, cb = ok ? cluster[b] : -1, cc = ok ? cluster[c] : -1;
    ok = ok && (uint32_t)ca < nv && (uint32_t)cb < nv && (uint32_t)cc < nv;      // -1: the vertex is not valid
    int32_t* p = pair + (size_t)f * 3;
    p[0] = ok ? ca : kNoCluster;
    p[1] = ok ? cb : kNoCluster;
    p[2] = ok ? cc : kNoCluster;
    const bool alive = ok && ca != cb && cb != cc && ca != cc;
    int32_t c0 = ca, c1 = cb, c2 = cc;                       // the rotation that starts at the smallest (unique: all three differ)
    if (cb < ca && cb < cc) { c0 = cb; c1 = cc; c2 = ca; }
    else if (cc < ca && cc < cb) { c0 = cc; c1 = ca; c2 = cb; }
    key_hi[f] = alive ? (long long)(((unsigned long long)(uint32_t)c0 << 32) | (uint32_t)c1) : kNoKey;
    key_lo[f] = alive ? c2 : kNoCluster;
}

// ---- clusters ----

// first position in sorted[0 : n) whose value is >= want; n < 2^31, so 32 halvings always finish
__device__ __forceinline__ uint32_t sim_lower_bound(const int32_t* __restrict__ sorted, uint32_t n, int32_t want) {
    uint32_t lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double sim_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(kSimBlock) sim_clusters_kernel(const uint8_t* __restrict__ vertices, uint32_t nv, uint32_t rec,
                                                                 const int32_t* __restrict__ faces, uint32_t nf,
                                                                 const long long* __restrict__ keys, const long long* __restrict__ perm,
                                                                 const int32_t* __restrict__ cl, const int32_t* __restrict__ pair,
                                                                 const int32_t* __restrict__ pair_face, CloudGrid g,
                                                                 uint8_t* __restrict__ reps) {
    const uint32_t i = blockIdx.x * kSimBlock + threadIdx.x;
    if (i >= nv) return;
    const int32_t c = cl[i];
    if ((uint32_t)c >= nv || (i > 0 && cl[i - 1] == c)) return;          // not a valid vertex, or not the head of its run
    const long long key = keys[i];
    if (key < 0 || key == kNoKey) return;
    uint8_t* out = reps + (size_t)c * rec;
    // the members, in sorted order = ascending vertex index: sums from 0.0, integer colour sums, the lowest member
    double sx = 0.0, sy = 0.0, sz = 0.0;
    uint32_t red = 0, green = 0, blue = 0, m = 0;
    const uint8_t* lowest = nullptr;
    for (uint32_t j = i; j < nv && cl[j] == c; ++j) {
        const long long v = perm[j];
        if ((unsigned long long)v >= nv) continue;
        const uint8_t* s = vertices + (size_t)v * rec;
        if (!lowest) lowest = s;
        sx += sim_coord(s); sy += sim_coord(s + 4); sz += sim_coord(s + 8);
        if (rec >= kSimColourRecord) { red += s[12]; green += s[13]; blue += s[14]; }
        ++m;
    }
    if (m == 0) return;
    for (uint32_t k = (m == 1 ? 0 : kSimMinRecord); k < rec; ++k) out[k] = lowest[k];      // one member: the record, unchanged
    if (m == 1) return;
    const double dm = (double)m, mx = sx / dm, my = sy / dm, mz = sz / dm;
    if (rec >= kSimColourRecord) {
        out[12] = (uint8_t)rint((double)red / dm);
        out[13] = (uint8_t)rint((double)green / dm);
        out[14] = (uint8_t)rint((double)blue / dm);
    }
    // the quadric of the valid faces with a corner in the cluster, once each, in ascending face index
    double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
    const uint32_t np = nf * 3;
    const uint32_t first = np ? sim_lower_bound(pair, np, c) : 0;
    for (uint32_t e = first; e < np && pair[e] == c; ++e) {
        const int32_t f = pair_face[e];
        if ((uint32_t)f >= nf || (e > first && pair_face[e - 1] == f)) continue;      // a face with two corners here counts once
        int32_t ia, ib, ic;
        if (!sim_face(faces, (uint32_t)f, nv, ia, ib, ic)) continue;
        const uint8_t *pa = vertices + (size_t)ia * rec, *pb = vertices + (size_t)ib * rec, *pc = vertices + (size_t)ic * rec;
        const double ax = sim_coord(pa), ay = sim_coord(pa + 4), az = sim_coord(pa + 8);
        const double ux = sim_coord(pb) - ax, uy = sim_coord(pb + 4) - ay, uz = sim_coord(pb + 8) - az;
        const double vx = sim_coord(pc) - ax, vy = sim_coord(pc + 4) - ay, vz = sim_coord(pc + 8) - az;
        const double nx = (uy * vz) - (uz * vy), ny = (uz * vx) - (ux * vz), nz = (ux * vy) - (uy * vx);
        const double h = ((nx * (ax - mx)) + (ny * (ay - my))) + (nz * (az - mz));
        axx += nx * nx; axy += nx * ny; axz += nx * nz; ayy += ny * ny; ayz += ny * nz; azz += nz * nz;
        rx += nx * h; ry += ny * h; rz += nz * h;
    }
    const double trace = (axx + ayy) + azz, lambda = ITERMVS_MESH_SIMPLIFY_REG * trace;
    const double a00 = axx + lambda, a11 = ayy + lambda, a22 = azz + lambda;
    const double c00 = (a11 * a22) - (ayz * ayz), c01 = (axz * ayz) - (axy * a22), c02 = (axy * ayz) - (axz * a11);
    const double c11 = (a00 * a22) - (axz * axz), c12 = (axy * axz) - (a00 * ayz), c22 = (a00 * a11) - (axy * axy);
    const double det = ((a00 * c00) + (axy * c01)) + (axz * c02);
    double yx = (((c00 * rx) + (c01 * ry)) + (c02 * rz)) / det;
    double yy = (((c01 * rx) + (c11 * ry)) + (c12 * rz)) / det;
    double yz = (((c02 * rx) + (c12 * ry)) + (c22 * rz)) / det;
    if (trace == 0.0 || !isfinite(det) || !(det > 0.0) || !isfinite(yx) || !isfinite(yy) || !isfinite(yz)) yx = yy = yz = 0.0;
    int ix, iy, iz;
    cell_from_key(key, g, ix, iy, iz);
    sim_store(out + 0, (float)sim_clamp(mx + yx, g.ox + (double)ix * g.edge, g.ox + (double)(ix + 1) * g.edge));
    sim_store(out + 4, (float)sim_clamp(my + yy, g.oy + (double)iy * g.edge, g.oy + (double)(iy + 1) * g.edge));
    sim_store(out + 8, (float)sim_clamp(mz + yz, g.oz + (double)iz * g.edge, g.oz + (double)(iz + 1) * g.edge));
}

// ---- emit ----

// per workgroup sum of `on` -> counts[blockIdx.x]; every thread of the workgroup calls it
__device__ __forceinline__ void sim_block_count(bool on, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t part[kSimWaves];
    const uint32_t n = wave_sum_lane0(on ? 1u : 0u);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int wv = 0; wv < kSimWaves; ++wv) s += part[wv];
        counts[blockIdx.x] = s;
    }
}

__device__ __forceinline__ uint32_t sim_block_rank(bool on) {
    uint32_t total;
    const uint32_t below = wave_rank(on, total);
    return block_exclusive<kSimWaves>(below + (on ? 1u : 0u), on ? 1u : 0u);
}

// one thread per position of the sorted triples: the head of a run of equal triples is the run's lowest face (the sorts are stable)
__global__ void __launch_bounds__(kSimBlock) sim_mark_kernel(const long long* __restrict__ key_hi, const int32_t* __restrict__ key_lo,
                                                             const int32_t* __restrict__ order, uint32_t nf, uint32_t nv,
                                                             uint8_t* __restrict__ ref, uint8_t* __restrict__ survive) {
    const uint32_t p = blockIdx.x * kSimBlock + threadIdx.x;
    if (p >= nf) return;
    const long long hi = key_hi[p];
    const int32_t lo = key_lo[p];
    if (hi < 0 || hi == kNoKey || (p > 0 && key_hi[p - 1] == hi && key_lo[p - 1] == lo)) return;
    const int32_t f = order[p];
    const uint32_t c0 = (uint32_t)((unsigned long long)hi >> 32), c1 = (uint32_t)hi, c2 = (uint32_t)lo;
    if ((uint32_t)f >= nf || c0 >= nv || c1 >= nv || c2 >= nv) return;
    survive[f] = 1;
    ref[c0] = 1;
    ref[c1] = 1;
    ref[c2] = 1;
}

__global__ void __launch_bounds__(kSimBlock) sim_count_kernel(const uint8_t* __restrict__ mark, uint32_t n,
                                                              unsigned long long* __restrict__ counts) {
    const uint32_t i = blockIdx.x * kSimBlock + threadIdx.x;
    sim_block_count(i < n && mark[i] != 0, counts);
}

// one workgroup: the cluster row and the face row of counts -> exclusive offsets in place; totals[0] = vertices, totals[1] = faces
__global__ void __launch_bounds__(kSimScanBlock) sim_scan_kernel(unsigned long long* __restrict__ counts, uint32_t nbv, uint32_t nbf,
                                                                 unsigned long long* __restrict__ totals) {
    const auto vertices = block_scan_exclusive_chunked<unsigned long long, kSimScanBlock>(counts, nbv, [](uint32_t) {});
    const auto faces = block_scan_exclusive_chunked<unsigned long long, kSimScanBlock>(counts + nbv, nbf, [](uint32_t) {});
    if (threadIdx.x == 0) { totals[0] = vertices; totals[1] = faces; }
}

__global__ void __launch_bounds__(kSimBlock) sim_vertex_kernel(const uint8_t* __restrict__ reps, uint32_t nv, uint32_t rec,
                                                               const uint8_t* __restrict__ ref, const unsigned long long* __restrict__ offsets,
                                                               uint32_t* __restrict__ rank, uint8_t* __restrict__ out, unsigned long long capacity) {
    const uint32_t c = blockIdx.x * kSimBlock + threadIdx.x;
    const bool on = c < nv && ref[c] != 0;
    const unsigned long long at = offsets[blockIdx.x] + sim_block_rank(on);
    if (!on) return;
    rank[c] = (uint32_t)at;                                // < 2^31: at most nv clusters
    if (at >= capacity) return;                            // the ONLY stores to out are guarded by at < capacity
    const uint8_t* s = reps + (size_t)c * rec;
    uint8_t* o = out + at * rec;
    for (uint32_t i = 0; i < rec; ++i) o[i] = s[i];
}

// the new index of a corner; -1 (instead of a word of the workspace) where the arrays do not describe this mesh
__device__ __forceinline__ int32_t sim_new_index(const int32_t* __restrict__ cluster, int32_t v, uint32_t nv, const uint8_t* __restrict__ ref,
                                                 const uint32_t* __restrict__ rank) {
    const int32_t c = cluster[v];
    return (uint32_t)c < nv && ref[c] != 0 ? (int32_t)rank[c] : -1;
}

__global__ void __launch_bounds__(kSimBlock) sim_face_kernel(const int32_t* __restrict__ faces, uint32_t nf, uint32_t nv,
                                                             const int32_t* __restrict__ cluster, const uint8_t* __restrict__ ref,
                                                             const uint8_t* __restrict__ survive, const unsigned long long* __restrict__ offsets,
                                                             const uint32_t* __restrict__ rank, int32_t* __restrict__ out,
                                                             unsigned long long capacity) {
    const uint32_t f = blockIdx.x * kSimBlock + threadIdx.x;
    int32_t a, b, c;
    const bool on = f < nf && survive[f] != 0 && sim_face(faces, f, nv, a, b, c);
    const unsigned long long at = offsets[blockIdx.x] + sim_block_rank(on);
    if (!on || at >= capacity) return;                     // the ONLY stores to out are guarded by at < capacity
    int32_t* o = out + at * 3;
    o[0] = sim_new_index(cluster, a, nv, ref, rank);
    o[1] = sim_new_index(cluster, b, nv, ref, rank);
    o[2] = sim_new_index(cluster, c, nv, ref, rank);
}

// workspace: counts uint64 [nbv + nbf] | rank uint32 [nv] | ref uint8 [nv] | survive uint8 [nf], rounded up to 8 bytes
struct SimWorkspace {
    int64_t nbv, nbf, rank, ref, survive, bytes;
};
static inline SimWorkspace sim_workspace(int64_t nv, int64_t nf) {
    SimWorkspace w;
    w.nbv = (nv + kSimBlock - 1) / kSimBlock;
    w.nbf = (nf + kSimBlock - 1) / kSimBlock;
    w.rank = (w.nbv + w.nbf) * 8;
    w.ref = w.rank + 4 * nv;
    w.survive = w.ref + nv;
    w.bytes = (w.survive + nf + 7) / 8 * 8;
    return w;
}

static inline int sim_sizes(int32_t nv, int64_t nf) {
    ITERMVS_RETURN_IF(nv < 0 || nf < 0 || nf > kSimMaxFaces, ITERMVS_ERR_DIMS);
    return ITERMVS_OK;
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_mesh_simplify_corners(const int32_t* faces, int64_t NF, int32_t NV, const int32_t* cluster, int32_t* pair_cluster,
                                             int64_t* key_hi, int32_t* key_lo, void* stream) {
    ITERMVS_RETURN_IF((NF != 0 && (!faces || !pair_cluster || !key_hi || !key_lo)) || (NV != 0 && !cluster), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(sim_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    if (NF == 0) return ITERMVS_OK;
    return flat_launch<sim_corners_kernel, kSimBlock>(FlatItems{NF, kFlatInt32}, (hipStream_t)stream, faces, (uint32_t)NF, (uint32_t)NV, cluster,
                                                      pair_cluster, (long long*)key_hi, key_lo);
}

extern "C" int itermvs_mesh_simplify_clusters(const uint8_t* vertices, int32_t NV, int32_t record_bytes, const int32_t* faces, int64_t NF,
                                              const int64_t* keys_sorted, const int64_t* perm, const int32_t* cluster_sorted,
                                              const int32_t* pair_sorted, const int32_t* pair_face, double ox, double oy, double oz,
                                              int32_t nx, int32_t ny, int32_t nz, double cell, uint8_t* reps, void* stream) {
    ITERMVS_RETURN_IF(NV != 0 && (!vertices || !keys_sorted || !perm || !cluster_sorted || !reps), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(NF != 0 && (!faces || !pair_sorted || !pair_face), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(sim_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(record_bytes < kSimMinRecord || record_bytes > kSimMaxRecord, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(!finite_all(ox, oy, oz, cell) || !(cell > 0.0), ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(nx < 1 || ny < 1 || nz < 1 || nx > kMaxCellDim || ny > kMaxCellDim || nz > kMaxCellDim, ITERMVS_ERR_DIMS);
    if (NV == 0) return ITERMVS_OK;
    const CloudGrid g{ox, oy, oz, cell, nx, ny, nz};
    return flat_launch<sim_clusters_kernel, kSimBlock>(FlatItems{(int64_t)NV}, (hipStream_t)stream, vertices, (uint32_t)NV, (uint32_t)record_bytes,
                                                       faces, (uint32_t)NF, (const long long*)keys_sorted, (const long long*)perm, cluster_sorted,
                                                       pair_sorted, pair_face, g, reps);
}

extern "C" int itermvs_mesh_simplify_emit_workspace_bytes(int32_t NV, int64_t NF, int64_t* bytes) {
    ITERMVS_RETURN_IF(!bytes, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(sim_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    *bytes = sim_workspace(NV, NF).bytes;
    return ITERMVS_OK;
}

extern "C" int itermvs_mesh_simplify_emit(const uint8_t* reps, int32_t NV, int32_t record_bytes, const int32_t* faces, int64_t NF,
                                          const int32_t* cluster, const int64_t* key_hi_sorted, const int32_t* key_lo_sorted,
                                          const int32_t* order, uint8_t* out_vertices, int64_t vertex_capacity, int32_t* out_faces,
                                          int64_t face_capacity, uint64_t* totals, uint8_t* workspace, void* stream) {
    ITERMVS_RETURN_IF(!totals || !workspace || (NV != 0 && (!reps || !cluster)), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(NF != 0 && (!faces || !key_hi_sorted || !key_lo_sorted || !order), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF((!out_vertices && vertex_capacity != 0) || (!out_faces && face_capacity != 0), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(sim_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(record_bytes < kSimMinRecord || record_bytes > kSimMaxRecord, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(vertex_capacity < 0 || vertex_capacity > kFlatInt32 || face_capacity < 0, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(((uintptr_t)workspace & 7) != 0, ITERMVS_ERR_ALIGN);
    hipStream_t s = (hipStream_t)stream;
    if (NV == 0 || NF == 0) {                              // no vertex or no face: no face survives, no cluster is referenced
        ITERMVS_RETURN_IF(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s) != hipSuccess, ITERMVS_ERR_LAUNCH);
        return ITERMVS_OK;
    }
    const SimWorkspace w = sim_workspace(NV, NF);
    unsigned long long* counts = (unsigned long long*)workspace;
    uint32_t* rank = (uint32_t*)(workspace + w.rank);
    uint8_t *ref = workspace + w.ref, *survive = workspace + w.survive;
    const FlatItems vs{(int64_t)NV}, fs{NF, kFlatInt32};
    const uint32_t nv = (uint32_t)NV, nf = (uint32_t)NF;
    ITERMVS_RETURN_IF(hipMemsetAsync(ref, 0, (size_t)NV + (size_t)NF, s) != hipSuccess, ITERMVS_ERR_LAUNCH);
    int bad = flat_launch<sim_mark_kernel, kSimBlock>(fs, s, (const long long*)key_hi_sorted, key_lo_sorted, order, nf, nv, ref, survive);
    if (bad == ITERMVS_OK) bad = flat_launch<sim_count_kernel, kSimBlock>(vs, s, (const uint8_t*)ref, nv, counts);
    if (bad == ITERMVS_OK) bad = flat_launch<sim_count_kernel, kSimBlock>(fs, s, (const uint8_t*)survive, nf, counts + w.nbv);
    if (bad != ITERMVS_OK) return bad;
    hipLaunchKernelGGL(sim_scan_kernel, dim3(1), dim3(kSimScanBlock), 0, s, counts, (uint32_t)w.nbv, (uint32_t)w.nbf, (unsigned long long*)totals);
    bad = flat_launch<sim_vertex_kernel, kSimBlock>(vs, s, reps, nv, (uint32_t)record_bytes, (const uint8_t*)ref, (const unsigned long long*)counts,
                                                    rank, out_vertices, (unsigned long long)vertex_capacity);
    if (bad != ITERMVS_OK) return bad;
    return flat_launch<sim_face_kernel, kSimBlock>(fs, s, faces, nf, nv, cluster, (const uint8_t*)ref, (const uint8_t*)survive,
                                                   (const unsigned long long*)(counts + w.nbv), (const uint32_t*)rank, out_faces,
                                                   (unsigned long long)face_capacity);
}
