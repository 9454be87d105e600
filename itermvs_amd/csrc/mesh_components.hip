// Connected components of an indexed triangle mesh and the order-preserving compaction of the components worth keeping (eval.py
// --mesh_min_component / --mesh_component_share, clean_mesh.py; no counterpart in the reference).  The definition of both entry
// points is in include/itermvs_hip.h; the numpy restatement is tests/mesh_components_reference.py.
// itermvs_mesh_components: a memset of the totals and five launches on the stream, 256 items per workgroup; `label` is the parent
//   array of a lock-free union-find while they run:
//   init    : label[v] = v, face_count[v] = 0;
//   hook    : one thread per valid face unites (a, b) and (a, c).  unite() finds both roots and hangs the LARGER root under the
//             smaller with ONE compare-and-swap at the larger root (expected value: the root itself);
//   flatten : label[v] = the root of v.  A launch of its own: the hooks are complete and visible, the roots are final;
//   count   : one thread per valid face adds 1 to face_count[label[a]], one atomic per distinct root of a wave;
//   totals  : one thread per vertex; per workgroup one atomicAdd (components with a face, valid faces) and one atomicMax (largest).
//   What holds at every moment of the hook launch: label[v] <= v; label[v] == v iff v is a root; a vertex that has stopped being
//   a root never becomes one again (the only store that changes a root is the CAS, and it expects the root itself); every value
//   label[v] ever held is a vertex of v's set.  The one other store, the path halving atomicMin(label[v], an ancestor of v), keeps
//   all of that and only ever lowers label[v].  Hence
//   * the root a set ends with is its smallest vertex index: every vertex starts as a root and a union keeps the smaller root;
//   * every loop ends by construction.  find() replaces v by label[v] < v until label[v] == v: at most v steps.  unite() retries
//     only after its CAS at root `hi` failed, i.e. after another thread lowered label[hi]; the retry starts from that lower value,
//     so the pair of roots it finds has a strictly smaller sum than the pair before: at most hi + lo retries, and some thread's CAS
//     succeeded each time.  No thread waits for a value that another thread has yet to write: no flag, no spin, no workgroup waits
//     on a workgroup.
//   * reads of label inside the hook launch are relaxed agent-scope atomic loads, so they come from memory and not from a
//     compute unit's L1 that another unit's CAS never refreshes.  A stale (older, larger) value would still be an ancestor and
//     the CAS, the one authority, would still refuse a wrong hook; the atomic load spares the walk that such a value costs.
//   The outputs are a function of the inputs alone: the partition, its minima, and integer sums and maxima, whatever the order
//   in which the atomics arrive.
// itermvs_mesh_keep: the pattern of tsdf.hip from wave_ops.hpp, no atomics: mark + per-256 count (vertices), per-256 count (faces),
//   ONE workgroup scans both count rows and writes the totals, vertex scatter (keeps every kept vertex's new index), face scatter.
#include "flat_launch.hpp"
#include "wave_ops.hpp"

namespace itermvs {

constexpr int kMeshBlock = 256;
constexpr int kMeshWaves = kMeshBlock / 64;
constexpr int kMeshScanBlock = 1024;
constexpr int kMeshMaxRecord = 64;

__device__ __forceinline__ int32_t cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v, halving the path on the way: label[x] = min(label[x], its grandparent)
__device__ __forceinline__ int32_t cc_find(int32_t* __restrict__ label, int32_t v) {
    int32_t p = cc_load(label + v);
    while (p != v) {                                       // p < v
        const int32_t g = cc_load(label + p);              // g <= p
        if (g == p) return p;
        atomicMin(label + v, g);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void cc_unite(int32_t* __restrict__ label, int32_t x, int32_t y) {
    for (;;) {
        x = cc_find(label, x);
        y = cc_find(label, y);
        if (x == y) return;
        const int32_t hi = x > y ? x : y, lo = x > y ? y : x;
        const int32_t old = atomicCAS(label + hi, hi, lo);
        if (old == hi) return;
        x = old;                                           // < hi: hi was hooked by another thread meanwhile
        y = lo;
    }
}

__device__ __forceinline__ bool mesh_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t nv, int32_t& a, int32_t& b, int32_t& c) {
    const int32_t* t = faces + (size_t)f * 3;
    a = t[0]; b = t[1]; c = t[2];
    return (uint32_t)a < nv && (uint32_t)b < nv && (uint32_t)c < nv;
}

__global__ void __launch_bounds__(kMeshBlock) cc_init_kernel(int32_t* __restrict__ label, int32_t* __restrict__ face_count, uint32_t nv) {
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    if (v >= nv) return;
    label[v] = (int32_t)v;
    face_count[v] = 0;
}

__global__ void __launch_bounds__(kMeshBlock) cc_hook_kernel(const int32_t* __restrict__ faces, uint32_t nf, uint32_t nv, int32_t* __restrict__ label) {
    const uint32_t f = blockIdx.x * kMeshBlock + threadIdx.x;
    int32_t a, b, c;
    if (f >= nf || !mesh_face(faces, f, nv, a, b, c)) return;
    if (b != a) cc_unite(label, a, b);
    if (c != a && c != b) cc_unite(label, a, c);
}

// the roots are final: every value label[v] holds or is given here is an ancestor of v, so plain walks end at the root
__global__ void __launch_bounds__(kMeshBlock) cc_flatten_kernel(int32_t* __restrict__ label, uint32_t nv) {
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    if (v >= nv) return;
    int32_t r = cc_load(label + v);
    for (int32_t p; (p = cc_load(label + r)) != r;) r = p;
    __hip_atomic_store(label + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kMeshBlock) cc_count_kernel(const int32_t* __restrict__ faces, uint32_t nf, uint32_t nv,
                                                              const int32_t* __restrict__ label, int32_t* __restrict__ face_count) {
    const uint32_t f = blockIdx.x * kMeshBlock + threadIdx.x;
    int32_t a, b, c;
    const bool on = f < nf && mesh_face(faces, f, nv, a, b, c);
    const int32_t r = on ? label[a] : -1;
    const int lane = threadIdx.x & 63;
    // the faces of a wave mostly share a root: one add per distinct root.  The loop is uniform; a pass retires >= 1 lane.
    for (unsigned long long left = __ballot(on); left != 0;) {
        const int lead = __ffsll((long long)left) - 1;
        const int32_t r0 = __shfl(r, lead, 64);
        const unsigned long long same = __ballot(on && r == r0);
        if (lane == lead) atomicAdd(face_count + r0, (int32_t)__popcll(same));
        left &= ~same;
    }
}

// totals: components with a face | the largest face_count | valid faces (zeroed by the entry point)
__global__ void __launch_bounds__(kMeshBlock) cc_totals_kernel(const int32_t* __restrict__ face_count, uint32_t nv,
                                                               unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long part[3][kMeshWaves];
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    const unsigned long long c = v < nv ? (unsigned long long)face_count[v] : 0ull;
    const unsigned long long comps = wave_sum_lane0<unsigned long long>(c != 0), sum = wave_sum_lane0(c);
    unsigned long long big = c;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_down(big, d, 64);
        big = o > big ? o : big;
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = comps; part[1][threadIdx.x >> 6] = big; part[2][threadIdx.x >> 6] = sum; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
        for (int wv = 0; wv < kMeshWaves; ++wv) s = threadIdx.x == 1 ? (part[1][wv] > s ? part[1][wv] : s) : s + part[threadIdx.x][wv];
        if (s != 0) {
            if (threadIdx.x == 1) atomicMax(totals + 1, s);
            else atomicAdd(totals + threadIdx.x, s);
        }
    }
}

// ---- keep ----

// per workgroup sum of `on` -> counts[blockIdx.x]; every thread of the workgroup calls it
__device__ __forceinline__ void keep_block_count(bool on, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t part[kMeshWaves];
    const uint32_t n = wave_sum_lane0(on ? 1u : 0u);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int wv = 0; wv < kMeshWaves; ++wv) s += part[wv];
        counts[blockIdx.x] = s;
    }
}

__device__ __forceinline__ uint32_t keep_block_rank(bool on) {
    uint32_t total;
    const uint32_t below = wave_rank(on, total);
    return block_exclusive<kMeshWaves>(below + (on ? 1u : 0u), on ? 1u : 0u);
}

// a label outside [0, nv) (not what itermvs_mesh_components writes) keeps nothing and reads nothing
__global__ void __launch_bounds__(kMeshBlock) keep_mark_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ face_count,
                                                               uint32_t nv, int32_t min_faces, uint8_t* __restrict__ mark,
                                                               unsigned long long* __restrict__ counts) {
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    bool on = false;
    if (v < nv) {
        const int32_t r = label[v];
        on = (uint32_t)r < nv && face_count[r] >= min_faces;
        mark[v] = on ? 1 : 0;
    }
    keep_block_count(on, counts);
}

__device__ __forceinline__ bool keep_face(const int32_t* __restrict__ faces, uint32_t f, uint32_t nf, uint32_t nv,
                                          const uint8_t* __restrict__ mark, int32_t& a, int32_t& b, int32_t& c) {
    return f < nf && mesh_face(faces, f, nv, a, b, c) && mark[a] != 0;
}

__global__ void __launch_bounds__(kMeshBlock) keep_face_count_kernel(const int32_t* __restrict__ faces, uint32_t nf, uint32_t nv,
                                                                     const uint8_t* __restrict__ mark, unsigned long long* __restrict__ counts) {
    int32_t a, b, c;
    keep_block_count(keep_face(faces, blockIdx.x * kMeshBlock + threadIdx.x, nf, nv, mark, a, b, c), counts);
}

// one workgroup: the vertex row and the face row of counts -> exclusive offsets in place; totals[0] = vertices, totals[1] = faces
__global__ void __launch_bounds__(kMeshScanBlock) keep_scan_kernel(unsigned long long* __restrict__ counts, uint32_t nbv, uint32_t nbf,
                                                                   unsigned long long* __restrict__ totals) {
    const auto vertices = block_scan_exclusive_chunked<unsigned long long, kMeshScanBlock>(counts, nbv, [](uint32_t) {});
    const auto faces = block_scan_exclusive_chunked<unsigned long long, kMeshScanBlock>(counts + nbv, nbf, [](uint32_t) {});
    if (threadIdx.x == 0) { totals[0] = vertices; totals[1] = faces; }
}

__global__ void __launch_bounds__(kMeshBlock) keep_vertex_kernel(const uint8_t* __restrict__ vertices, uint32_t nv, uint32_t record_bytes,
                                                                 const uint8_t* __restrict__ mark, const unsigned long long* __restrict__ offsets,
                                                                 uint32_t* __restrict__ rank, uint8_t* __restrict__ out, unsigned long long capacity) {
    const uint32_t v = blockIdx.x * kMeshBlock + threadIdx.x;
    const bool on = v < nv && mark[v] != 0;
    const unsigned long long at = offsets[blockIdx.x] + keep_block_rank(on);
    if (!on) return;
    rank[v] = (uint32_t)at;                                // < 2^31: at most nv vertices are kept
    if (at >= capacity) return;                            // the ONLY stores to out are guarded by at < capacity
    const uint8_t* s = vertices + (size_t)v * record_bytes;
    uint8_t* o = out + at * record_bytes;
    for (uint32_t i = 0; i < record_bytes; ++i) o[i] = s[i];
}

__global__ void __launch_bounds__(kMeshBlock) keep_face_kernel(const int32_t* __restrict__ faces, uint32_t nf, uint32_t nv,
                                                               const uint8_t* __restrict__ mark, const unsigned long long* __restrict__ offsets,
                                                               const uint32_t* __restrict__ rank, int32_t* __restrict__ out,
                                                               unsigned long long capacity) {
    int32_t a, b, c;
    const bool on = keep_face(faces, blockIdx.x * kMeshBlock + threadIdx.x, nf, nv, mark, a, b, c);
    const unsigned long long at = offsets[blockIdx.x] + keep_block_rank(on);
    if (!on || at >= capacity) return;                     // the ONLY stores to out are guarded by at < capacity
    // b and c carry a's label: marked like a.  Labels that do not describe these faces could leave them unmarked: their rank
    // was never written, so they get -1 instead of a word of the workspace
    int32_t* o = out + at * 3;
    o[0] = (int32_t)rank[a];
    o[1] = mark[b] != 0 ? (int32_t)rank[b] : -1;
    o[2] = mark[c] != 0 ? (int32_t)rank[c] : -1;
}

// workspace: counts uint64 [nbv + nbf] | rank uint32 [nv] | mark uint8 [nv], rounded up to 8 bytes
struct KeepWorkspace {
    int64_t nbv, nbf, rank, mark, bytes;
};
static inline KeepWorkspace keep_workspace(int64_t nv, int64_t nf) {
    KeepWorkspace w;
    w.nbv = (nv + kMeshBlock - 1) / kMeshBlock;
    w.nbf = (nf + kMeshBlock - 1) / kMeshBlock;
    w.rank = (w.nbv + w.nbf) * 8;
    w.mark = w.rank + 4 * nv;
    w.bytes = (w.mark + nv + 7) / 8 * 8;
    return w;
}

// the mesh's sizes, by both entry points: nv is an int32 (labels are vertex indices), nf at most 2^31 - 1 (a face_count is an int32)
static inline int mesh_sizes(int32_t nv, int64_t nf) {
    ITERMVS_RETURN_IF(nv < 0 || nf < 0, ITERMVS_ERR_DIMS);
    dim3 grid;
    ITERMVS_RETURN_IF(nf > 0 && flat_grid({nf, kFlatInt32}, kMeshBlock, &grid) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    return ITERMVS_OK;
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_mesh_components(const int32_t* faces, int64_t NF, int32_t NV, int32_t* label, int32_t* face_count, uint64_t* totals,
                                       void* stream) {
    ITERMVS_RETURN_IF(!label || !face_count || !totals || (!faces && NF != 0), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(mesh_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    hipStream_t s = (hipStream_t)stream;
    ITERMVS_RETURN_IF(hipMemsetAsync(totals, 0, 3 * sizeof(uint64_t), s) != hipSuccess, ITERMVS_ERR_LAUNCH);
    if (NV == 0) return ITERMVS_OK;
    const FlatItems vs{(int64_t)NV}, fs{NF, kFlatInt32};
    const uint32_t nv = (uint32_t)NV, nf = (uint32_t)NF;
    int bad = flat_launch<cc_init_kernel, kMeshBlock>(vs, s, label, face_count, nv);
    if (bad == ITERMVS_OK && nf) bad = flat_launch<cc_hook_kernel, kMeshBlock>(fs, s, faces, nf, nv, label);
    if (bad == ITERMVS_OK) bad = flat_launch<cc_flatten_kernel, kMeshBlock>(vs, s, label, nv);
    if (bad == ITERMVS_OK && nf) bad = flat_launch<cc_count_kernel, kMeshBlock>(fs, s, faces, nf, nv, (const int32_t*)label, face_count);
    if (bad != ITERMVS_OK) return bad;
    return flat_launch<cc_totals_kernel, kMeshBlock>(vs, s, (const int32_t*)face_count, nv, (unsigned long long*)totals);
}

extern "C" int itermvs_mesh_keep_workspace_bytes(int32_t NV, int64_t NF, int64_t* bytes) {
    ITERMVS_RETURN_IF(!bytes, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(mesh_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    *bytes = keep_workspace(NV, NF).bytes;
    return ITERMVS_OK;
}

extern "C" int itermvs_mesh_keep(const uint8_t* vertices, int32_t NV, int32_t record_bytes, const int32_t* faces, int64_t NF,
                                 const int32_t* label, const int32_t* face_count, int32_t min_faces, uint8_t* out_vertices,
                                 int64_t vertex_capacity, int32_t* out_faces, int64_t face_capacity, uint64_t* totals, uint8_t* workspace,
                                 void* stream) {
    ITERMVS_RETURN_IF(!label || !face_count || !totals || !workspace || (!vertices && NV != 0) || (!faces && NF != 0), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF((!out_vertices && vertex_capacity != 0) || (!out_faces && face_capacity != 0), ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(mesh_sizes(NV, NF) != ITERMVS_OK, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(record_bytes < 1 || record_bytes > kMeshMaxRecord || min_faces < 1, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(vertex_capacity < 0 || vertex_capacity > kFlatInt32 || face_capacity < 0, ITERMVS_ERR_DIMS);
    ITERMVS_RETURN_IF(((uintptr_t)workspace & 7) != 0, ITERMVS_ERR_ALIGN);
    hipStream_t s = (hipStream_t)stream;
    if (NV == 0) {                                         // no vertex: no face is valid
        ITERMVS_RETURN_IF(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s) != hipSuccess, ITERMVS_ERR_LAUNCH);
        return ITERMVS_OK;
    }
    const KeepWorkspace w = keep_workspace(NV, NF);
    unsigned long long* counts = (unsigned long long*)workspace;
    uint32_t* rank = (uint32_t*)(workspace + w.rank);
    uint8_t* mark = workspace + w.mark;
    const FlatItems vs{(int64_t)NV}, fs{NF, kFlatInt32};
    const uint32_t nv = (uint32_t)NV, nf = (uint32_t)NF;
    int bad = flat_launch<keep_mark_kernel, kMeshBlock>(vs, s, label, face_count, nv, min_faces, mark, counts);
    if (bad == ITERMVS_OK && nf) bad = flat_launch<keep_face_count_kernel, kMeshBlock>(fs, s, faces, nf, nv, (const uint8_t*)mark, counts + w.nbv);
    if (bad != ITERMVS_OK) return bad;
    hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(kMeshScanBlock), 0, s, counts, (uint32_t)w.nbv, (uint32_t)w.nbf, (unsigned long long*)totals);
    bad = flat_launch<keep_vertex_kernel, kMeshBlock>(vs, s, vertices, nv, (uint32_t)record_bytes, (const uint8_t*)mark,
                                                      (const unsigned long long*)counts, rank, out_vertices, (unsigned long long)vertex_capacity);
    if (bad != ITERMVS_OK || !nf) return bad;
    return flat_launch<keep_face_kernel, kMeshBlock>(fs, s, faces, nf, nv, (const uint8_t*)mark, (const unsigned long long*)(counts + w.nbv),
                                                     (const uint32_t*)rank, out_faces, (unsigned long long)face_capacity);
}
