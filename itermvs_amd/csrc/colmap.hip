// The two device stages of the COLMAP converter (colmap_input.py of the reference): the depth range of every image and the
// view-selection score of every image pair, from the sparse model's observation lists.
//
// Observations are CSR: offsets[V + 1] (int64) into point[] (int32, dense point index or -1, in file order).  An entry outside
// [0, P) is treated like -1 by both kernels, so no list content can make them read outside xyz.
//
// itermvs_view_scores (colmap_input.py:336-364).  The reference's `[it for it in id_i if it in id_j]` is a membership test of
// every entry of the LOWER-indexed image's list (in list order, with multiplicity) against the other image's list.  Here a
// workgroup owns image j and a slice of the images i < j.  It builds j's membership bitmap over a chunk of point indices
// (chunk_bits of them, at most kMaxChunkBits) in LDS (integer atomicOr: the result does not depend on order), then each of its waves streams the list of one image i
// past the bitmap: lane t takes entries t, t + 64, ... in that order, the 64 partial sums meet in a fixed shuffle tree,
// lane 0 stores score[i][j] and score[j][i].  Every pair belongs to exactly one wave, so there is nothing to combine between
// workgroups: no floating-point atomics, and the bits do not depend on scheduling.  Models with more points than one bitmap
// holds (kMaxChunkBits) are walked chunk by chunk inside the same workgroup; the owning lane adds the chunks' sums in ascending
// chunk order.
//
// itermvs_depth_ranges (colmap_input.py:319-333): one workgroup per image selects the two order statistics
// zs[int(len * .01)] and zs[int(len * .99)] of z = ((e0 x + e1 y) + e2 z) + e3 by an 8-pass, 8-bit radix select on
// order-preserving 64-bit keys (LDS histograms, integer atomics); z is recomputed in every pass, so no scratch memory is needed
// and the selected key IS one of the z values, bit for bit.
//
// Not reproduced from the reference: a cosine that rounds above 1 makes np.arccos return NaN there (the cosine is clamped to
// [-1, 1] here), and an image without a valid observation raises IndexError there (its range is NaN here; the host raises).
#include <math.h>

#include "wave_ops.hpp"

namespace itermvs {

constexpr int kScoreBlock = 256;                       // 4 waves, each owns one image i at a time
constexpr int kScoreWaves = kScoreBlock / 64;
constexpr int kMaxChunkBits = 64 * 1024 * 8;           // 64 KB of LDS: 524288 points per bitmap chunk, two workgroups per CU
constexpr int kRangeBlock = 256;

__device__ __forceinline__ double score_term(const double* __restrict__ xyz, int p, double cix, double ciy, double ciz,
                                             double cjx, double cjy, double cjz, double theta0, double den1, double den2) {
    const double px = xyz[(size_t)p * 3 + 0], py = xyz[(size_t)p * 3 + 1], pz = xyz[(size_t)p * 3 + 2];
    const double ax = cix - px, ay = ciy - py, az = ciz - pz;
    const double bx = cjx - px, by = cjy - py, bz = cjz - pz;
    const double dot = (ax * bx + ay * by) + az * bz;
    const double na = sqrt((ax * ax + ay * ay) + az * az), nb = sqrt((bx * bx + by * by) + bz * bz);
    double c = dot / na / nb;                                                          // colmap_input.py:348-349
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);                                         // NaN passes through
    const double theta = (180.0 / 3.141592653589793) * acos(c);
    const double d = theta - theta0;
    return exp(-d * d / (theta <= theta0 ? den1 : den2));                              // den = 2 sigma^2 (:350-351)
}

// grid (V, split): workgroup (j, s) owns the pairs (i, j) with i < j and (i / kScoreWaves) % split == s
__global__ void __launch_bounds__(kScoreBlock) view_scores_kernel(const int64_t* __restrict__ offsets,
                                                                  const int32_t* __restrict__ point,
                                                                  const double* __restrict__ xyz,
                                                                  const double* __restrict__ centre, int V, int P,
                                                                  int chunk_bits, double theta0, double den1, double den2,
                                                                  double* __restrict__ score) {
    extern __shared__ uint32_t bitmap[];                   // chunk_bits / 32 words
    const int j = blockIdx.x, split = gridDim.y, s = blockIdx.y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (s == 0 && threadIdx.x == 0) score[(size_t)j * V + j] = 0.0;
    if (j == 0) return;                                    // uniform: image 0 has no lower-indexed partner
    const int64_t jb = offsets[j], je = offsets[j + 1];
    const double cjx = centre[j * 3 + 0], cjy = centre[j * 3 + 1], cjz = centre[j * 3 + 2];
    const int words = chunk_bits >> 5;
    for (long long base = 0; base < P; base += chunk_bits) {
        if (base) __syncthreads();                         // the previous chunk's readers are done
        for (int w = threadIdx.x; w < words; w += kScoreBlock) bitmap[w] = 0u;
        __syncthreads();
        for (int64_t e = jb + threadIdx.x; e < je; e += kScoreBlock) {
            const int p = point[e];
            const long long rel = (long long)p - base;
            if (p >= 0 && p < P && rel >= 0 && rel < chunk_bits) atomicOr(&bitmap[rel >> 5], 1u << (rel & 31));
        }
        __syncthreads();
        for (int i = s * kScoreWaves + wv; i < j; i += split * kScoreWaves) {
            const int64_t ib = offsets[i], ie = offsets[i + 1];
            const double cix = centre[i * 3 + 0], ciy = centre[i * 3 + 1], ciz = centre[i * 3 + 2];
            double acc = 0.0;
            for (int64_t e = ib + lane; e < ie; e += 64) {
                const int p = point[e];
                const long long rel = (long long)p - base;
                if (p >= 0 && p < P && rel >= 0 && rel < chunk_bits && ((bitmap[rel >> 5] >> (rel & 31)) & 1u))
                    acc = acc + score_term(xyz, p, cix, ciy, ciz, cjx, cjy, cjz, theta0, den1, den2);
            }
            acc = wave_sum_lane0(acc);
            if (lane == 0) {                               // the same lane of the same wave owns the pair in every chunk
                const size_t a = (size_t)i * V + j, b = (size_t)j * V + i;
                const double total = base ? score[a] + acc : acc;
                score[a] = total;
                score[b] = total;
            }
        }
    }
}

__device__ __forceinline__ unsigned long long order_key(double z) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(z);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(kRangeBlock) depth_ranges_kernel(const int64_t* __restrict__ offsets,
                                                                   const int32_t* __restrict__ point,
                                                                   const double* __restrict__ xyz,
                                                                   const double* __restrict__ ext_row2, int P,
                                                                   double* __restrict__ range) {
    __shared__ unsigned int hist[2][256];
    __shared__ unsigned long long prefix[2];
    __shared__ long long rank[2];                          // order statistic still to find inside the prefix's bucket
    __shared__ int empty;
    const int v = blockIdx.x;
    const int64_t b = offsets[v], e = offsets[v + 1];
    const double e0 = ext_row2[v * 4 + 0], e1 = ext_row2[v * 4 + 1], e2 = ext_row2[v * 4 + 2], e3 = ext_row2[v * 4 + 3];
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int t = threadIdx.x; t < 512; t += kRangeBlock) hist[t >> 8][t & 255] = 0u;
        __syncthreads();
        const unsigned long long p0 = pass ? prefix[0] : 0ull, p1 = pass ? prefix[1] : 0ull;
        for (int64_t o = b + threadIdx.x; o < e; o += kRangeBlock) {
            const int p = point[o];
            if (p < 0 || p >= P) continue;
            const double x = xyz[(size_t)p * 3 + 0], y = xyz[(size_t)p * 3 + 1], z = xyz[(size_t)p * 3 + 2];
            const unsigned long long k = order_key(((e0 * x + e1 * y) + e2 * z) + e3);
            const unsigned bin = (unsigned)(k >> shift) & 255u;
            if (pass == 0 || (k >> (shift + 8)) == p0) atomicAdd(&hist[0][bin], 1u);
            if (pass == 0 || (k >> (shift + 8)) == p1) atomicAdd(&hist[1][bin], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const int t = threadIdx.x;
            long long want;
            if (pass == 0) {
                long long len = 0;
                for (int k = 0; k < 256; ++k) len += hist[t][k];
                want = (long long)((double)len * (t == 0 ? .01 : .99));                 // int(len(zs) * .01), int(len(zs) * .99)
                if (t == 0) empty = len == 0;
            } else {
                want = rank[t];
            }
            int bin = 0;
            for (; bin < 255 && want >= (long long)hist[t][bin]; ++bin) want -= hist[t][bin];
            rank[t] = want;
            prefix[t] = pass == 0 ? (unsigned long long)bin : ((prefix[t] << 8) | (unsigned long long)bin);
        }
        __syncthreads();
    }
    if (threadIdx.x < 2)
        range[v * 2 + threadIdx.x] = empty ? __longlong_as_double(0x7ff8000000000000LL) : key_value(prefix[threadIdx.x]);
}

}  // namespace itermvs

using namespace itermvs;

extern "C" int itermvs_view_scores(const int64_t* offsets, const int32_t* point, const double* xyz, const double* centre,
                                   int32_t V, int32_t P, double theta0, double sigma1, double sigma2, double* score,
                                   void* stream) {
    ITERMVS_RETURN_IF(!offsets || !point || !xyz || !centre || !score, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(V < 1 || P < 1, ITERMVS_ERR_DIMS);
    const int chunk_bits = P >= kMaxChunkBits ? kMaxChunkBits : (P + 31) / 32 * 32;
    // enough workgroups for every CU at small V; one wave per pair bounds the useful split
    int split = (4 * itermvs_num_cus() + V - 1) / V;
    const int most = (V - 1 + kScoreWaves - 1) / kScoreWaves;
    split = split > most ? most : split;
    split = split < 1 ? 1 : split;
    hipLaunchKernelGGL(view_scores_kernel, dim3(V, split), dim3(kScoreBlock), (size_t)chunk_bits / 8, (hipStream_t)stream,
                       offsets, point, xyz, centre, V, P, chunk_bits, theta0, 2.0 * (sigma1 * sigma1),
                       2.0 * (sigma2 * sigma2), score);
    return itermvs_launch_status();
}

extern "C" int itermvs_depth_ranges(const int64_t* offsets, const int32_t* point, const double* xyz, const double* ext_row2,
                                    int32_t V, int32_t P, double* range, void* stream) {
    ITERMVS_RETURN_IF(!offsets || !point || !xyz || !ext_row2 || !range, ITERMVS_ERR_NULL);
    ITERMVS_RETURN_IF(V < 1 || P < 1, ITERMVS_ERR_DIMS);
    hipLaunchKernelGGL(depth_ranges_kernel, dim3(V), dim3(kRangeBlock), 0, (hipStream_t)stream, offsets, point, xyz,
                       ext_row2, P, range);
    return itermvs_launch_status();
}
