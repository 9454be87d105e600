// float32 camera matrix times float64 point, once: the products of fusion.hip, fuse_points.hip and tsdf_integrate_kernel.
// They restate numpy's promotion in the reference (eval.py:162-169, 181-185, 291-294: np.matmul of a float32 matrix with float64
// points upcasts the matrix): k-ascending products and sums, each rounded once.  The build's -ffp-contract=off keeps a * b + c
// two roundings; oracle/fusion_oracle.py is the CPU restatement that the tests compare with, bit for bit.
#pragma once

#include "common.hpp"

namespace itermvs {

// 3x3 @ point
__device__ __forceinline__ void mat3(const float* __restrict__ m, double x, double y, double z, double& ox, double& oy,
                                     double& oz) {
    ox = ((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z;
    oy = ((double)m[3] * x + (double)m[4] * y) + (double)m[5] * z;
    oz = ((double)m[6] * x + (double)m[7] * y) + (double)m[8] * z;
}
// rows 0..2 of a 4x4 @ (point, 1)
__device__ __forceinline__ void mat34(const float* __restrict__ m, double x, double y, double z, double& ox, double& oy,
                                      double& oz) {
    ox = (((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z) + (double)m[3] * 1.0;
    oy = (((double)m[4] * x + (double)m[5] * y) + (double)m[6] * z) + (double)m[7] * 1.0;
    oz = (((double)m[8] * x + (double)m[9] * y) + (double)m[10] * z) + (double)m[11] * 1.0;
}
// the same rows without the translation: what a direction (a normal) takes
__device__ __forceinline__ void rot34(const float* __restrict__ m, double x, double y, double z, double& ox, double& oy,
                                      double& oz) {
    ox = ((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z;
    oy = ((double)m[4] * x + (double)m[5] * y) + (double)m[6] * z;
    oz = ((double)m[8] * x + (double)m[9] * y) + (double)m[10] * z;
}

// a float32 into a record that is not padded: no alignment to rely on, four byte stores (little-endian)
__device__ __forceinline__ void put_f32_bytes(uint8_t* __restrict__ o, float v) {
    const uint32_t b = __float_as_uint(v);
    o[0] = (uint8_t)b; o[1] = (uint8_t)(b >> 8); o[2] = (uint8_t)(b >> 16); o[3] = (uint8_t)(b >> 24);
}

}  // namespace itermvs
