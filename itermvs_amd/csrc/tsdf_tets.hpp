// Marching tetrahedra over a cell of 8 voxel centres, the two tables that the kernels of tsdf.hip and the host (itermvs_tsdf_tet_corners,
// itermvs_tsdf_tet_case; tests/test_tsdf_cpu.py) both read.  No HIP call, no device state.
//   Cube corners: bit 0 = +x, bit 1 = +y, bit 2 = +z, so corner 0 is the cell's own voxel and corner 7 its +xyz neighbour.
//   Tetrahedra: the six of the Freudenthal (Kuhn) triangulation, one per order (a, b, c) of the axes in lexicographic order xyz, xzy,
//     yxz, yzx, zxy, zyx: the chain 0, a, a|b, 7.  All share the diagonal 0-7, and every face diagonal runs from the lower to the upper
//     corner, so the two cells on a face cut it alike.  For the odd orders the two middle corners are exchanged: every row below is
//     positively oriented, det(q1 - q0, q2 - q0, q3 - q0) > 0.  Any two corners of a row are nested as bit sets: each of the 19 edges
//     goes from a corner lo to a corner hi = lo | d, d in 1..7, and belongs to the voxel at lo, direction d.
//   Cases: bit p of the mask = local corner p is inside (value < 0).  Written once for a positively oriented tetrahedron:
//     one corner i inside, (j, k, l) the others ascending, j and k exchanged if (i, j, k, l) is an odd permutation:
//         triangle (ij, ik, il); with i the one corner OUTSIDE: (ij, il, ik);
//     two inside i < j, two outside k < l, exchanged if (i, j, k, l) is odd: triangles (ik, il, jl) and (ik, jl, jk).
//     Seen from the outside (the positive side) every triangle is counter-clockwise.  An edge is stored as (lower, upper) local corner.
//   Directions: a vertex belongs to (voxel, direction); directions are numbered +x, +y, +z, +xy, +xz, +yz, +xyz = 0..6.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ITERMVS_HD __host__ __device__
#else
#define ITERMVS_HD
#endif

namespace itermvs {

struct TetCase { uint8_t n; uint8_t edge[12]; };      // n triangles; triangle t, vertex v: local corners edge[6t + 2v], edge[6t + 2v + 1]

constexpr int kTsdfDirs = 7;

ITERMVS_HD inline int tsdf_tet_corner(int tet, int p) {
    constexpr uint8_t k[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
    return k[tet][p];
}

ITERMVS_HD inline TetCase tsdf_tet_case(int mask) {
    constexpr TetCase k[16] = {
        {0, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},   // 0000
        {1, {0, 1, 0, 2, 0, 3, 0, 0, 0, 0, 0, 0}},   // 0001
        {1, {1, 2, 0, 1, 1, 3, 0, 0, 0, 0, 0, 0}},   // 0010
        {2, {0, 2, 0, 3, 1, 3, 0, 2, 1, 3, 1, 2}},   // 0011
        {1, {0, 2, 1, 2, 2, 3, 0, 0, 0, 0, 0, 0}},   // 0100
        {2, {0, 3, 0, 1, 1, 2, 0, 3, 1, 2, 2, 3}},   // 0101
        {2, {0, 1, 1, 3, 2, 3, 0, 1, 2, 3, 0, 2}},   // 0110
        {1, {1, 3, 2, 3, 0, 3, 0, 0, 0, 0, 0, 0}},   // 0111
        {1, {1, 3, 0, 3, 2, 3, 0, 0, 0, 0, 0, 0}},   // 1000
        {2, {0, 1, 0, 2, 2, 3, 0, 1, 2, 3, 1, 3}},   // 1001
        {2, {1, 2, 0, 1, 0, 3, 1, 2, 0, 3, 2, 3}},   // 1010
        {1, {0, 2, 2, 3, 1, 2, 0, 0, 0, 0, 0, 0}},   // 1011
        {2, {0, 2, 1, 2, 1, 3, 0, 2, 1, 3, 0, 3}},   // 1100
        {1, {1, 2, 1, 3, 0, 1, 0, 0, 0, 0, 0, 0}},   // 1101
        {1, {0, 1, 0, 3, 0, 2, 0, 0, 0, 0, 0, 0}},   // 1110
        {0, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}},   // 1111
    };
    return k[mask];
}

// triangles of a tetrahedron with this mask: 0, 1, 2 by the number of inside corners 0 | 4, 1 | 3, 2
ITERMVS_HD inline int tsdf_tet_triangles(int mask) { return (0x0112122112212110ull >> (4 * mask)) & 15; }

// direction number 0..6 of the corner difference d = hi ^ lo in 1..7 (+x +y +z +xy +xz +yz +xyz), and back
ITERMVS_HD inline int tsdf_dir_of_bits(int d) { return (0x65423100 >> (4 * d)) & 7; }
ITERMVS_HD inline int tsdf_bits_of_dir(int dir) { return (0x7653421 >> (4 * dir)) & 7; }

// local mask of tetrahedron `tet` from the cell's 8-bit inside mask
ITERMVS_HD inline int tsdf_tet_mask(int tet, int cube) {
    int m = 0;
    for (int p = 0; p < 4; ++p) m |= ((cube >> tsdf_tet_corner(tet, p)) & 1) << p;
    return m;
}

}  // namespace itermvs
