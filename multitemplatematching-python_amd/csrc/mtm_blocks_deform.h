// Window deformation between the passes of a block-matching call (mtm_match_blocks_passes_deformed, mtm_deform_image;
// DESIGN 5.6.4): the displacement field interpolated from a coarse grid's displacements and the bilinear warp of an
// image by it, as inline functions for the host (mtm_deform_image without a context, the weight tables of a call) and
// the device (deform_image_kernel, mtm_k_deform.hip.h; blocks_deform_record_kernel, mtm_k_blocks.hip.h) - a single source
// for the rule, so that the pixels a test computes on the host are the pixels the kernel writes.  Integers only.
// (MTM.blocks.displacement_field, field_at and deform state the same rule in numpy.)
//
// Coordinates are DOUBLED: pixel x is X2 = 2 x, the centre of a block at x of width w is X2 = 2 x + w - 1, the centre of
// coarse column i (blocks of width wc at stride sx) is Cx_i = 2 i sx + wc - 1.  The field is in Q8 (1/256 pixel).
#pragma once
#include <cstdint>

#include "../../include/mtm_hip.h"
#include "mtm_blocks_predict.h"    // BlockGrid
#include "mtm_templ_stats.h"       // MTM_HOST_DEVICE

namespace mtm {

// The largest |displacement| the field takes: Q8 values, and the products below, then stay far inside int32 / int64.
constexpr long long kDeformMaxDisp = 1ll << 22;

// One axis of n coarse blocks of size wc at stride s: the lower node *i and the weight *a8 (0 .. 256) of node min(*i + 1,
// n - 1) at doubled coordinate X2.  Constant extrapolation outside the hull of the centres; n == 1: node 0 alone.
MTM_HOST_DEVICE inline void deform_axis_inl(int n, int s, int wc, long long X2, int* i, int* a8) {
    if (n <= 1) {
        *i = 0;
        *a8 = 0;
        return;
    }
    const long long s2 = 2ll * s, num = X2 - (wc - 1);
    long long q = num > 0 ? num / s2 : 0;           // (floor, clamped at 0: a negative quotient is 0 either way)
    q = q < n - 2 ? q : n - 2;
    long long a = X2 - (2ll * q * s + wc - 1);
    a = a < 0 ? 0 : (a > s2 ? s2 : a);
    *i = (int)q;
    *a8 = (int)((256 * a + s) / s2);
}

// (i, a8) of an axis packed into one word of a call's weight tables: i << 9 | a8 (i < 2^23).
MTM_HOST_DEVICE inline uint32_t deform_pack_inl(int i, int a8) { return ((uint32_t)i << 9) | (uint32_t)a8; }

// One component of the field from its four nodes and the weights: an arithmetic shift, a floor.  The weights' products
// (at most 2^16) are formed in 32 bits first, so that each node costs one 32 x 32 -> 64-bit multiply-add.
MTM_HOST_DEVICE inline long long deform_field_inl(int32_t d00, int32_t d01, int32_t d10, int32_t d11, int ax, int ay) {
    const int32_t w00 = (256 - ax) * (256 - ay), w01 = ax * (256 - ay), w10 = (256 - ax) * ay, w11 = ax * ay;
    return ((long long)d00 * w00 + (long long)d01 * w01 + (long long)d10 * w10 + (long long)d11 * w11 + 128) >> 8;
}

// The field (Q8) of the coarse grid g with displacements d - d[2 k], d[2 k + 1] = (dx, dy) of block k in row-major order -
// at the doubled point (X2, Y2).
MTM_HOST_DEVICE inline void deform_field_at_inl(const BlockGrid& g, const int32_t* d, long long X2, long long Y2, long long* fx,
                                                long long* fy) {
    int i, ax, j, ay;
    deform_axis_inl(g.nx, g.sx, g.bw, X2, &i, &ax);
    deform_axis_inl(g.ny, g.sy, g.bh, Y2, &j, &ay);
    const int i1 = i + 1 < g.nx ? i + 1 : g.nx - 1, j1 = j + 1 < g.ny ? j + 1 : g.ny - 1;
    const int32_t* p00 = d + 2 * ((long long)j * g.nx + i);
    const int32_t* p01 = d + 2 * ((long long)j * g.nx + i1);
    const int32_t* p10 = d + 2 * ((long long)j1 * g.nx + i);
    const int32_t* p11 = d + 2 * ((long long)j1 * g.nx + i1);
    *fx = deform_field_inl(p00[0], p01[0], p10[0], p11[0], ax, ay);
    *fy = deform_field_inl(p00[1], p01[1], p10[1], p11[1], ax, ay);
}

// The largest |Q8 node| of the sub-pixel fields below (mtm_deform_image_q8, steer = 1): the same 2^22 pixels.
constexpr long long kDeformMaxDispQ8 = kDeformMaxDisp << 8;

// deform_field_inl for nodes that are themselves in Q8 (1/256 pixel; |s| <= 2^30, so every product stays below 2^46):
// the weights' 2^16 is divided out in one arithmetic shift, rounded half up.  For s = 256 d this is deform_field_inl(d),
// bit for bit: (256 sum + 32768) >> 16 = (sum + 128) >> 8.
MTM_HOST_DEVICE inline long long deform_field_q8_inl(int32_t s00, int32_t s01, int32_t s10, int32_t s11, int ax, int ay) {
    const int32_t w00 = (256 - ax) * (256 - ay), w01 = ax * (256 - ay), w10 = (256 - ax) * ay, w11 = ax * ay;
    return ((long long)s00 * w00 + (long long)s01 * w01 + (long long)s10 * w10 + (long long)s11 * w11 + 32768) >> 16;
}

// The field of either kind of node: Q8 nodes (deform_field_q8_inl) or whole pixels (deform_field_inl).
template <bool Q8>
MTM_HOST_DEVICE inline long long deform_field_of_inl(int32_t d00, int32_t d01, int32_t d10, int32_t d11, int ax, int ay) {
    if constexpr (Q8) return deform_field_q8_inl(d00, d01, d10, d11, ax, ay);
    else return deform_field_inl(d00, d01, d10, d11, ax, ay);
}

// deform_field_at_inl for either kind of node.
template <bool Q8>
MTM_HOST_DEVICE inline void deform_field_at_of_inl(const BlockGrid& g, const int32_t* d, long long X2, long long Y2, long long* fx,
                                                   long long* fy) {
    if constexpr (!Q8) {
        deform_field_at_inl(g, d, X2, Y2, fx, fy);
    } else {
        int i, ax, j, ay;
        deform_axis_inl(g.nx, g.sx, g.bw, X2, &i, &ax);
        deform_axis_inl(g.ny, g.sy, g.bh, Y2, &j, &ay);
        const int i1 = i + 1 < g.nx ? i + 1 : g.nx - 1, j1 = j + 1 < g.ny ? j + 1 : g.ny - 1;
        const int32_t* p00 = d + 2 * ((long long)j * g.nx + i);
        const int32_t* p01 = d + 2 * ((long long)j * g.nx + i1);
        const int32_t* p10 = d + 2 * ((long long)j1 * g.nx + i);
        const int32_t* p11 = d + 2 * ((long long)j1 * g.nx + i1);
        *fx = deform_field_q8_inl(p00[0], p01[0], p10[0], p11[0], ax, ay);
        *fy = deform_field_q8_inl(p00[1], p01[1], p10[1], p11[1], ax, ay);
    }
}

// Along one axis of n pixels: the sample of output pixel x under field f (Q8) - the lower source pixel *x0, its
// neighbour *x1 = min(*x0 + 1, n - 1) and the weight *w8 (0 .. 255) of the neighbour.  Replicated edges.
MTM_HOST_DEVICE inline void deform_sample_inl(int x, long long f, int n, int* x0, int* x1, int* w8) {
    long long X = 256ll * x + f;
    const long long top = 256ll * (n - 1);
    X = X < 0 ? 0 : (X > top ? top : X);
    *x0 = (int)(X >> 8);
    *w8 = (int)(X & 255);
    *x1 = *x0 + 1 < n ? *x0 + 1 : n - 1;
}

// The bilinear blend of four pixel values (uint8 or uint16) with weights fx, fy: rounded to nearest, half up.  The four
// weights sum to 2^16, so the sum stays below 65535 * 65536 + 32768 < 2^32: 32-bit arithmetic is exact.
MTM_HOST_DEVICE inline uint32_t deform_blend_inl(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, int fx, int fy) {
    const uint32_t w00 = (uint32_t)((256 - fx) * (256 - fy)), w01 = (uint32_t)(fx * (256 - fy));
    const uint32_t w10 = (uint32_t)((256 - fx) * fy), w11 = (uint32_t)(fx * fy);
    return (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + 32768u) >> 16;
}

// The integer part of a Q8 field value, rounded half towards +infinity: what a deformed pass adds to its records.
MTM_HOST_DEVICE inline long long deform_round_inl(long long q8) { return (q8 + 128) >> 8; }

}  // namespace mtm
