// Window deformation kernels: the bilinear warp of an image in the device layout by the displacement
// field of a coarse grid of blocks (mtm_blocks_deform.h: the rule, shared with the host).  Launched by mtm_blocks.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mtm_blocks_deform.h"
#include "mtm_kernels.h"

namespace mtm {

constexpr int kDeformPx = 8;        // consecutive output pixels per lane: one 8-byte store per plane
constexpr int kDeformLanesX = 32;   // lanes along a row per work-group (256 pixels), 8 rows of them

// What deform_image_kernel reads and writes.  src / dst: byte planes of `pitch` bytes per row (a multiple of 8, at least
// cols + 7), plane c at c * plane; uint16: plane 0 the high bytes, plane 1 the low bytes XOR 0x80 (src_lo / dst_lo).
// disp: the coarse grid's displacements, (dx, dy) of node k = j nx + i at disp[2 k]; colw[x] / roww[y]: deform_pack_inl
// of deform_axis_inl at X2 = 2 x / Y2 = 2 y, colw padded to a multiple of kDeformPx entries.
struct DeformArgs {
    const uint8_t* src;
    const uint8_t* src_lo;
    long long src_plane;
    int src_pitch;
    uint8_t* dst;
    uint8_t* dst_lo;
    long long dst_plane;
    int dst_pitch;
    int rows, cols;
    const int32_t* disp;
    int nx, ny;
    const uint32_t* colw;
    const uint32_t* roww;
};

// One lane per block k < nx ny of grid g: the displacement of the block's record - record position minus block position -
// as a compact (dx, dy) pair, so that the warp's inner loop never touches the 24-byte records.
__global__ __launch_bounds__(256) void deform_disp_kernel(const mtm_hit* __restrict__ recs, BlockGrid g,
                                                          int32_t* __restrict__ disp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= g.nx * g.ny) return;
    const mtm_hit r = recs[k];
    disp[2 * (size_t)k] = r.x - (k % g.nx) * g.sx;
    disp[2 * (size_t)k + 1] = r.y - (k / g.nx) * g.sy;
}

// Grid: (ceil(cols / 256), ceil(rows / 8)) work-groups of 256 lanes, lane t: row 8 blockIdx.y + t / 32, the kDeformPx
// pixels from column 8 (32 blockIdx.x + t % 32).  Per pixel the field from the four nodes around it (deform_field_inl; the
// node values are reloaded only when the column's node changes: a smooth table, cache hits), the sample
// (deform_sample_inl) and per plane four gathered bytes and their blend (deform_blend_inl); the field never reaches
// memory.  Every source index is clamped into rows x cols by deform_sample_inl; a lane whose first pixel lies outside the
// image leaves; the bytes of a lane's pixels right of the image are stored as zero (inside the pitch: pitch >= cols + 7).
// Q8: disp holds Q8 nodes (mtm_deform_image_q8, steer = 1) and the field is deform_field_q8_inl's; else whole pixels.
template <int CH, bool U16, bool Q8 = false>
__global__ __launch_bounds__(256) void deform_image_kernel(DeformArgs a) {
    constexpr int NP = U16 ? 2 : CH;        // byte planes written
    const int x0 = ((int)blockIdx.x * kDeformLanesX + ((int)threadIdx.x & (kDeformLanesX - 1))) * kDeformPx;
    const int y = (int)blockIdx.y * (256 / kDeformLanesX) + ((int)threadIdx.x / kDeformLanesX);
    if (x0 >= a.cols || y >= a.rows) return;
    const uint32_t rw = a.roww[y];
    const int j = (int)(rw >> 9), ay = (int)(rw & 511u);
    const int j1 = j + 1 < a.ny ? j + 1 : a.ny - 1;
    const int32_t* __restrict__ n0 = a.disp + 2 * (size_t)j * a.nx;
    const int32_t* __restrict__ n1 = a.disp + 2 * (size_t)j1 * a.nx;
    uint32_t cw[kDeformPx];
    {
        const uint4 w0 = *reinterpret_cast<const uint4*>(a.colw + x0), w1 = *reinterpret_cast<const uint4*>(a.colw + x0 + 4);
        cw[0] = w0.x; cw[1] = w0.y; cw[2] = w0.z; cw[3] = w0.w;
        cw[4] = w1.x; cw[5] = w1.y; cw[6] = w1.z; cw[7] = w1.w;
    }
    uint32_t out[NP][2];
#pragma unroll
    for (int c = 0; c < NP; ++c) out[c][0] = out[c][1] = 0u;
    int ci = -1;
    int2 d00 = make_int2(0, 0), d01 = d00, d10 = d00, d11 = d00;
#pragma unroll
    for (int p = 0; p < kDeformPx; ++p) {
        const int x = x0 + p;
        if (x < a.cols) {
            const int i = (int)(cw[p] >> 9), ax = (int)(cw[p] & 511u);
            if (i != ci) {
                const int i1 = i + 1 < a.nx ? i + 1 : a.nx - 1;
                d00 = *reinterpret_cast<const int2*>(n0 + 2 * (size_t)i);
                d01 = *reinterpret_cast<const int2*>(n0 + 2 * (size_t)i1);
                d10 = *reinterpret_cast<const int2*>(n1 + 2 * (size_t)i);
                d11 = *reinterpret_cast<const int2*>(n1 + 2 * (size_t)i1);
                ci = i;
            }
            const long long fx = deform_field_of_inl<Q8>(d00.x, d01.x, d10.x, d11.x, ax, ay);
            const long long fy = deform_field_of_inl<Q8>(d00.y, d01.y, d10.y, d11.y, ax, ay);
            int sx0, sx1, wx, sy0, sy1, wy;
            deform_sample_inl(x, fx, a.cols, &sx0, &sx1, &wx);
            deform_sample_inl(y, fy, a.rows, &sy0, &sy1, &wy);
            const size_t r0 = (size_t)sy0 * a.src_pitch, r1 = (size_t)sy1 * a.src_pitch;
            if constexpr (U16) {
                const uint8_t* __restrict__ hi = a.src;
                const uint8_t* __restrict__ lo = a.src_lo;
                const uint32_t v00 = ((uint32_t)hi[r0 + sx0] << 8) | ((uint32_t)lo[r0 + sx0] ^ 0x80u);
                const uint32_t v01 = ((uint32_t)hi[r0 + sx1] << 8) | ((uint32_t)lo[r0 + sx1] ^ 0x80u);
                const uint32_t v10 = ((uint32_t)hi[r1 + sx0] << 8) | ((uint32_t)lo[r1 + sx0] ^ 0x80u);
                const uint32_t v11 = ((uint32_t)hi[r1 + sx1] << 8) | ((uint32_t)lo[r1 + sx1] ^ 0x80u);
                const uint32_t v = deform_blend_inl(v00, v01, v10, v11, wx, wy);
                out[0][p >> 2] |= (v >> 8) << (8 * (p & 3));
                out[1][p >> 2] |= ((v & 255u) ^ 0x80u) << (8 * (p & 3));
            } else {
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const uint8_t* __restrict__ s = a.src + (size_t)c * a.src_plane;
                    const uint32_t v = deform_blend_inl(s[r0 + sx0], s[r0 + sx1], s[r1 + sx0], s[r1 + sx1], wx, wy);
                    out[c][p >> 2] |= v << (8 * (p & 3));
                }
            }
        }
    }
    const size_t o = (size_t)y * a.dst_pitch + (size_t)x0;
    if constexpr (U16) {
        *reinterpret_cast<uint2*>(a.dst + o) = make_uint2(out[0][0], out[0][1]);
        *reinterpret_cast<uint2*>(a.dst_lo + o) = make_uint2(out[1][0], out[1][1]);
    } else {
#pragma unroll
        for (int c = 0; c < CH; ++c)
            *reinterpret_cast<uint2*>(a.dst + (size_t)c * a.dst_plane + o) = make_uint2(out[c][0], out[c][1]);
    }
}

}  // namespace mtm
