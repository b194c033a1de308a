// The 3 x 3 score neighbourhood of one window from exact integer sums, for the kernels that score nine windows of a point
// (sub_nbhd_kernel, mtm_subpixel.hip; track_nbhd_kernel, mtm_track.hip).  A tile kernel would compute 256 outputs to keep
// nine, so the work is split over the template's pixels instead (split-K): each chunk of kSubR x kSubC template pixels
// gives every thread of a 256-thread work-group one 4-pixel quad, whose products with the nine windows' image pixels -
// staged in LDS as the chunk's (kSubR + 2) x (kSubC + 2) patch - the thread adds to its own nine correlations and window
// sums (v_dot4_u32_u8, kept in uint64: exact).  The work-group's sums are reduced in a fixed order and threads 0 .. 8
// finish window (dy, dx) = (tid / 3 - 1, tid % 3 - 1) with win_score (unmasked) or finish_masked.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "mtm_device_util.hip.h"
#include "mtm_k_window.hip.h"

namespace mtm {

// Kinds of a neighbourhood launch: the image's pixel type and whether its templates carry masks.
enum SubKind { kSubU8 = 0, kSubU8Mask = 1, kSubU16 = 2, kSubF32 = 3, kSubF32Mask = 4 };

constexpr int kSubR = kWinKR, kSubC = kWinKC;       // template chunk: rows x columns (one 4-pixel quad per thread)
constexpr int kSubLdsW = (kSubC + 8) / 4;           // dwords per LDS image row: kSubC + 2 bytes and the alignbyte reach
constexpr int kSubLdsR = kSubR + 2;                 // LDS image rows
static_assert(kSubR * (kSubC / 4) == 256, "one template quad per thread and chunk");

typedef uint32_t SubImageLds[kSubLdsR][kSubLdsW];

// Image rows y0 .. y0 + kSubLdsR - 1, columns x0 .. of one byte plane into LDS (zero outside rows x cols; y0 and x0 may be
// -1); every byte XOR `bias`.
__device__ __forceinline__ void sub_load_image(SubImageLds& Il, const uint8_t* __restrict__ ip, int pitch, int rows, int cols,
                                               int y0, int x0, uint32_t bias, int tid) {
    for (int k = tid; k < kSubLdsR * kSubLdsW; k += 256) {
        const int i = k / kSubLdsW, j = (k % kSubLdsW) * 4;
        const int y = y0 + i;
        uint32_t v = 0u;
        if (y >= 0 && y < rows)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int x = x0 + j + b;
                if (x >= 0 && x < cols) v |= ((uint32_t)ip[(size_t)y * pitch + x] ^ bias) << (8 * b);
            }
        Il[i][j >> 2] = v;
    }
}

// Bytes j + d .. j + d + 3 of LDS row `irow` (j a multiple of 4, d in 0..2), the bytes past the chunk's last template
// column (nj) masked off.
__device__ __forceinline__ uint32_t sub_quad(const uint32_t* irow, int j, int d, int nj) {
    const int q = (j + d) >> 2;
    uint32_t v = __builtin_amdgcn_alignbyte(irow[q + 1], irow[q], d);
    if (nj - j < 4) v &= (1u << (8 * (nj - j))) - 1u;
    return v;
}

// Wave-then-work-group sum of `v` in a fixed order (xor butterfly, then the four waves in order): identical run to run.
// The result is valid in every thread.  `red` holds one slot per wave.
template <typename T>
__device__ __forceinline__ T sub_reduce(T v, T* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    const int tid = threadIdx.x;
    __syncthreads();                    // the previous reduction's reads of `red` are done
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// The neighbourhood of window (px, py) of a `rows` x `cols` image, called by every thread of the work-group (it holds
// barriers): thread tid < 9 gets the score of window (px + tid % 3 - 1, py + tid / 3 - 1), NaN when that window is outside
// the image's map; the other threads' result means nothing.  KIND: kSubU8, kSubU8Mask or kSubU16.
//   ip:    uint8 - plane c at ip + c * plane; uint16 - the high-byte plane, with `lo_b` the low-byte plane XOR 0x80.
//   tp:    the template's bytes, planar [CH][h][w] (masked: T * M); uint16 - the high-byte plane then the low-byte plane.
//   mk:    the mask's bytes 0xFF / 0x00, planar (kSubU8Mask only).
// Pixels outside the image read as zero: `ip` / `lo_b` may point at one frame of a stack of frames, whose neighbours'
// rows are then never read.  Tl / Il / red: the work-group's LDS (Tl[1] for kSubU8Mask and kSubU16, Il[1] for kSubU16).
template <int CH, int KIND>
__device__ __forceinline__ float sub_nbhd_int(WinTemplLds* Tl, SubImageLds* Il, unsigned long long* red,
                                              const uint8_t* __restrict__ ip, long long plane,
                                              const uint8_t* __restrict__ lo_b, int pitch, int rows, int cols,
                                              const uint8_t* __restrict__ tp, const uint8_t* __restrict__ mk,
                                              const TemplDev& T, int px, int py, int method) {
    static_assert(KIND == kSubU8 || KIND == kSubU8Mask || KIND == kSubU16, "integer kinds only");
    constexpr bool kMasked = KIND == kSubU8Mask;
    constexpr int kS1 = kMasked ? 0 : CH;       // window sums per channel (unmasked only)
    constexpr int kT1 = KIND == kSubU8 ? 0 : 1, kI1 = KIND == kSubU16 ? 1 : 0;
    const int h = T.rows, w = T.cols;
    const int tid = threadIdx.x;
    // the nine windows' correlations (masked: sum I T M^2), second sums (sum I^2, masked: sum I^2 M^2) and per-channel sums
    unsigned long long corr[9], s2[9], s1[9][kS1 > 0 ? kS1 : 1];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        corr[k] = 0;
        s2[k] = 0;
#pragma unroll
        for (int c = 0; c < (kS1 > 0 ? kS1 : 1); ++c) s1[k][c] = 0;
    }
    const int oy = py - 1, ox = px - 1;         // image pixel of LDS patch (0, 0) for template pixel (r0, c0)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        for (int r0 = 0; r0 < h; r0 += kSubR)
            for (int c0 = 0; c0 < w; c0 += kSubC) {
                const int ni = min(kSubR, h - r0), nj = min(kSubC, w - c0);
                __syncthreads();                // the previous chunk's LDS reads are done
                if constexpr (KIND == kSubU16) {
                    win_load_templ(Tl[0], tp, h, w, r0, c0, tid);
                    win_load_templ(Tl[kT1], tp + (size_t)h * w, h, w, r0, c0, tid);
                    sub_load_image(Il[0], ip, pitch, rows, cols, oy + r0, ox + c0, 0u, tid);
                    sub_load_image(Il[kI1], lo_b, pitch, rows, cols, oy + r0, ox + c0, 0x80u, tid);
                } else {
                    win_load_templ(Tl[0], tp + (size_t)c * h * w, h, w, r0, c0, tid);
                    if constexpr (KIND == kSubU8Mask) win_load_templ(Tl[kT1], mk + (size_t)c * h * w, h, w, r0, c0, tid);
                    sub_load_image(Il[0], ip + c * plane, pitch, rows, cols, oy + r0, ox + c0, 0u, tid);
                }
                __syncthreads();
                const int i = tid / (kSubC / 4), j = (tid % (kSubC / 4)) * 4;
                if (i < ni && j < nj) {
                    const uint32_t t0 = Tl[0][i][j >> 2];
                    const uint32_t t1 = Tl[kT1][i][j >> 2];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const uint32_t* r = &Il[0][i + dy][0];
                        const uint32_t* rl = &Il[kI1][i + dy][0];
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const int k = dy * 3 + dx;
                            const uint32_t v = sub_quad(r, j, dx, nj);
                            if constexpr (KIND == kSubU8) {
                                corr[k] += __builtin_amdgcn_udot4(v, t0, 0u, false);
                                s1[k][c < kS1 ? c : 0] += __builtin_amdgcn_udot4(v, 0x01010101u, 0u, false);
                                s2[k] += __builtin_amdgcn_udot4(v, v, 0u, false);
                            } else if constexpr (KIND == kSubU8Mask) {
                                const uint32_t vm = v & t1;                 // I M (M binary: bytes 0xFF / 0x00)
                                corr[k] += __builtin_amdgcn_udot4(v, t0, 0u, false);
                                s2[k] += __builtin_amdgcn_udot4(vm, vm, 0u, false);
                            } else {                                         // uint16: I = 256 Ih + Il, T = 256 Th + Tl
                                const uint32_t vl = sub_quad(rl, j, dx, nj);
                                const unsigned long long hh = __builtin_amdgcn_udot4(v, t0, 0u, false);
                                const unsigned long long hl = __builtin_amdgcn_udot4(v, t1, 0u, false);
                                const unsigned long long lh = __builtin_amdgcn_udot4(vl, t0, 0u, false);
                                const unsigned long long ll = __builtin_amdgcn_udot4(vl, t1, 0u, false);
                                corr[k] += (hh << 16) + ((hl + lh) << 8) + ll;
                                s1[k][0] += ((unsigned long long)__builtin_amdgcn_udot4(v, 0x01010101u, 0u, false) << 8) +
                                            __builtin_amdgcn_udot4(vl, 0x01010101u, 0u, false);
                                s2[k] += ((unsigned long long)__builtin_amdgcn_udot4(v, v, 0u, false) << 16) +
                                         ((unsigned long long)__builtin_amdgcn_udot4(v, vl, 0u, false) << 9) +
                                         __builtin_amdgcn_udot4(vl, vl, 0u, false);
                            }
                        }
                    }
                }
            }
    }
    // reduce; thread k < 9 keeps window k's sums
    unsigned long long rc = 0, r2 = 0, r1[kS1 > 0 ? kS1 : 1];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const unsigned long long a = sub_reduce(corr[k], red);
        const unsigned long long b = sub_reduce(s2[k], red);
        if (tid == k) {
            rc = a;
            r2 = b;
        }
#pragma unroll
        for (int c = 0; c < kS1; ++c) {
            const unsigned long long s = sub_reduce(s1[k][c], red);
            if (tid == k) r1[c] = s;
        }
    }
    float score = NAN;
    if (tid < 9) {
        const int wy = py + tid / 3 - 1, wx = px + tid % 3 - 1;
        if (wy >= 0 && wx >= 0 && wy <= rows - h && wx <= cols - w) {
            if constexpr (kMasked) {
                score = finish_masked(method, (double)rc, (double)r2, T);
            } else {
                const double inv_area = 1.0 / ((double)h * (double)w);
                unsigned long long s1u[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) s1u[c] = r1[c];
                score = win_score<CH>(method, T, inv_area, rc, s1u, r2);
            }
        }
    }
    return score;
}

}  // namespace mtm
