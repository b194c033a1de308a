// Exact window sums of one 16 x 16 tile of score-map outputs, for the kernels that score arbitrary regions of a map: the
// template streams through LDS in chunks of kWinKR x kWinKC pixels next to the image rows the tile's windows cover, and
// v_dot4_u32_u8 forms the correlation and the window sums S1 (per channel) and S2 of the chunk in uint32; they are flushed
// to uint64 after every chunk, so the template's size is bounded by neither LDS nor the uint32 range.  Thread (ly, lx) =
// (tid / 16, tid % 16) of a 256-thread work-group owns output (oy0 + ly, ox0 + lx), whose window's top-left pixel is image
// pixel (oy0 + ly, ox0 + lx).  Image pixels outside `rows` x `cols` read as zero: only outputs outside the map read them,
// and those are never scored.
// win_score_tile is the one body of the kernels that score a tile of a unit's map for one template - boxes_score_kernel
// (mtm_boxes.hip), track_score_kernel and track_reacquire_kernel (mtm_track.hip), blocks_score_kernel and
// blocks_plane_kernel (mtm_k_blocks.hip.h): the sums, the lane's output and whether it lies in the map, and the float32 score
// (win_score) handed to the kernel's sink, which stores it, merges it into a key (win_merge_key) or adds it to a plane.
// win_score_tile_masked is its sibling for a uint8 template with a binary mask (blocks_tile_masked, mtm_k_blocks.hip.h).
// That these kernels give the same float32 bits rests on this one function.  pyr_window_kernel (mtm_pyramid.hip, uint8
// only) calls win_tile_sums_u8 and win_score itself inside its tile loop: with win_score_tile as the loop's body its
// 414 x 400 template case ran 6 % longer on the device (profiles/window_tile/summary.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mtm_device_util.hip.h"

namespace mtm {

constexpr int kWinTile = 16;                    // a tile of 16 x 16 outputs, one per thread
constexpr int kWinKR = 16, kWinKC = 64;         // template chunk in LDS: rows x columns
constexpr int kWinIW = kWinTile + kWinKC + 4;   // bytes per LDS image row: the dword right of the last one a thread reads
constexpr int kWinIR = kWinTile + kWinKR - 1;   // LDS image rows
// the uint32 sums of one chunk cannot overflow; they are flushed to uint64 after every chunk
static_assert((unsigned long long)kWinKR * kWinKC * 255ull * 255ull < (1ull << 32), "chunk too large for uint32 sums");

typedef uint32_t WinTemplLds[kWinKR][kWinKC / 4];
typedef uint32_t WinImageLds[kWinIR][kWinIW / 4];

// Template rows r0 .., columns c0 .. of one byte plane `tc` (h x w, tightly packed) into LDS, zero outside the template.
__device__ __forceinline__ void win_load_templ(WinTemplLds& Tl, const uint8_t* __restrict__ tc, int h, int w, int r0, int c0,
                                               int tid) {
    for (int k = tid; k < kWinKR * (kWinKC / 4); k += 256) {
        const int i = k / (kWinKC / 4), j = (k % (kWinKC / 4)) * 4;
        uint32_t v = 0u;
        if (r0 + i < h)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (c0 + j + b < w) v |= (uint32_t)tc[(size_t)(r0 + i) * w + c0 + j + b] << (8 * b);
        Tl[i][j >> 2] = v;
    }
}

// Image rows y0 .., columns x0 .. of one byte plane into LDS (zero outside rows x cols); every byte XOR `bias`.
__device__ __forceinline__ void win_load_image(WinImageLds& Il, const uint8_t* __restrict__ ip, int pitch, int rows, int cols,
                                               int y0, int x0, uint32_t bias, int tid) {
    for (int k = tid; k < kWinIR * (kWinIW / 4); k += 256) {
        const int i = k / (kWinIW / 4), j = (k % (kWinIW / 4)) * 4;
        const int y = y0 + i, x = x0 + j;
        uint32_t v = 0u;
        if (y < rows)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (x + b < cols) v |= ((uint32_t)ip[(size_t)y * pitch + x + b] ^ bias) << (8 * b);
        Il[i][j >> 2] = v;
    }
}

// Bytes lx + j .. lx + j + 3 of LDS image row `irow`, the columns past the chunk's last template column (nj) masked off.
__device__ __forceinline__ uint32_t win_image_quad(const uint32_t* irow, int lx, int j, int nj) {
    const int q = (lx + j) >> 2;
    uint32_t v = __builtin_amdgcn_alignbyte(irow[q + 1], irow[q], lx & 3);
    if (nj - j < 4) v &= (1u << (8 * (nj - j))) - 1u;
    return v;
}

// uint8 pixels, CH planes: corr = sum I T, s1[c] = sum I over channel c, s2 = sum I^2 over all channels, for the window of
// output (oy0 + ly, ox0 + lx).  `ip` plane c at ip + c * plane; template plane c at tp + c * h * w.
template <int CH>
__device__ __forceinline__ void win_tile_sums_u8(WinTemplLds& Tl, WinImageLds& Il, const uint8_t* __restrict__ ip,
                                                 long long plane, int pitch, int rows, int cols,
                                                 const uint8_t* __restrict__ tp, int h, int w, int oy0, int ox0,
                                                 unsigned long long& corr, unsigned long long (&s1)[CH],
                                                 unsigned long long& s2) {
    const int tid = threadIdx.x, ly = tid / kWinTile, lx = tid % kWinTile;
    corr = 0ull;
    s2 = 0ull;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        s1[c] = 0ull;
        const uint8_t* ipc = ip + c * plane;
        const uint8_t* tc = tp + (size_t)c * h * w;
        for (int r0 = 0; r0 < h; r0 += kWinKR)
            for (int c0 = 0; c0 < w; c0 += kWinKC) {
                __syncthreads();            // the previous chunk's LDS reads are done
                win_load_templ(Tl, tc, h, w, r0, c0, tid);
                win_load_image(Il, ipc, pitch, rows, cols, oy0 + r0, ox0 + c0, 0u, tid);
                __syncthreads();
                const int ni = min(kWinKR, h - r0), nj = min(kWinKC, w - c0);
                uint32_t a_corr = 0u, a_s1 = 0u, a_s2 = 0u;
                for (int i = 0; i < ni; ++i) {
                    const uint32_t* irow = &Il[ly + i][0];
                    for (int j = 0; j < nj; j += 4) {
                        const uint32_t v = win_image_quad(irow, lx, j, nj);
                        a_corr = __builtin_amdgcn_udot4(v, Tl[i][j >> 2], a_corr, false);
                        a_s1 = __builtin_amdgcn_udot4(v, 0x01010101u, a_s1, false);
                        a_s2 = __builtin_amdgcn_udot4(v, v, a_s2, false);
                    }
                }
                corr += a_corr;
                s1[c] += a_s1;
                s2 += a_s2;
            }
    }
}

// win_tile_sums_u8 for a template with a binary mask M (the same for every output): corr = sum I (T M), s2 = sum (I M)^2 over
// all channels - the two sums finish_masked takes; there is no S1.  `tp`: the planes of T M, `mk`: the mask's planes of
// 0xFF / 0x00 bytes, both [CH][h][w] tightly packed (sub_nbhd_int's kSubU8Mask operands).  The same chunk walk and
// barriers; per image quad two v_dot4 streams and one AND where the unmasked body issues three streams.  A quad's bytes
// past the chunk's last column are zero in v, in Tl and in Ml alike.
template <int CH>
__device__ __forceinline__ void win_tile_sums_u8_masked(WinTemplLds& Tl, WinTemplLds& Ml, WinImageLds& Il,
                                                        const uint8_t* __restrict__ ip, long long plane, int pitch, int rows,
                                                        int cols, const uint8_t* __restrict__ tp,
                                                        const uint8_t* __restrict__ mk, int h, int w, int oy0, int ox0,
                                                        unsigned long long& corr, unsigned long long& s2) {
    const int tid = threadIdx.x, ly = tid / kWinTile, lx = tid % kWinTile;
    corr = 0ull;
    s2 = 0ull;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const uint8_t* ipc = ip + c * plane;
        const uint8_t* tc = tp + (size_t)c * h * w;
        const uint8_t* mc = mk + (size_t)c * h * w;
        for (int r0 = 0; r0 < h; r0 += kWinKR)
            for (int c0 = 0; c0 < w; c0 += kWinKC) {
                __syncthreads();            // the previous chunk's LDS reads are done
                win_load_templ(Tl, tc, h, w, r0, c0, tid);
                win_load_templ(Ml, mc, h, w, r0, c0, tid);
                win_load_image(Il, ipc, pitch, rows, cols, oy0 + r0, ox0 + c0, 0u, tid);
                __syncthreads();
                const int ni = min(kWinKR, h - r0), nj = min(kWinKC, w - c0);
                uint32_t a_corr = 0u, a_s2 = 0u;
                for (int i = 0; i < ni; ++i) {
                    const uint32_t* irow = &Il[ly + i][0];
                    for (int j = 0; j < nj; j += 4) {
                        const uint32_t v = win_image_quad(irow, lx, j, nj);
                        a_corr = __builtin_amdgcn_udot4(v, Tl[i][j >> 2], a_corr, false);
                        const uint32_t vm = v & Ml[i][j >> 2];          // I M (M binary: bytes 0xFF / 0x00)
                        a_s2 = __builtin_amdgcn_udot4(vm, vm, a_s2, false);
                    }
                }
                corr += a_corr;
                s2 += a_s2;
            }
    }
}

// uint16 pixels, one channel, as byte planes: I = 256 Ih + Il, T = 256 Th + Tl.  Nine v_dot4 streams per chunk -
// Ih Th, Ih Tl, Il Th, Il Tl (the correlation), Ih, Il (S1), Ih^2, Ih Il, Il^2 (S2) - each < 2^32 per chunk, combined in
// uint64: every sum is exact.  `hi` = the high-byte plane, `lo_b` = the low-byte plane with every byte XOR 0x80 (the
// planes the MFMA kernel reads); template planes: high bytes at tp, low bytes at tp + h * w.
__device__ __forceinline__ void win_tile_sums_u16(WinTemplLds& Th, WinTemplLds& Tlo, WinImageLds& Ih, WinImageLds& Ilo,
                                                  const uint8_t* __restrict__ hi, const uint8_t* __restrict__ lo_b, int pitch,
                                                  int rows, int cols, const uint8_t* __restrict__ tp, int h, int w, int oy0,
                                                  int ox0, unsigned long long& corr, unsigned long long& s1,
                                                  unsigned long long& s2) {
    const int tid = threadIdx.x, ly = tid / kWinTile, lx = tid % kWinTile;
    corr = s1 = s2 = 0ull;
    const uint8_t* tlo = tp + (size_t)h * w;
    for (int r0 = 0; r0 < h; r0 += kWinKR)
        for (int c0 = 0; c0 < w; c0 += kWinKC) {
            __syncthreads();
            win_load_templ(Th, tp, h, w, r0, c0, tid);
            win_load_templ(Tlo, tlo, h, w, r0, c0, tid);
            win_load_image(Ih, hi, pitch, rows, cols, oy0 + r0, ox0 + c0, 0u, tid);
            win_load_image(Ilo, lo_b, pitch, rows, cols, oy0 + r0, ox0 + c0, 0x80u, tid);
            __syncthreads();
            const int ni = min(kWinKR, h - r0), nj = min(kWinKC, w - c0);
            uint32_t hh = 0u, hl = 0u, lh = 0u, ll = 0u, s1h = 0u, s1l = 0u, s2hh = 0u, s2hl = 0u, s2ll = 0u;
            for (int i = 0; i < ni; ++i) {
                const uint32_t* rh = &Ih[ly + i][0];
                const uint32_t* rl = &Ilo[ly + i][0];
                for (int j = 0; j < nj; j += 4) {
                    const uint32_t vh = win_image_quad(rh, lx, j, nj), vl = win_image_quad(rl, lx, j, nj);
                    const uint32_t th = Th[i][j >> 2], tl = Tlo[i][j >> 2];
                    hh = __builtin_amdgcn_udot4(vh, th, hh, false);
                    hl = __builtin_amdgcn_udot4(vh, tl, hl, false);
                    lh = __builtin_amdgcn_udot4(vl, th, lh, false);
                    ll = __builtin_amdgcn_udot4(vl, tl, ll, false);
                    s1h = __builtin_amdgcn_udot4(vh, 0x01010101u, s1h, false);
                    s1l = __builtin_amdgcn_udot4(vl, 0x01010101u, s1l, false);
                    s2hh = __builtin_amdgcn_udot4(vh, vh, s2hh, false);
                    s2hl = __builtin_amdgcn_udot4(vh, vl, s2hl, false);
                    s2ll = __builtin_amdgcn_udot4(vl, vl, s2ll, false);
                }
            }
            corr += ((unsigned long long)hh << 16) + (((unsigned long long)hl + lh) << 8) + ll;
            s1 += ((unsigned long long)s1h << 8) + s1l;
            s2 += ((unsigned long long)s2hh << 16) + ((unsigned long long)s2hl << 9) + s2ll;
        }
}

// ---- a set of templates of one shape over one tile (track_score_sets_kernel, mtm_track.hip) ----------------------------
// nv <= NV templates of one h x w share the tile's image rows and both window sums: per chunk the image rows are staged
// once, S1 and S2 are accumulated once, and only the correlation stream runs per template - 2 + nv v_dot4 streams where nv
// calls of win_tile_sums_u8 issue 3 nv (uint16: 5 + 4 nv against 9 nv).  Every sum is the exact integer the single-template
// functions above form, so win_score gives each template the same bits.  nv is the same for the whole work-group.

// The dot products of one staged chunk for exactly N templates: the inner loop holds no branch on the set's size.
template <int N, int NV>
__device__ __forceinline__ void win_set_dots_u8(const WinTemplLds (&Tl)[NV], const WinImageLds& Il, int ly, int lx, int ni,
                                                int nj, unsigned long long (&corr)[NV], unsigned long long& s1,
                                                unsigned long long& s2) {
    uint32_t a_corr[N], a_s1 = 0u, a_s2 = 0u;
#pragma unroll
    for (int n = 0; n < N; ++n) a_corr[n] = 0u;
    for (int i = 0; i < ni; ++i) {
        const uint32_t* irow = &Il[ly + i][0];
        for (int j = 0; j < nj; j += 4) {
            const uint32_t v = win_image_quad(irow, lx, j, nj);
#pragma unroll
            for (int n = 0; n < N; ++n) a_corr[n] = __builtin_amdgcn_udot4(v, Tl[n][i][j >> 2], a_corr[n], false);
            a_s1 = __builtin_amdgcn_udot4(v, 0x01010101u, a_s1, false);
            a_s2 = __builtin_amdgcn_udot4(v, v, a_s2, false);
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n) corr[n] += a_corr[n];
    s1 += a_s1;
    s2 += a_s2;
}

template <int N, int NV>
__device__ __forceinline__ void win_set_dispatch_u8(int nv, const WinTemplLds (&Tl)[NV], const WinImageLds& Il, int ly, int lx,
                                                    int ni, int nj, unsigned long long (&corr)[NV], unsigned long long& s1,
                                                    unsigned long long& s2) {
    if (nv == N) win_set_dots_u8<N, NV>(Tl, Il, ly, lx, ni, nj, corr, s1, s2);
    else if constexpr (N > 1) win_set_dispatch_u8<N - 1, NV>(nv, Tl, Il, ly, lx, ni, nj, corr, s1, s2);
}

// win_tile_sums_u8 for templates tp[0 .. nv - 1] (1 <= nv <= NV), all h x w with CH planes: corr[n] = sum I T_n; s1 and s2
// as there.  corr[n] for n >= nv is 0.
template <int CH, int NV>
__device__ __forceinline__ void win_tile_sums_u8_set(WinTemplLds (&Tl)[NV], WinImageLds& Il, const uint8_t* __restrict__ ip,
                                                     long long plane, int pitch, int rows, int cols,
                                                     const uint8_t* const (&tp)[NV], int nv, int h, int w, int oy0, int ox0,
                                                     unsigned long long (&corr)[NV], unsigned long long (&s1)[CH],
                                                     unsigned long long& s2) {
    const int tid = threadIdx.x, ly = tid / kWinTile, lx = tid % kWinTile;
#pragma unroll
    for (int n = 0; n < NV; ++n) corr[n] = 0ull;
    s2 = 0ull;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        s1[c] = 0ull;
        const uint8_t* ipc = ip + c * plane;
        for (int r0 = 0; r0 < h; r0 += kWinKR)
            for (int c0 = 0; c0 < w; c0 += kWinKC) {
                __syncthreads();            // the previous chunk's LDS reads are done
#pragma unroll
                for (int n = 0; n < NV; ++n)
                    if (n < nv) win_load_templ(Tl[n], tp[n] + (size_t)c * h * w, h, w, r0, c0, tid);
                win_load_image(Il, ipc, pitch, rows, cols, oy0 + r0, ox0 + c0, 0u, tid);
                __syncthreads();
                const int ni = min(kWinKR, h - r0), nj = min(kWinKC, w - c0);
                win_set_dispatch_u8<NV, NV>(nv, Tl, Il, ly, lx, ni, nj, corr, s1[c], s2);
            }
    }
}

// The uint16 counterpart (win_tile_sums_u16's byte planes): five streams for S1 and S2 once, four per template.
template <int N, int NV>
__device__ __forceinline__ void win_set_dots_u16(const WinTemplLds (&Th)[NV], const WinTemplLds (&Tlo)[NV],
                                                 const WinImageLds& Ih, const WinImageLds& Ilo, int ly, int lx, int ni, int nj,
                                                 unsigned long long (&corr)[NV], unsigned long long& s1,
                                                 unsigned long long& s2) {
    uint32_t hh[N], hl[N], lh[N], ll[N], s1h = 0u, s1l = 0u, s2hh = 0u, s2hl = 0u, s2ll = 0u;
#pragma unroll
    for (int n = 0; n < N; ++n) hh[n] = hl[n] = lh[n] = ll[n] = 0u;
    for (int i = 0; i < ni; ++i) {
        const uint32_t* rh = &Ih[ly + i][0];
        const uint32_t* rl = &Ilo[ly + i][0];
        for (int j = 0; j < nj; j += 4) {
            const uint32_t vh = win_image_quad(rh, lx, j, nj), vl = win_image_quad(rl, lx, j, nj);
#pragma unroll
            for (int n = 0; n < N; ++n) {
                const uint32_t th = Th[n][i][j >> 2], tl = Tlo[n][i][j >> 2];
                hh[n] = __builtin_amdgcn_udot4(vh, th, hh[n], false);
                hl[n] = __builtin_amdgcn_udot4(vh, tl, hl[n], false);
                lh[n] = __builtin_amdgcn_udot4(vl, th, lh[n], false);
                ll[n] = __builtin_amdgcn_udot4(vl, tl, ll[n], false);
            }
            s1h = __builtin_amdgcn_udot4(vh, 0x01010101u, s1h, false);
            s1l = __builtin_amdgcn_udot4(vl, 0x01010101u, s1l, false);
            s2hh = __builtin_amdgcn_udot4(vh, vh, s2hh, false);
            s2hl = __builtin_amdgcn_udot4(vh, vl, s2hl, false);
            s2ll = __builtin_amdgcn_udot4(vl, vl, s2ll, false);
        }
    }
#pragma unroll
    for (int n = 0; n < N; ++n)
        corr[n] += ((unsigned long long)hh[n] << 16) + (((unsigned long long)hl[n] + lh[n]) << 8) + ll[n];
    s1 += ((unsigned long long)s1h << 8) + s1l;
    s2 += ((unsigned long long)s2hh << 16) + ((unsigned long long)s2hl << 9) + s2ll;
}

template <int N, int NV>
__device__ __forceinline__ void win_set_dispatch_u16(int nv, const WinTemplLds (&Th)[NV], const WinTemplLds (&Tlo)[NV],
                                                     const WinImageLds& Ih, const WinImageLds& Ilo, int ly, int lx, int ni,
                                                     int nj, unsigned long long (&corr)[NV], unsigned long long& s1,
                                                     unsigned long long& s2) {
    if (nv == N) win_set_dots_u16<N, NV>(Th, Tlo, Ih, Ilo, ly, lx, ni, nj, corr, s1, s2);
    else if constexpr (N > 1) win_set_dispatch_u16<N - 1, NV>(nv, Th, Tlo, Ih, Ilo, ly, lx, ni, nj, corr, s1, s2);
}

// win_tile_sums_u16 for templates tp[0 .. nv - 1] (1 <= nv <= NV), all h x w: high bytes at tp[n], low bytes at
// tp[n] + h * w.  corr[n] for n >= nv is 0.
template <int NV>
__device__ __forceinline__ void win_tile_sums_u16_set(WinTemplLds (&Th)[NV], WinTemplLds (&Tlo)[NV], WinImageLds& Ih,
                                                      WinImageLds& Ilo, const uint8_t* __restrict__ hi,
                                                      const uint8_t* __restrict__ lo_b, int pitch, int rows, int cols,
                                                      const uint8_t* const (&tp)[NV], int nv, int h, int w, int oy0, int ox0,
                                                      unsigned long long (&corr)[NV], unsigned long long& s1,
                                                      unsigned long long& s2) {
    const int tid = threadIdx.x, ly = tid / kWinTile, lx = tid % kWinTile;
#pragma unroll
    for (int n = 0; n < NV; ++n) corr[n] = 0ull;
    s1 = s2 = 0ull;
    const size_t lo_off = (size_t)h * w;
    for (int r0 = 0; r0 < h; r0 += kWinKR)
        for (int c0 = 0; c0 < w; c0 += kWinKC) {
            __syncthreads();
#pragma unroll
            for (int n = 0; n < NV; ++n)
                if (n < nv) {
                    win_load_templ(Th[n], tp[n], h, w, r0, c0, tid);
                    win_load_templ(Tlo[n], tp[n] + lo_off, h, w, r0, c0, tid);
                }
            win_load_image(Ih, hi, pitch, rows, cols, oy0 + r0, ox0 + c0, 0u, tid);
            win_load_image(Ilo, lo_b, pitch, rows, cols, oy0 + r0, ox0 + c0, 0x80u, tid);
            __syncthreads();
            const int ni = min(kWinKR, h - r0), nj = min(kWinKC, w - c0);
            win_set_dispatch_u16<NV, NV>(nv, Th, Tlo, Ih, Ilo, ly, lx, ni, nj, corr, s1, s2);
        }
}

// The float32 score of a window from its exact sums: the statistics of stats_u8_kernel / stats_u8_mc_kernel /
// stats_u16_kernel / vsum_stats_kernel (exact sums, S1^2 summed over the channels, times 1 / area) and the epilogue of every
// score kernel (window_norm, finish_unmasked_with) - the exhaustive map's value bit for bit.
template <int CH>
__device__ __forceinline__ float win_score(int method, const TemplDev& T, double inv_area, unsigned long long corr,
                                           const unsigned long long (&s1)[CH], unsigned long long s2) {
    const bool centred = method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED;
    double s1d[kMaxChans] = {0.0, 0.0, 0.0, 0.0};
    double mean2 = 0.0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        s1d[c] = (double)s1[c];
        if (centred) mean2 += s1d[c] * s1d[c];
    }
    const double sum2 = (double)s2;
    const double wnd_mean2 = mean2 * inv_area;
    return finish_unmasked_with(
        method, (double)corr, [&](int c) { return s1d[c]; }, [&]() { return sum2; },
        [&]() { return window_norm(sum2, wnd_mean2); }, T, CH);
}

// The position word of output (y, x) of a map ow wide in a quality key: ~(row-major index), so that among equal
// qualities the first output in row-major order has the largest key.
__device__ __forceinline__ unsigned long long win_pos_word(int y, int x, int ow) {
    return 0xFFFFFFFFull - (unsigned long long)((long long)y * ow + x);
}

// The key of this lane's output - order(quality) << 32 | pos (win_pos_word), quality score() or its negative for the
// difference methods; 0 for a lane outside the map, which never calls score() -, reduced per wave and merged into *slot
// with one atomicMax per wave, as boxes_peaks_kernel keys a unit's extremum in global mode.  Every lane of the wave calls
// it (the shuffles).  (The tracking score kernels, mtm_track.hip, and blocks_score_kernel, mtm_k_blocks.hip.h.)
template <class Score>
__device__ __forceinline__ void win_merge_key(bool inside, unsigned long long pos, int mode_min, Score&& score,
                                              unsigned long long* __restrict__ slot) {
    unsigned long long key = 0ull;
    if (inside) {
        const float s = score();
        const float v = mode_min ? -s : s;
        key = ((unsigned long long)mf_float_order(v) << 32) | pos;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(slot, key);
}

// One tile of a map scored for one template: the tile's first output is (ty0, tx0) of a map of oh x ow outputs, and the
// window of that output has its top-left pixel at image pixel (py0, px0).  `img` holds the planes as the sums read them
// (uint8: plane c at img.u8 + c * img.u8_plane; uint16: img.u8 the high-byte plane, lo_b the low-byte plane XOR 0x80), tp
// the template's planes (win_tile_sums_*) and T its constants.  The sums run once, every lane through their barriers; then
// every lane calls sink(inside, y, x, score) exactly once: (y, x) the lane's output, inside = it lies in the map, score() the
// float32 value of win_score - the exhaustive map's bits.  The sink calls score() only where it needs the value and never
// for a lane that is not inside (such a lane's windows read pixels as zero).  Called by the whole work-group, outside
// divergent control flow.
template <int CH, bool U16, class Sink>
__device__ __forceinline__ void win_score_tile(WinTemplLds (&Tl)[U16 ? 2 : 1], WinImageLds (&Il)[U16 ? 2 : 1],
                                               const ImageDev& img, const uint8_t* __restrict__ lo_b,
                                               const uint8_t* __restrict__ tp, const TemplDev& T, int py0, int px0, int ty0,
                                               int tx0, int oh, int ow, int method, Sink&& sink) {
    const int h = T.rows, w = T.cols;
    const int tid = threadIdx.x;
    const double inv_area = 1.0 / ((double)h * (double)w);
    unsigned long long corr, s2, s1[CH];
    if constexpr (U16)
        win_tile_sums_u16(Tl[0], Tl[1], Il[0], Il[1], img.u8, lo_b, img.u8_pitch, img.rows, img.cols, tp, h, w, py0, px0, corr,
                          s1[0], s2);
    else
        win_tile_sums_u8<CH>(Tl[0], Il[0], img.u8, img.u8_plane, img.u8_pitch, img.rows, img.cols, tp, h, w, py0, px0, corr, s1,
                             s2);
    const int y = ty0 + tid / kWinTile, x = tx0 + tid % kWinTile;
    sink(y < oh && x < ow, y, x, [&] { return win_score<CH>(method, T, inv_area, corr, s1, s2); });
}

// win_score_tile for a masked uint8 template (methods TM_SQDIFF and TM_CCORR_NORMED): win_tile_sums_u8_masked's sums, the
// float32 score finish_masked gives for them with T.templ2_mask2_sum - the exhaustive masked map's bits - and
// sink(valid, y, x, score) with valid = the lane's output lies in the map AND its score is not NaN (TM_CCORR_NORMED where
// sum (I M)^2 or sum (T M)^2 is zero): mf_float_order ranks a positive NaN above +inf, so a NaN must never reach a key.
// score() is the value itself, NaN for a lane outside the map.  `mk`: the mask's planes.  Called as win_score_tile is.
template <int CH, class Sink>
__device__ __forceinline__ void win_score_tile_masked(WinTemplLds (&Tl)[2], WinImageLds& Il, const ImageDev& img,
                                                      const uint8_t* __restrict__ tp, const uint8_t* __restrict__ mk,
                                                      const TemplDev& T, int py0, int px0, int ty0, int tx0, int oh, int ow,
                                                      int method, Sink&& sink) {
    const int tid = threadIdx.x;
    unsigned long long corr, s2;
    win_tile_sums_u8_masked<CH>(Tl[0], Tl[1], Il, img.u8, img.u8_plane, img.u8_pitch, img.rows, img.cols, tp, mk, T.rows, T.cols,
                                py0, px0, corr, s2);
    const int y = ty0 + tid / kWinTile, x = tx0 + tid % kWinTile;
    float s = __builtin_nanf("");
    if (y < oh && x < ow) s = finish_masked(method, (double)corr, (double)s2, T);
    sink(s == s, y, x, [&] { return s; });
}

}  // namespace mtm
