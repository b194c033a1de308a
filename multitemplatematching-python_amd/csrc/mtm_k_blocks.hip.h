// Block matching kernels: every block of a reference image is a template that never exists on the host.
// blocks_gather_kernel cuts the blocks out of the reference's planes into planes of the call's own - the layout
// prepare_window_templates gives a template set - with the constants mtm_set_templates would give them; blocks_score_kernel
// scores the tiles of every block's map with the window kernels' tile scorer (win_score_tile, mtm_k_window.hip.h: the
// exhaustive map's float32 bits) and keeps each block's extremum in a key, no map is written; blocks_nbhd_kernel decodes
// the keys and scores the 3 x 3 neighbourhoods in the whole image's map; blocks_plane_kernel (5.6.1) sums planes instead.
// Boxes that follow a displacement (5.6.2): blocks_unit_kernel computes the units on the device, blocks_score_fixed_kernel
// scores over a fixed tile table, blocks_record_kernel decodes the keys into records, blocks_validate_kernel is the median
// test over a pass's records.  Second peaks (5.6.3): blocks_score_plane_kernel also stores the scores, blocks_second_kernel
// reduces each plane outside the exclusion window, blocks_second_record_kernel decodes.  Window deformation (5.6.4; the
// warp: mtm_k_deform.hip.h): blocks_deform_record_kernel adds the field at a block's centre to its record; steer = 1:
// blocks_steer_q8_kernel and blocks_smooth_q8_kernel make the Q8 nodes the next pass's warp and record kernels read.
// A mask over the reference (5.6.5): blocks_gather_masked_kernel cuts T M and the mask, blocks_score_masked_kernel,
// blocks_score_plane_masked_kernel and blocks_nbhd_masked_kernel are the masked siblings over one tile body of their own
// (blocks_tile_masked); the unmasked kernels are untouched by them.
// The passes over a frame stack (5.6.6): blocks_unit_clip_kernel computes a unit together with its clip offsets,
// blocks_plane_fixed_kernel sums planes over the fixed tile table at those offsets, blocks_plane_peak_kernel turns a pass's
// sums into means, NaN fill and the peak record that steers the next pass.
// The rules (mtm_blocks_*.h, mtm_quality_key.h, mtm_templ_stats.h) are the single source of host and device; one of each:
// the tile body of the four score kernels (blocks_tile; the kernels supply the sink), the key's decoder, the record that
// steers (blocks_steer_record_inl).  Launched by mtm_blocks.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mtm_blocks_deform.h"
#include "mtm_blocks_predict.h"
#include "mtm_blocks_second.h"
#include "mtm_blocks_steer.h"
#include "mtm_blocks_validate.h"
#include "mtm_ctx.h"
#include "mtm_device_util.hip.h"
#include "mtm_k_deform.hip.h"
#include "mtm_k_nbhd.hip.h"
#include "mtm_k_window.hip.h"
#include "mtm_templ_stats.h"

namespace mtm {

static_assert(kTrackTile == kWinTile, "plan_blocks tiles the maps as the window kernels walk them");

// Grid: one 256-thread work-group per block (launch slice; block k = k0 + blockIdx.x).  `ref` is the reference image - the
// stack's planes entered at its first row and bounded by its own `rows` -: uint8, plane c at ref.u8 + c * u8_plane;
// uint16, the high-byte plane with `lo_b` the low-byte plane XOR 0x80.  The block's window is copied into the call's
// template planes at tpx + toff[k] - uint8: [CH][h][w], tightly packed; uint16: the high-byte plane, then the low-byte
// plane, unbiased - and the sums of its pixels and of their squares per channel are reduced in uint64 (exact: at most 2^21
// uint16 pixels, sum v^2 < 2^53) in a fixed order; thread 0 writes the constants templ_stats_from_sums_inl gives for them -
// what mtm_set_templates would compute for the block set as a template - and the block's size into td[k] (the fields
// prepare_box_td fills; the others are zero).  A block that is not inside the reference is left alone (plan_blocks
// refuses it: a window that did not lie inside would be read out of bounds).
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_gather_kernel(ImageDev ref, const uint8_t* __restrict__ lo_b,
                                                            const mtm_block* __restrict__ blocks, int k0,
                                                            uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                            TemplDev* __restrict__ td, int method) {
    __shared__ unsigned long long red[4];
    const int k = k0 + (int)blockIdx.x;
    const mtm_block B = blocks[k];
    const int h = B.h, w = B.w;
    // (the same for the whole work-group: before any barrier)
    if (w < 1 || h < 1 || B.x < 0 || B.y < 0 || B.x > ref.cols - w || B.y > ref.rows - h) return;
    const int tid = threadIdx.x;
    const uint32_t n = (uint32_t)h * (uint32_t)w;           // (< 2^31: plan_blocks)
    uint8_t* tp = tpx + toff[k];
    const size_t base = (size_t)B.y * ref.u8_pitch + (size_t)B.x;
    unsigned long long s1[CH], s2[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        s1[c] = 0ull;
        s2[c] = 0ull;
        for (uint32_t p = (uint32_t)tid; p < n; p += 256u) {
            const size_t ip = base + (size_t)(p / (uint32_t)w) * ref.u8_pitch + (size_t)(p % (uint32_t)w);
            uint32_t v;
            if constexpr (U16) {
                const uint32_t hi = ref.u8[ip], lo = (uint32_t)lo_b[ip] ^ 0x80u;
                tp[p] = (uint8_t)hi;
                tp[(size_t)n + p] = (uint8_t)lo;
                v = (hi << 8) | lo;
            } else {
                v = ref.u8[(size_t)c * ref.u8_plane + ip];
                tp[(size_t)c * n + p] = (uint8_t)v;
            }
            s1[c] += v;
            s2[c] += (unsigned long long)v * v;
        }
    }
    double sum[kMaxChans] = {0.0, 0.0, 0.0, 0.0}, sumsq[kMaxChans] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        sum[c] = (double)sub_reduce(s1[c], red);
        sumsq[c] = (double)sub_reduce(s2[c], red);
    }
    if (tid == 0) {
        const TemplStats st = templ_stats_from_sums_inl(sum, sumsq, 0.0, false, h, w, CH, method);
        TemplDev T{};
#pragma unroll
        for (int c = 0; c < kMaxChans; ++c) T.mean[c] = st.mean[c];
        T.templ_norm = st.templ_norm;
        T.templ_sum2 = st.templ_sum2;
        T.all_ones = st.all_ones;
        T.rows = h;
        T.cols = w;
        td[k] = T;
    }
}

// The tile body of the three score kernels below, one work-group per tile of the launch's part of the tile table.  `img` is
// the searched image, entered and bounded as `ref` above: no row of the reference is read.  The windows of tile (ty0, tx0)
// of block u0's map are summed and scored by win_score_tile - boxes_score_kernel's float32 bits, the same function -, with
// the gathered template of the block, and every lane's output goes to sink(K, U, inside, y, x, score) instead of a map.
// MAY_LIE_OUTSIDE: the fixed table (fix_block_tiles) over units that a kernel computed - a tile outside its unit's clipped
// map leaves before any barrier, the test being the same for the whole work-group (track_score_kernel's rule); else
// every tile lies inside its map (plan_blocks).  A (2 margin + 1)^2 map fills only part of its tiles.
template <int CH, bool U16, bool MAY_LIE_OUTSIDE, class Sink>
__device__ __forceinline__ void blocks_tile(WinTemplLds (&Tl)[U16 ? 2 : 1], WinImageLds (&Il)[U16 ? 2 : 1], const ImageDev& img,
                                            const uint8_t* __restrict__ lo_b, const uint8_t* __restrict__ tpx,
                                            const long long* __restrict__ toff, const TemplDev* __restrict__ td,
                                            const TrackUnit* __restrict__ units, const TrackTile* __restrict__ tiles,
                                            int method, Sink&& sink) {
    const TrackTile K = tiles[blockIdx.x];
    const TrackUnit U = units[K.u0];
    if constexpr (MAY_LIE_OUTSIDE)
        if (K.ty0 >= U.oh || K.tx0 >= U.ow) return;     // (the same for the whole work-group: before any barrier)
    const TemplDev T = td[K.u0];
    win_score_tile<CH, U16>(Tl, Il, img, lo_b, tpx + toff[K.u0], T, U.y0 + K.ty0, U.x0 + K.tx0, K.ty0, K.tx0, U.oh, U.ow, method,
                            [&](bool inside, int y, int x, auto&& score) { sink(K, U, inside, y, x, score); });
}

// The sink of the two key kernels: the tile's best output goes into keys[u0] (win_merge_key): order(quality) << 32 |
// ~index, one atomicMax per wave.
struct BlocksKeySink {
    int mode_min;
    unsigned long long* __restrict__ keys;
    template <class Score>
    __device__ __forceinline__ void operator()(const TrackTile& K, const TrackUnit& U, bool inside, int y, int x,
                                               Score&& score) const {
        win_merge_key(inside, win_pos_word(y, x, U.ow), mode_min, score, keys + K.u0);
    }
};

// Each block's extremum as a key, over the plan's own tile table (blocks_tile, BlocksKeySink).
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_score_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                           const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                           const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units,
                                                           const TrackTile* __restrict__ tiles, int method, int mode_min,
                                                           unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    blocks_tile<CH, U16, false>(Tl, Il, img, lo_b, tpx, toff, td, units, tiles, method, BlocksKeySink{mode_min, keys});
}

// blocks_score_kernel over a FIXED tile table (fix_block_tiles, mtm_host.cpp: ceil((2 margin + 1) / 16)^2 tiles per
// block) for units that a kernel computed (blocks_unit_kernel): the same body and sink, with the early exit.  No LDS and
// no scratch over blocks_score_kernel.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_score_fixed_kernel(
    ImageDev img, const uint8_t* __restrict__ lo_b, const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
    const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units, const TrackTile* __restrict__ tiles, int method,
    int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    blocks_tile<CH, U16, true>(Tl, Il, img, lo_b, tpx, toff, td, units, tiles, method, BlocksKeySink{mode_min, keys});
}

// BlocksKeySink that also keeps the scores: an inside lane calls score() once, stores the float32 at cell (y, x) of block
// u0's plane - plane[poff[u0] + y U.ow + x], the map row-major and contiguous - and feeds the same value to win_merge_key,
// so the key is BlocksKeySink's.  A plain store: the tile table partitions a map, every cell has one writer.
struct BlocksScoredPlaneSink {
    int mode_min;
    unsigned long long* __restrict__ keys;
    float* __restrict__ plane;
    const long long* __restrict__ poff;
    template <class Score>
    __device__ __forceinline__ void operator()(const TrackTile& K, const TrackUnit& U, bool inside, int y, int x,
                                               Score&& score) const {
        float s = 0.0f;
        if (inside) {
            s = score();
            plane[(size_t)poff[K.u0] + (size_t)y * (size_t)U.ow + (size_t)x] = s;
        }
        win_merge_key(inside, win_pos_word(y, x, U.ow), mode_min, [&] { return s; }, keys + K.u0);
    }
};

// blocks_score_fixed_kernel with the scored-plane sink (the second-peak calls; their tables are always the fixed ones): the
// same body, LDS and keys, and every output of every unit's map lands in the unit's plane for blocks_second_kernel.  The
// plane of block u0 holds at least U.oh U.ow floats whatever unit the device computed (second_plane_floats).
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_score_plane_kernel(
    ImageDev img, const uint8_t* __restrict__ lo_b, const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
    const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units, const TrackTile* __restrict__ tiles, int method,
    int mode_min, unsigned long long* __restrict__ keys, float* __restrict__ plane, const long long* __restrict__ poff) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    blocks_tile<CH, U16, true>(Tl, Il, img, lo_b, tpx, toff, td, units, tiles, method,
                               BlocksScoredPlaneSink{mode_min, keys, plane, poff});
}

// ---- a static mask over the reference (mtm_match_blocks_masked): uint8 images, TM_SQDIFF / TM_CCORR_NORMED

// blocks_gather_kernel for a masked call.  `mask` is the call's mask plane, rows x cols bytes at `mask_pitch` bytes per
// row, non-zero = the pixel takes part, for every channel.  Block k's planes at tpx + toff[k] are T M, [CH][h][w], then the
// mask as bytes 0xFF / 0x00, [CH][h][w] (one copy per channel): what win_tile_sums_u8_masked and sub_nbhd_int<CH,
// kSubU8Mask> read as tp / mk.  sum (T M)^2 over all channels and the count of set pixels are reduced in uint64 in
// sub_reduce's fixed order (exact: < 2^49); thread 0 writes templ_stats_from_sums_inl's masked constants and the block's
// size into td[k], and the count into td[k].map_off (a block's template has no map in the arena): 0 = the mask keeps no
// pixel of the block, which is then not searched.  The same bounds test as blocks_gather_kernel covers the mask's reads.
template <int CH>
__global__ __launch_bounds__(256) void blocks_gather_masked_kernel(ImageDev ref, const uint8_t* __restrict__ mask,
                                                                   int mask_pitch, const mtm_block* __restrict__ blocks, int k0,
                                                                   uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                                   TemplDev* __restrict__ td, int method) {
    __shared__ unsigned long long red[4];
    const int k = k0 + (int)blockIdx.x;
    const mtm_block B = blocks[k];
    const int h = B.h, w = B.w;
    // (the same for the whole work-group: before any barrier)
    if (w < 1 || h < 1 || B.x < 0 || B.y < 0 || B.x > ref.cols - w || B.y > ref.rows - h) return;
    const int tid = threadIdx.x;
    const uint32_t n = (uint32_t)h * (uint32_t)w;           // (< 2^31: plan_blocks)
    uint8_t* tp = tpx + toff[k];
    uint8_t* mp = tp + (size_t)CH * n;
    const size_t base = (size_t)B.y * ref.u8_pitch + (size_t)B.x;
    const size_t mbase = (size_t)B.y * (size_t)mask_pitch + (size_t)B.x;
    unsigned long long tms = 0ull, count = 0ull;
    for (uint32_t p = (uint32_t)tid; p < n; p += 256u) {
        const size_t py = (size_t)(p / (uint32_t)w), px = (size_t)(p % (uint32_t)w);
        const bool m = mask[mbase + py * (size_t)mask_pitch + px] != 0;
        count += m ? 1ull : 0ull;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const uint32_t v = m ? (uint32_t)ref.u8[(size_t)c * ref.u8_plane + base + py * ref.u8_pitch + px] : 0u;
            tp[(size_t)c * n + p] = (uint8_t)v;
            mp[(size_t)c * n + p] = m ? (uint8_t)0xFF : (uint8_t)0x00;
            tms += (unsigned long long)(v * v);
        }
    }
    const unsigned long long tms_all = sub_reduce(tms, red);
    const unsigned long long count_all = sub_reduce(count, red);
    if (tid == 0) {
        const double none[kMaxChans] = {0.0, 0.0, 0.0, 0.0};
        const TemplStats st = templ_stats_from_sums_inl(none, none, (double)tms_all, /*masked=*/true, h, w, CH, method);
        TemplDev T{};
        T.templ2_mask2_sum = st.templ2_mask2_sum;
        T.map_off = (long long)count_all;
        T.rows = h;
        T.cols = w;
        td[k] = T;
    }
}

// blocks_tile for a masked call: the same tables and early exit, and a block whose mask keeps no pixel (td[u0].map_off ==
// 0, blocks_gather_masked_kernel) leaves as well - the same for the whole work-group, before any barrier -, so its key
// stays 0.  The tile is summed and scored by win_score_tile_masked with the block's T M and mask planes, and the sink gets
// valid = in the map and not NaN in place of `inside`.
template <int CH, bool MAY_LIE_OUTSIDE, class Sink>
__device__ __forceinline__ void blocks_tile_masked(WinTemplLds (&Tl)[2], WinImageLds& Il, const ImageDev& img,
                                                   const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                   const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units,
                                                   const TrackTile* __restrict__ tiles, int method, Sink&& sink) {
    const TrackTile K = tiles[blockIdx.x];
    const TrackUnit U = units[K.u0];
    if constexpr (MAY_LIE_OUTSIDE)
        if (K.ty0 >= U.oh || K.tx0 >= U.ow) return;     // (the same for the whole work-group: before any barrier)
    const TemplDev T = td[K.u0];
    if (T.map_off == 0) return;                         // (likewise: an empty mask)
    const uint8_t* tp = tpx + toff[K.u0];
    win_score_tile_masked<CH>(Tl, Il, img, tp, tp + (size_t)CH * (size_t)T.rows * (size_t)T.cols, T, U.y0 + K.ty0, U.x0 + K.tx0,
                              K.ty0, K.tx0, U.oh, U.ow, method,
                              [&](bool valid, int y, int x, auto&& score) { sink(K, U, valid, y, x, score); });
}

// blocks_score_kernel (FIXED = false: the plan's own tile table) and blocks_score_fixed_kernel (FIXED = true) of a masked
// call: blocks_tile_masked with the key sink, which a NaN lane enters as a lane outside the map does.
template <int CH, bool FIXED>
__global__ __launch_bounds__(256) void blocks_score_masked_kernel(ImageDev img, const uint8_t* __restrict__ tpx,
                                                                  const long long* __restrict__ toff,
                                                                  const TemplDev* __restrict__ td,
                                                                  const TrackUnit* __restrict__ units,
                                                                  const TrackTile* __restrict__ tiles, int method, int mode_min,
                                                                  unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[2];
    __shared__ __attribute__((aligned(16))) WinImageLds Il;
    blocks_tile_masked<CH, FIXED>(Tl, Il, img, tpx, toff, td, units, tiles, method, BlocksKeySink{mode_min, keys});
}

// BlocksScoredPlaneSink of a masked call: every cell of the map is stored, a NaN score as NaN - second_cell_key gives such
// a cell no key, so blocks_second_kernel never chooses it -, and only valid lanes compete for the first key.
struct BlocksMaskedPlaneSink {
    int mode_min;
    unsigned long long* __restrict__ keys;
    float* __restrict__ plane;
    const long long* __restrict__ poff;
    template <class Score>
    __device__ __forceinline__ void operator()(const TrackTile& K, const TrackUnit& U, bool valid, int y, int x,
                                               Score&& score) const {
        const float s = score();
        if (y < U.oh && x < U.ow) plane[(size_t)poff[K.u0] + (size_t)y * (size_t)U.ow + (size_t)x] = s;
        win_merge_key(valid, win_pos_word(y, x, U.ow), mode_min, [&] { return s; }, keys + K.u0);
    }
};

// blocks_score_plane_kernel of a masked call.  The plane of a block with an empty mask is not written and not read: its key
// stays 0, and blocks_second_kernel reads no cell of a block without a key.
template <int CH>
__global__ __launch_bounds__(256) void blocks_score_plane_masked_kernel(
    ImageDev img, const uint8_t* __restrict__ tpx, const long long* __restrict__ toff, const TemplDev* __restrict__ td,
    const TrackUnit* __restrict__ units, const TrackTile* __restrict__ tiles, int method, int mode_min,
    unsigned long long* __restrict__ keys, float* __restrict__ plane, const long long* __restrict__ poff) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[2];
    __shared__ __attribute__((aligned(16))) WinImageLds Il;
    blocks_tile_masked<CH, true>(Tl, Il, img, tpx, toff, td, units, tiles, method,
                                 BlocksMaskedPlaneSink{mode_min, keys, plane, poff});
}

// Grid: one 256-thread work-group per block (launch slice; block k = k0 + blockIdx.x), behind the score launch that wrote
// the block's plane: the largest key among the cells of the unit's oh x ow map outside the exclusion of radius
// `exclusion` around the first peak (keys[k], decoded by key_index) goes into keys2[k] - second_excluded and
// second_cell_key (mtm_blocks_second.h, the host's functions).  Lanes walk idx = tid, tid + 256, .. < oh ow: coalesced
// loads of cells the score launch wrote, nothing outside the map is read; per wave the shuffle ladder of win_merge_key,
// then the four waves through 32 B of LDS.  A block without a key reads nothing; keys2[k] is written either way (0: no
// second peak).
__global__ __launch_bounds__(256) void blocks_second_kernel(const TrackUnit* __restrict__ units,
                                                            const unsigned long long* __restrict__ keys,
                                                            const float* __restrict__ plane, const long long* __restrict__ poff,
                                                            int k0, int mode_min, int exclusion,
                                                            unsigned long long* __restrict__ keys2) {
    __shared__ unsigned long long red[4];
    const int k = k0 + (int)blockIdx.x;
    const int tid = threadIdx.x;
    const unsigned long long first = keys[k];
    if (first == 0ull) {                                    // (the same for the whole work-group: before any barrier)
        if (tid == 0) keys2[k] = 0ull;
        return;
    }
    const TrackUnit U = units[k];
    const uint32_t ow = (uint32_t)U.ow, n = (uint32_t)U.oh * ow;     // (< 2^32: plan_blocks, fix_block_tiles)
    const uint32_t at = key_index(first);
    const int py = (int)(at / ow), px = (int)(at % ow);
    const float* __restrict__ m = plane + poff[k];
    // the lane's cell (y, x) steps by 256 cells: 256 / ow rows and 256 % ow columns, with one carry
    const uint32_t sy = 256u / ow, sx = 256u % ow;
    uint32_t y = (uint32_t)tid / ow, x = (uint32_t)tid % ow;
    unsigned long long best = 0ull;
    for (unsigned long long idx = (unsigned long long)tid; idx < (unsigned long long)n; idx += 256ull) {
        if (!second_excluded((int)y, (int)x, py, px, exclusion)) {
            const unsigned long long key = second_cell_key(m[idx], mode_min, (uint32_t)idx);
            best = key > best ? key : best;
        }
        y += sy;
        x += sx;
        if (x >= ow) {
            x -= ow;
            ++y;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = red[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) b = red[w] > b ? red[w] : b;
        keys2[k] = b;
    }
}

// blocks_record_kernel for the second keys: second_key_record (mtm_blocks_second.h) at the unit's origin into recs2[k] -
// a block without a second peak gets position (-1, -1) and a NaN score.
__global__ __launch_bounds__(256) void blocks_second_record_kernel(const TrackUnit* __restrict__ units,
                                                                   const unsigned long long* __restrict__ keys2,
                                                                   const mtm_block* __restrict__ blocks, int n, int mode_min,
                                                                   mtm_hit* __restrict__ recs2) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const TrackUnit U = units[k];
    recs2[k] = second_key_record(keys2[k], mode_min, k, U.y0, U.x0, U.ow, blocks[k].w, blocks[k].h);
}

// One lane per block k < n: the unit of the block moved by its displacement - offs[2 k], offs[2 k + 1], or (prev !=
// nullptr) the one the records `prev` of the previous pass over grid `coarse` predict (blocks_predict_inl) -, clamped,
// widened by `margin` and clipped to the rows x cols image (blocks_unit_at_inl): units[k] = (k, y0, x0, oh, ow).  Every
// block lies inside the image (plan_blocks), so the coarse index is in range and the map has an output.
__global__ __launch_bounds__(256) void blocks_unit_kernel(const mtm_block* __restrict__ blocks, int n,
                                                          const int32_t* __restrict__ offs, const mtm_hit* __restrict__ prev,
                                                          BlockGrid coarse, int margin, int rows, int cols,
                                                          TrackUnit* __restrict__ units) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const mtm_block B = blocks[k];
    long long dx, dy;
    if (prev) {
        blocks_predict_inl(coarse, prev, B, &dx, &dy);
    } else {
        dx = offs[2 * (size_t)k];
        dy = offs[2 * (size_t)k + 1];
    }
    const BlockUnitBox u = blocks_unit_at_inl(B, dx, dy, margin, rows, cols);
    units[k] = TrackUnit{k, u.y0, u.x0, u.oh, u.ow};
}

// One lane per block k < n, after the pass's score launches: the block's key as its record in image coordinates -
// quality_key_record (mtm_quality_key.h) at the unit's origin, what decode_block_keys gives on the host - into recs[k].
__global__ __launch_bounds__(256) void blocks_record_kernel(const TrackUnit* __restrict__ units,
                                                            const unsigned long long* __restrict__ keys,
                                                            const mtm_block* __restrict__ blocks, int n, int mode_min,
                                                            mtm_hit* __restrict__ recs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const TrackUnit U = units[k];
    recs[k] = quality_key_record(keys[k], mode_min, k, U.y0, U.x0, U.ow, blocks[k].w, blocks[k].h);
}

// One lane per block k < n of a DEFORMED pass, behind the pass's blocks_record_kernel: the field of the coarse grid's
// displacements `disp` (deform_disp_kernel's pairs) at the block's doubled centre (deform_field_at_inl) goes into
// pred[2 k], pred[2 k + 1] in Q8, and its rounded integer part is added to the record's position - found in the warped
// image - so that recs[k] carries the block's displacement in the original image.  The position is not clamped.
// Q8: the nodes are themselves in Q8 (steer = 1: blocks_smooth_q8_kernel's), else whole pixels.
template <bool Q8>
__global__ __launch_bounds__(256) void blocks_deform_record_kernel(const mtm_block* __restrict__ blocks, int n, BlockGrid coarse,
                                                                   const int32_t* __restrict__ disp, mtm_hit* __restrict__ recs,
                                                                   int32_t* __restrict__ pred) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const mtm_block B = blocks[k];
    long long fx, fy;
    deform_field_at_of_inl<Q8>(coarse, disp, 2ll * B.x + B.w - 1, 2ll * B.y + B.h - 1, &fx, &fy);
    pred[2 * (size_t)k] = (int32_t)fx;
    pred[2 * (size_t)k + 1] = (int32_t)fy;
    recs[k].x += (int)deform_round_inl(fx);
    recs[k].y += (int)deform_round_inl(fy);
}

// One lane per block k < nx ny of a pass's grid, after the pass's blocks_record_kernel: the median test of the block's
// displacement against those of its 3 x 3 grid neighbourhood (blocks_steer_record_inl, mtm_blocks_validate.h: raw records
// only, so no lane waits for another) - valid[k] = 1 / 0, and steer[k] = the record that steers the next pass: recs[k],
// or for an outlier recs[k] moved to block position + the neighbours' median.  Every neighbour index is checked against
// the grid before its record is read.  No LDS and no scratch: the eight values are sorted in registers.
__global__ __launch_bounds__(256) void blocks_validate_kernel(const mtm_hit* __restrict__ recs, int nx, int ny, int sx, int sy,
                                                              double threshold, double e4, uint8_t* __restrict__ valid,
                                                              mtm_hit* __restrict__ steer) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nx * ny) return;
    mtm_hit r;
    valid[k] = blocks_steer_record_inl(recs, nx, ny, sx, sy, k, threshold, e4, &r) ? 1 : 0;
    steer[k] = r;
}

// One lane per record k < nx ny of a pass that steers another by refined positions (steer = 1), behind the pass's records,
// neighbourhoods and - with validation - flags: the record's steering displacement in Q8 (steer_d8_inl, mtm_blocks_steer.h:
// the fitted position in the searched image plus the field that steered the pass, minus the block's position; an outlier's:
// its neighbours' median) as a compact pair d8[2 k], d8[2 k + 1] - one 8-byte store.  Reads its own record only.
__global__ __launch_bounds__(256) void blocks_steer_q8_kernel(const mtm_hit* __restrict__ recs, const float* __restrict__ nbhd,
                                                              const int32_t* __restrict__ pred, const uint8_t* __restrict__ valid,
                                                              const mtm_hit* __restrict__ steer, int nx, int ny, int sx, int sy,
                                                              int mode_min, int32_t* __restrict__ d8) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nx * ny) return;
    int32_t dx, dy;
    steer_d8_inl(recs, nbhd, pred, valid, steer, nx, sx, sy, mode_min, k, &dx, &dy);
    *reinterpret_cast<int2*>(d8 + 2 * (size_t)k) = make_int2(dx, dy);
}

// One lane per node k < nx ny: the predictor filter (steer_smooth_inl: 3 x 3 binomial, clamped indices) of the pairs d8
// into `out` - another buffer, the one the warp reads -, so that no lane reads what another writes.
__global__ __launch_bounds__(256) void blocks_smooth_q8_kernel(const int32_t* __restrict__ d8, int nx, int ny,
                                                               int32_t* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nx * ny) return;
    int32_t sx8, sy8;
    steer_smooth_inl(d8, nx, ny, k % nx, k / nx, &sx8, &sy8);
    *reinterpret_cast<int2*>(out + 2 * (size_t)k) = make_int2(sx8, sy8);
}

// blocks_score_kernel's sibling for the ensemble planes of mtm_match_blocks_stack: the same tile and float32 score
// (win_score_tile), and instead of merging a key every output (y, x) of the map adds its score, widened to float64, to its
// cell of block u0's side x side plane of sums: acc[(u0 side + y + oy) side + x + ox], (ox, oy) = clip[2 u0],
// clip[2 u0 + 1] the block's clip offsets (BlockPlan::clip: y + oy, x + ox < side).  A plain read-modify-write:
// the tile table partitions every map, so a cell has one writer per launch, and the launches of successive pairs are
// ordered by the call's one stream - the sums are those of the pairs in order, bit for bit.  `first` (the call's first
// pair) stores instead of adding: the sum starts from s_0 itself, a -0.0 included.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_plane_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                           const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                           const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units,
                                                           const TrackTile* __restrict__ tiles, int method,
                                                           const int32_t* __restrict__ clip, int side, int first,
                                                           double* __restrict__ acc) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    blocks_tile<CH, U16, false>(Tl, Il, img, lo_b, tpx, toff, td, units, tiles, method,
                                [&](const TrackTile& K, const TrackUnit&, bool inside, int y, int x, auto&& score) {
                                    const int cy = y + clip[2 * K.u0 + 1], cx = x + clip[2 * K.u0];
                                    if (inside && cy < side && cx < side) {
                                        const float s = score();
                                        double* cell = acc + ((size_t)K.u0 * (size_t)side + (size_t)cy) * (size_t)side + (size_t)cx;
                                        *cell = first ? (double)s : *cell + (double)s;
                                    }
                                });
}

// ---- ensemble planes of boxes that follow a displacement (mtm_match_blocks_stack_at, mtm_match_blocks_stack_passes)

// blocks_unit_kernel's sibling for a call that sums planes: the same unit - the same arguments and functions -, and the
// block's clip offsets next to it: clip[2 k], clip[2 k + 1] = (ox, oy) = (U.x0 - (cx - margin), U.y0 - (cy - margin)) with
// (cx, cy) the moved and clamped position (blocks_moved_at_inl) - what BlockPlan::clip is to the host's units, both >= 0 -,
// one 8-byte store.
__global__ __launch_bounds__(256) void blocks_unit_clip_kernel(const mtm_block* __restrict__ blocks, int n,
                                                               const int32_t* __restrict__ offs, const mtm_hit* __restrict__ prev,
                                                               BlockGrid coarse, int margin, int rows, int cols,
                                                               TrackUnit* __restrict__ units, int32_t* __restrict__ clip) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const mtm_block B = blocks[k];
    long long dx, dy;
    if (prev) {
        blocks_predict_inl(coarse, prev, B, &dx, &dy);
    } else {
        dx = offs[2 * (size_t)k];
        dy = offs[2 * (size_t)k + 1];
    }
    const BlockUnitBox u = blocks_unit_at_inl(B, dx, dy, margin, rows, cols);
    int cx, cy;
    blocks_moved_at_inl(B, dx, dy, rows, cols, &cx, &cy);
    units[k] = TrackUnit{k, u.y0, u.x0, u.oh, u.ow};
    *reinterpret_cast<int2*>(clip + 2 * (size_t)k) = make_int2(u.x0 - (cx - margin), u.y0 - (cy - margin));
}

// blocks_plane_kernel over the FIXED tile table for units and clip offsets that blocks_unit_clip_kernel computed: the same
// body, score and read-modify-write, with blocks_score_fixed_kernel's early exit for a tile outside the unit's map.  Every
// output of the unit's map has one tile and one lane, so a cell still has one writer per launch; y + oy <= 2 margin and
// x + ox <= 2 margin for every output of a moved unit, and the guard against `side` stays.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_plane_fixed_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                                 const uint8_t* __restrict__ tpx,
                                                                 const long long* __restrict__ toff,
                                                                 const TemplDev* __restrict__ td,
                                                                 const TrackUnit* __restrict__ units,
                                                                 const TrackTile* __restrict__ tiles, int method,
                                                                 const int32_t* __restrict__ clip, int side, int first,
                                                                 double* __restrict__ acc) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    blocks_tile<CH, U16, true>(Tl, Il, img, lo_b, tpx, toff, td, units, tiles, method,
                               [&](const TrackTile& K, const TrackUnit&, bool inside, int y, int x, auto&& score) {
                                   const int cy = y + clip[2 * K.u0 + 1], cx = x + clip[2 * K.u0];
                                   if (inside && cy >= 0 && cx >= 0 && cy < side && cx < side) {
                                       const float s = score();
                                       double* cell = acc + ((size_t)K.u0 * (size_t)side + (size_t)cy) * (size_t)side + (size_t)cx;
                                       *cell = first ? (double)s : *cell + (double)s;
                                   }
                               });
}

// Grid: one 256-thread work-group per block (launch slice; block k = k0 + blockIdx.x), behind the last pair's plane launch:
// the block's side x side plane of sums becomes its plane of means and its peak.  Cell (cy, cx) lies in the clipped box iff
// oy <= cy < oy + U.oh and ox <= cx < ox + U.ow, (ox, oy) = clip[2 k], clip[2 k + 1]; such a cell's mean is
// (float)(acc / pairs) - the division in float64, one rounding to float32 -, every other cell is the quiet NaN (its sum is
// not read), and all side^2 cells are stored to planes.  The peak is plane_peaks' (MTM.blocks): the largest mean - the
// smallest, mode_min - over the cells that are not NaN, -0 equal to +0, of equal ones the first in row-major order:
// second_cell_key's key (mtm_blocks_second.h) with the plane's row-major index.  Lanes walk idx = tid, tid + 256, .. in
// order; the wave's maximum by the shuffle ladder, the four waves through 32 B of LDS: integer maxima, so the result is
// the same whatever the schedule.  The lane that holds the peak writes recs[k]: the peak's position (cx_k + dx, cy_k + dy) in image
// coordinates - (cx_k, cy_k) = (U.x0 - ox + margin, U.y0 - oy + margin), the moved block - and the plane's own float32 at
// that cell (a -0 stays -0); a plane without a number gives (-1, -1) and NaN.  Reads acc, writes planes and recs only.
__global__ __launch_bounds__(256) void blocks_plane_peak_kernel(const double* __restrict__ acc,
                                                                const TrackUnit* __restrict__ units,
                                                                const int32_t* __restrict__ clip,
                                                                const mtm_block* __restrict__ blocks, int k0, int side,
                                                                double pairs, int mode_min, float* __restrict__ planes,
                                                                mtm_hit* __restrict__ recs) {
    __shared__ unsigned long long red[4];
    const int k = k0 + (int)blockIdx.x;
    const int tid = threadIdx.x;
    const TrackUnit U = units[k];
    const int ox = clip[2 * (size_t)k], oy = clip[2 * (size_t)k + 1];
    const uint32_t sd = (uint32_t)side, n = sd * sd;        // (side^2 <= the planes' float budget < 2^31)
    const double* __restrict__ a = acc + (size_t)k * n;
    float* __restrict__ p = planes + (size_t)k * n;
    // the lane's cell (cy, cx) steps by 256 cells: 256 / side rows and 256 % side columns, with one carry
    const uint32_t sy = 256u / sd, sx = 256u % sd;
    uint32_t cy = (uint32_t)tid / sd, cx = (uint32_t)tid % sd;
    unsigned long long best = 0ull;
    float best_v = __builtin_nanf("");
    for (uint32_t idx = (uint32_t)tid; idx < n; idx += 256u) {
        const int y = (int)cy - oy, x = (int)cx - ox;
        float v = __builtin_nanf("");
        if (y >= 0 && y < U.oh && x >= 0 && x < U.ow) v = (float)(a[idx] / pairs);
        p[idx] = v;
        const unsigned long long key = second_cell_key(v, mode_min, idx);
        if (key > best) {
            best = key;
            best_v = v;
        }
        cy += sy;
        cx += sx;
        if (cx >= sd) {
            cx -= sd;
            ++cy;
        }
    }
    unsigned long long top = best;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(top, off);
        top = o > top ? o : top;
    }
    if ((tid & 63) == 0) red[tid >> 6] = top;
    __syncthreads();
    unsigned long long b = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) b = red[w] > b ? red[w] : b;
    // the lane that holds the winning cell writes the record (keys of different cells differ: one lane), or - no cell
    // holds a number - thread 0 the record that says so
    const mtm_block B = blocks[k];
    if (b != 0ull && best == b) {
        const uint32_t idx = key_index(b);
        recs[k] = key_record(idx, best_v, k, U.y0 - oy, U.x0 - ox, side, B.w, B.h);
    } else if (b == 0ull && tid == 0) {
        recs[k] = second_key_record(0ull, mode_min, k, 0, 0, side, B.w, B.h);
    }
}

// Grid: one 256-thread work-group per block (launch slice; block k = k0 + blockIdx.x), after the chunk's score launches:
// the key of the block is decoded (key_index, mtm_quality_key.h: the extremum's index in the block's map, moved by the
// map's origin into image coordinates) and the 3 x 3 neighbourhood of that window in the WHOLE image's map goes into
// out[9 k ..]: sub_nbhd_int's sums and win_score, mtm_hit_neighbourhoods' float32 bits, NaN outside the map.  A block
// without a key (no output scored) gets nine NaNs and reads no pixel.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void blocks_nbhd_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                          const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                          const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units,
                                                          const unsigned long long* __restrict__ keys, int k0, int method,
                                                          float* __restrict__ out) {
    constexpr int kKind = U16 ? kSubU16 : kSubU8;
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) SubImageLds Il[U16 ? 2 : 1];
    __shared__ unsigned long long red[4];
    const int k = k0 + (int)blockIdx.x;
    const TrackUnit U = units[k];
    const TemplDev T = td[k];
    const unsigned long long key = keys[k];
    const uint32_t idx = key_index(key);
    const int px = U.x0 + (int)(idx % (uint32_t)U.ow), py = U.y0 + (int)(idx / (uint32_t)U.ow);
    const int tid = threadIdx.x;
    float score = NAN;
    // (the same for the whole work-group: before any barrier)
    if (key != 0ull && px >= 0 && py >= 0 && px <= img.cols - T.cols && py <= img.rows - T.rows)
        score = sub_nbhd_int<CH, kKind>(Tl, Il, red, img.u8, img.u8_plane, lo_b, img.u8_pitch, img.rows, img.cols,
                                        tpx + toff[k], nullptr, T, px, py, method);
    if (tid < 9) out[(size_t)k * 9 + tid] = score;
}

// blocks_nbhd_kernel of a masked call: sub_nbhd_int's kSubU8Mask kind over the block's T M and mask planes
// (blocks_gather_masked_kernel's layout) - mtm_hit_neighbourhoods' float32 bits for the block set as a masked template.
// A block without a key - an empty mask, or a map of NaNs - gets nine NaNs and reads no pixel.
template <int CH>
__global__ __launch_bounds__(256) void blocks_nbhd_masked_kernel(ImageDev img, const uint8_t* __restrict__ tpx,
                                                                 const long long* __restrict__ toff,
                                                                 const TemplDev* __restrict__ td,
                                                                 const TrackUnit* __restrict__ units,
                                                                 const unsigned long long* __restrict__ keys, int k0, int method,
                                                                 float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[2];
    __shared__ __attribute__((aligned(16))) SubImageLds Il[1];
    __shared__ unsigned long long red[4];
    const int k = k0 + (int)blockIdx.x;
    const TrackUnit U = units[k];
    const TemplDev T = td[k];
    const unsigned long long key = keys[k];
    const uint32_t idx = key_index(key);
    const int px = U.x0 + (int)(idx % (uint32_t)U.ow), py = U.y0 + (int)(idx / (uint32_t)U.ow);
    const int tid = threadIdx.x;
    float score = NAN;
    // (the same for the whole work-group: before any barrier)
    if (key != 0ull && px >= 0 && py >= 0 && px <= img.cols - T.cols && py <= img.rows - T.rows) {
        const uint8_t* tp = tpx + toff[k];
        score = sub_nbhd_int<CH, kSubU8Mask>(Tl, Il, red, img.u8, img.u8_plane, nullptr, img.u8_pitch, img.rows, img.cols, tp,
                                             tp + (size_t)CH * (size_t)T.rows * (size_t)T.cols, T, px, py, method);
    }
    if (tid < 9) out[(size_t)k * 9 + tid] = score;
}

}  // namespace mtm
