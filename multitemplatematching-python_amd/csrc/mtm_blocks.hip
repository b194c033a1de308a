// libmtm_hip.so - block matching between two images of one shape in one call (mtm_match_blocks): every block
// of the reference image is a template, searched in the other image inside the block's own box widened by a margin - what
// mtm_find_matches_boxes returns in MTM_PEAKS_GLOBAL mode for the block's pixels set as a template.  The templates never
// exist on the host: both images go up as one stack of two (the reference in rows 0 .., the image below it),
// blocks_gather_kernel cuts every block out of the reference's planes into planes of the call's own - the layout
// prepare_window_templates gives a template set - and computes the constants mtm_set_templates would give it
// (templ_stats_from_sums_inl, the single source of host and device); blocks_score_kernel scores the tiles of every block's
// map with the window kernels' tile scorer (win_score_tile, mtm_k_window.hip.h: the exhaustive map's float32 bits) and
// keeps each block's extremum in a key, no map is written; blocks_nbhd_kernel, where asked for, decodes the keys and
// scores the 3 x 3 neighbourhoods in the whole image's map.  plan_blocks (mtm_host.cpp) checks the blocks and lays out
// the unit and tile tables and the chunks; the host waits once per call.  uint8 (1 or 3 channels) and single-channel
// uint16.  The template set of the context is neither read nor written.
// mtm_match_blocks_stack runs the same chain for every pair of a frame stack: the frames go up in stacked
// chunks (plan_blocks_stack, mtm_host.cpp), every pair has a row of keys of its own, and - ensemble planes - blocks_plane_kernel
// adds every output's score to the block's plane of float64 sums instead of keeping an extremum.
// mtm_match_blocks_at and mtm_match_blocks_passes search boxes that follow a displacement - uploaded
// offsets, or the previous pass's records -: blocks_unit_kernel computes every block's unit on the device
// (mtm_blocks_predict.h, the single source of host and device), blocks_score_fixed_kernel runs blocks_score_kernel's tile
// over a fixed tile table and leaves the tiles outside the unit's map, blocks_record_kernel decodes the keys into records
// on the device, which the next pass and the final copy read.  One chain (match_block_passes) behind both; every pass has
// its own row of keys, records and neighbourhoods.
// mtm_match_blocks_passes_validated runs the same chain with blocks_validate_kernel behind every pass's
// blocks_record_kernel: the median test of mtm_blocks_validate.h (the single source of host and device) over the pass's
// records, a flag per record and the records that steer the next pass instead of the raw ones.
// mtm_match_blocks_second and mtm_match_blocks_passes_second add every block's second correlation peak to that
// chain: blocks_score_plane_kernel - blocks_score_fixed_kernel with a sink that also stores the float32 scores - fills the
// planes of one sub-range of whole blocks, blocks_second_kernel reduces each plane to the best key outside the exclusion
// window around the first peak (mtm_blocks_second.h, the single source of host and device), and
// blocks_second_record_kernel decodes those keys behind blocks_record_kernel; the records come back behind the same wait.
// mtm_match_blocks_passes_deformed and mtm_deform_image add window deformation: a pass p >= 1 warps the
// original image by the field of the records that steer it (deform_disp_kernel, deform_image_kernel: mtm_k_deform.hip.h;
// the rule: mtm_blocks_deform.h, the single source of host and device) into a buffer of its own, searches the warped image
// over the host's units, and blocks_deform_record_kernel behind blocks_record_kernel adds the field at every block's centre
// to its record.  mtm_match_blocks_passes_steered with steer = 1 steers those passes by refined positions: behind a pass
// that steers another, blocks_steer_q8_kernel turns records and neighbourhoods into Q8 displacements and
// blocks_smooth_q8_kernel filters them over the grid (the rule: mtm_blocks_steer.h) into the nodes the next pass's warp and
// record kernels read - their Q8 instantiations; mtm_deform_image_q8 is the warp by Q8 nodes alone.
// One of each: the tile body of the four score kernels (blocks_tile; the kernels supply the sink), the key's decoder
// (mtm_quality_key.h: decode_block_keys on the host, blocks_record_kernel and blocks_nbhd_kernel on the device), the
// record that steers (blocks_steer_record_inl).  Every entry point is a composition of the same host steps:
// check_block_entry / check_block_pair, stage_block_call (buffers, the call's clock, uploads), blocks_pair (a pair's
// launch chain, the one place its kernels are launched), finish_block_call (copies back, the single wait, timing).
#include <climits>
#include <type_traits>

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

using namespace mtm;
using namespace mtmi;

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

}  // namespace mtm

namespace {

// f(ch, u16) with the images' pixel kind as compile-time constants, the kernels' <CH, U16>.
template <class F>
int blocks_dispatch(int dtype, int chans, F&& f) {
    if (dtype == MTM_U16) return f(std::integral_constant<int, 1>{}, std::true_type{});
    if (chans == 1) return f(std::integral_constant<int, 1>{}, std::false_type{});
    return f(std::integral_constant<int, 3>{}, std::false_type{});
}

// The image of rows row_off .. row_off + rows - 1 of the stack `st`: its planes entered at that row and bounded by `rows`,
// so that pixels below it read as zero whatever the stack holds there.
ImageDev stack_view(const ImageDev& st, int row_off, int rows) {
    ImageDev v = st;
    v.u8 = st.u8 + (size_t)row_off * st.u8_pitch;
    v.f32 = nullptr;
    v.rows = rows;
    return v;
}

// What both entry points check of their images behind check_image_args: the pixel kind, and that a pair's two images -
// one stack - stay within the rows a layout launch's grid holds.  `noun`: "images" / "frames", as the entry names them.
int check_block_images(const char* who, const std::string& noun, int rows, int chans, int dtype) {
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        set_error(std::string(who) + ": takes uint8 " + noun + " with 1 or 3 channels and single-channel uint16 " + noun);
        return MTM_E_INVALID;
    }
    if (2ll * rows > kBatchMaxRows) {
        set_error(std::string(who) + ": " + noun + " of more than " + std::to_string(kBatchMaxRows / 2) + " rows");
        return MTM_E_INVALID;
    }
    return MTM_OK;
}

// The host tables of a call, n blocks and n_tiles tiles in all (a multipass call: those of every pass, concatenated), and
// what the call needs besides them: `cells` float64 sums with the clip table (ensemble planes: cells > 0), or `key_rows`
// rows of n keys - with as many rows of neighbourhoods (nbhd), the uploaded offsets (offsets != nullptr), a row of records
// (recs) and of validation flags and steering records (validate); the second-peak calls: the plane offsets `poff` with
// plane_floats floats of planes (the largest launch sub-range's), a row of second keys and of their records.
struct BlockStage {
    const mtm_block* blocks;
    const long long* toff;
    const TrackUnit* units;
    const TrackTile* tiles;
    size_t n, n_tiles, max_bytes;
    size_t key_rows = 1, cells = 0;
    const int32_t *clip = nullptr, *offsets = nullptr;
    bool nbhd = false, recs = false, validate = false;
    const long long* poff = nullptr;
    size_t plane_floats = 0;
    // a deformed call: the weight tables of its deformed passes (dtab_words words), the warped image's bytes, the largest
    // steering grid's blocks and a row of Q8 fields at the blocks' centres
    const uint32_t* dtab = nullptr;
    size_t dtab_words = 0, warp_bytes = 0, disp_blocks = 0;
    bool deform = false;
    // ... steered by refined positions: the largest steering grid's unfiltered Q8 displacements
    size_t d8_blocks = 0;
};
BlockStage plan_stage(const mtm_block* blocks, const BlockPlan& P) {
    return BlockStage{blocks, P.toff.data(), P.units.data(), P.tiles.data(), P.units.size(), P.tiles.size(), P.max_bytes};
}

// The staging of every block call: the call's buffers, sized by S, then before() - what the entry enqueues ahead of the
// call's clock -, the event the call's time counts from, and the tables and zeroed results on the stream.
template <class Before>
int stage_block_call(mtm_ctx* c, const BlockStage& S, Before&& before) {
    const size_t n = S.n, n_keys = S.cells ? 0 : S.key_rows * n;
    // what goes up, in stream order (no source: not part of this call), and what is only sized
    const struct { DevBuf& buf; const void* src; size_t bytes; } up[] = {
        {c->blk_blocks, S.blocks, sizeof(mtm_block) * n},   {c->blk_toff, S.toff, sizeof(long long) * n},
        {c->blk_units, S.units, sizeof(TrackUnit) * n},     {c->blk_tiles, S.tiles, sizeof(TrackTile) * S.n_tiles},
        {c->blk_clip, S.clip, sizeof(int32_t) * 2 * n},     {c->blk_offs, S.offsets, sizeof(int32_t) * 2 * n},
        {c->blk_poff, S.poff, sizeof(long long) * n},       {c->blk_dtab, S.dtab, sizeof(uint32_t) * S.dtab_words}};
    const struct { DevBuf& buf; size_t bytes; } sized[] = {
        {c->blk_tpx, S.max_bytes},                          {c->blk_td, sizeof(TemplDev) * n},
        {c->blk_acc, sizeof(double) * S.cells},             {c->blk_keys, sizeof(unsigned long long) * n_keys},
        {c->blk_recs, S.recs ? sizeof(mtm_hit) * n : 0},    {c->blk_nbhd, S.nbhd ? sizeof(float) * 9 * n_keys : 0},
        {c->blk_valid, S.validate ? n : 0},                 {c->blk_steer, S.validate ? sizeof(mtm_hit) * n : 0},
        {c->blk_plane, sizeof(float) * S.plane_floats},     {c->blk_keys2, S.poff ? sizeof(unsigned long long) * n : 0},
        {c->blk_recs2, S.poff ? sizeof(mtm_hit) * n : 0},   {c->blk_warp, S.warp_bytes},
        {c->blk_disp, sizeof(int32_t) * 2 * S.disp_blocks}, {c->blk_pred, S.deform ? sizeof(int32_t) * 2 * n : 0},
        {c->blk_d8, sizeof(int32_t) * 2 * S.d8_blocks}};
    HIPC(hipSetDevice(c->device));
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    for (const auto& u : up)
        if (u.src) MTMC(u.buf.ensure(u.bytes));
    for (const auto& s : sized) MTMC(s.buf.ensure(s.bytes));
    MTMC(before());
    HIPC(hipEventRecord(c->ev[0], c->stream));
    for (const auto& u : up)
        if (u.src) HIPC(hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    if (S.cells) HIPC(hipMemsetAsync(c->blk_acc.p, 0, sizeof(double) * S.cells, c->stream));
    else HIPC(hipMemsetAsync(c->blk_keys.p, 0, sizeof(unsigned long long) * n_keys, c->stream));
    if (S.deform) HIPC(hipMemsetAsync(c->blk_pred.p, 0, sizeof(int32_t) * 2 * n, c->stream));    // (pass 0 predicts nothing)
    return MTM_OK;
}

// The end of every block call's chain: the event its time counts to, the copies back (`dst` == nullptr: not asked for),
// the call's single wait and its timing; the stacks a call uploads are none of the caller's images (no current image).
struct BlockCopy {
    void* dst;
    const void* src;
    size_t bytes;
};
int finish_block_call(mtm_ctx* c, std::initializer_list<BlockCopy> copies, size_t n_hits) {
    HIPC(hipEventRecord(c->ev[1], c->stream));
    for (const BlockCopy& b : copies)
        if (b.dst) HIPC(hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    c->timing.n_hits = (int64_t)n_hits;
    c->have_image = false;
    return MTM_OK;
}

// The two images of a pair entry point, of one shape and pixel kind.
struct BlockPair {
    const void* reference;
    int64_t reference_stride_bytes;
    const void* image;
    int64_t image_stride_bytes;
    int rows, cols, chans, dtype;
};

// ONE upload of each image of a pair, ahead of the call's clock: the stack's rows 0 .. rows - 1 are the reference, rows ..
// 2 rows - 1 the image.
int upload_block_pair(mtm_ctx* c, const BlockPair& I) {
    adopt_image(c, 2 * I.rows, I.cols, I.chans, I.dtype);
    return upload_image_pair(c, c->slot[c->cur], I.reference, I.reference_stride_bytes, I.image, I.image_stride_bytes, I.rows,
                             I.cols, I.chans, I.dtype, c->stream);
}

// The preamble of every entry point with a chain: the context, the entry's own argument test (`args_ok`) and the method, as
// one "bad arguments"; then no call in flight.
int check_block_entry(mtm_ctx* c, const char* who, bool args_ok, int method) {
    if (!c || !args_ok || method < MTM_TM_SQDIFF || method > MTM_TM_CCOEFF_NORMED) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    return MTM_OK;
}
// ... and of the pair entry points: both images, then what blocks ask of them.
int check_block_pair(mtm_ctx* c, const char* who, bool args_ok, int method, const BlockPair& I) {
    MTMC(check_block_entry(c, who, args_ok, method));
    MTMC(check_image_args(I.reference, I.rows, I.cols, I.chans, I.dtype, I.reference_stride_bytes, who));
    MTMC(check_image_args(I.image, I.rows, I.cols, I.chans, I.dtype, I.image_stride_bytes, who));
    return check_block_images(who, "images", I.rows, I.chans, I.dtype);
}

// What a pair's chain writes: a row of keys (and of neighbourhoods, or nullptr), or - side > 0, ensemble planes - the
// call's planes of sums, which the call's first pair starts.
struct BlockSink {
    unsigned long long* keys;
    float* nbhd;
    int side, first;
};

// The device tables a chain reads, indexed as its plan indexes them: the call's buffers from their start, or - one pass
// of several - from the pass's first block b0 and tile t0 (the constants td are every pass's in turn).  fixed: `tiles` is
// the fixed table (fix_block_tiles) and the units are the device's - blocks_score_fixed_kernel scores.
struct BlockTables {
    const mtm_block* blocks;
    const long long* toff;
    TemplDev* td;
    TrackUnit* units;
    const TrackTile* tiles;
    bool fixed;
};
BlockTables ctx_block_tables(mtm_ctx* c, size_t b0 = 0, size_t t0 = 0, bool fixed = false) {
    return BlockTables{c->blk_blocks.as<mtm_block>() + b0, c->blk_toff.as<long long>() + b0, c->blk_td.as<TemplDev>(),
                       c->blk_units.as<TrackUnit>() + b0, c->blk_tiles.as<TrackTile>() + t0, fixed};
}

// The floats block b's scored plane holds: the largest map a moved block can have, min(2 margin + 1, rows - h + 1) x
// min(2 margin + 1, cols - w + 1) (fix_block_tiles' spans: < 2^32) - known to the host whatever unit the device computes.
size_t second_plane_floats(const mtm_block& b, int margin, int rows, int cols) {
    const long long side = 2ll * margin + 1;
    return (size_t)std::min(side, (long long)rows - b.h + 1) * (size_t)std::min(side, (long long)cols - b.w + 1);
}

// What a second-peak pass adds to its chain (blocks_pair): the plan's blocks in sub-ranges of whole blocks - within a
// template-byte chunk, and their planes within `budget` floats, never fewer than one block -, each scored into the plane
// buffer (block k's plane at poff[k] floats) and reduced to keys2 by blocks_second_kernel before the next one overwrites it.
struct BlockSecondPass {
    int exclusion;
    std::vector<std::pair<int, int>> ranges;    // [b0, b1), in order, covering the pass
    std::vector<size_t> tstart;                 // block k's tiles are tiles[tstart[k] .. tstart[k + 1] - 1] of the pass
    const long long* poff;                      // device, indexed as the pass's tables
    unsigned long long* keys2;
};

// The sub-ranges and tile starts of plan P (fixed tile table) over `blocks`, the plane offsets appended to `poff` (one per
// block, relative to its sub-range's start) and the largest sub-range's floats raised into *max_floats.
void plan_second_pass(const BlockPlan& P, const mtm_block* blocks, int margin, int rows, int cols, size_t budget,
                      BlockSecondPass& X, std::vector<long long>& poff, size_t* max_floats) {
    const size_t n = P.units.size();
    X.tstart.assign(n + 1, P.tiles.size());
    for (size_t t = P.tiles.size(); t-- > 0;) X.tstart[(size_t)P.tiles[t].u0] = t;
    for (const BlockChunk& C : P.chunks) {
        int r0 = C.b0;
        size_t used = 0;
        for (int k = C.b0; k < C.b1; ++k) {
            const size_t f = second_plane_floats(blocks[k], margin, rows, cols);
            if (k > r0 && used + f > budget) {
                X.ranges.emplace_back(r0, k);
                r0 = k;
                used = 0;
            }
            poff.push_back((long long)used);
            used += f;
            *max_floats = std::max(*max_floats, used);
        }
        X.ranges.emplace_back(r0, C.b1);
    }
}

// One pair's launch chain for every block chunk - gather (unless the templates are already there), score or plane,
// [neighbourhoods] - in stream order: the next chunk's gather overwrites the template planes behind this chunk's last
// reader, and the host waits for none of them.  The pair is the stack's current image: the reference its rows
// r_slot * rows .., the searched image its rows i_slot * rows ...  X != nullptr (a second-peak pass over the fixed table):
// the chunk's score launch runs sub-range by sub-range with the scored-plane sink, blocks_second_kernel behind each.
// W != nullptr (a deformed pass): the searched image is *W with its low-byte plane W_lo - the warped image in a buffer
// of its own - instead of the stack's slot i_slot.
int blocks_pair(mtm_ctx* c, const BlockPlan& P, const BlockTables& B, int rows, int chans, int dtype, int method, int r_slot,
                int i_slot, bool gather, const BlockSink& S, const BlockSecondPass* X = nullptr, const ImageDev* W = nullptr,
                const uint8_t* W_lo = nullptr) {
    const ImageDev st = image_dev(c);
    const uint8_t* st_lo = c->slot[c->cur].u8b.as<uint8_t>() + st.u8_plane;        // uint16: [high ^ 0x80][low ^ 0x80]
    const ImageDev ref = stack_view(st, r_slot * rows, rows), img = W ? *W : stack_view(st, i_slot * rows, rows);
    const uint8_t* ref_lo = st_lo + (size_t)r_slot * rows * st.u8_pitch;
    const uint8_t* img_lo = W ? W_lo : st_lo + (size_t)i_slot * rows * st.u8_pitch;
    const int mode_min = method_mode_min(method) ? 1 : 0;
    uint8_t* tpx = c->blk_tpx.as<uint8_t>();
    const long long* toff = B.toff;
    TemplDev* td = B.td;
    const TrackUnit* units = B.units;
    return blocks_dispatch(dtype, chans, [&](auto ch, auto u16) -> int {
        constexpr int CH = decltype(ch)::value;
        constexpr bool U16 = decltype(u16)::value;
        size_t xr = 0;          // (the second-peak sub-ranges are walked in step with the chunks)
        for (const BlockChunk& C : P.chunks) {
            if (gather)
                MTMC(for_launch_slices((size_t)C.b0, (size_t)C.b1, [&](size_t b0, unsigned nb) -> int {
                    hipLaunchKernelGGL((blocks_gather_kernel<CH, U16>), dim3(nb), dim3(256), 0, c->stream, ref, ref_lo,
                                       B.blocks, (int)b0, tpx, toff, td, method);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
            for (; X && xr < X->ranges.size() && X->ranges[xr].second <= C.b1; ++xr) {
                const size_t r0 = (size_t)X->ranges[xr].first, r1 = (size_t)X->ranges[xr].second;
                MTMC(for_launch_slices(X->tstart[r0], X->tstart[r1], [&](size_t t0, unsigned nt) -> int {
                    hipLaunchKernelGGL((blocks_score_plane_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx,
                                       toff, td, units, B.tiles + t0, method, mode_min, S.keys, c->blk_plane.as<float>(), X->poff);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
                MTMC(for_launch_slices(r0, r1, [&](size_t b0, unsigned nb) -> int {
                    hipLaunchKernelGGL(blocks_second_kernel, dim3(nb), dim3(256), 0, c->stream, units, S.keys,
                                       c->blk_plane.as<float>(), X->poff, (int)b0, mode_min, X->exclusion, X->keys2);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
            }
            if (!X) MTMC(for_launch_slices(C.t0, C.t1, [&](size_t t0, unsigned nt) -> int {
                if (S.side > 0)
                    hipLaunchKernelGGL((blocks_plane_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx, toff,
                                       td, units, B.tiles + t0, method, c->blk_clip.as<int32_t>(), S.side, S.first,
                                       c->blk_acc.as<double>());
                else if (B.fixed)
                    hipLaunchKernelGGL((blocks_score_fixed_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx,
                                       toff, td, units, B.tiles + t0, method, mode_min, S.keys);
                else
                    hipLaunchKernelGGL((blocks_score_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx, toff,
                                       td, units, B.tiles + t0, method, mode_min, S.keys);
                HIPC(hipGetLastError());
                return MTM_OK;
            }));
            if (S.nbhd)
                MTMC(for_launch_slices((size_t)C.b0, (size_t)C.b1, [&](size_t b0, unsigned nb) -> int {
                    hipLaunchKernelGGL((blocks_nbhd_kernel<CH, U16>), dim3(nb), dim3(256), 0, c->stream, img, img_lo, tpx, toff,
                                       td, units, S.keys, (int)b0, method, S.nbhd);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
        }
        return MTM_OK;
    });
}

// A pair's row of keys as hits: each block's extremum in its own map, at the map's origin in image coordinates
// (quality_key_record: blocks_record_kernel's function).
void decode_block_keys(const BlockPlan& P, const mtm_block* blocks, const unsigned long long* hkeys, int method, mtm_hit* out) {
    const int mode_min = method_mode_min(method) ? 1 : 0;
    for (size_t k = 0; k < P.units.size(); ++k) {
        const TrackUnit& u = P.units[k];
        out[k] = quality_key_record(hkeys[k], mode_min, (int)k, u.y0, u.x0, u.ow, blocks[k].w, blocks[k].h);
    }
}

// The weight tables of the warp by the field of grid g over a rows x cols image, appended to t: deform_pack_inl of
// deform_axis_inl per column (padded with the last column's word to a multiple of kDeformPx) and per row (padded
// likewise, so that the next tables start 32-byte aligned).  Returns the column table's first word.
size_t deform_tables(const BlockGrid& g, int rows, int cols, std::vector<uint32_t>& t) {
    const size_t at = t.size();
    auto axis = [&](int n, int s, int wc, int len) {
        uint32_t w = 0;
        for (int x = 0; x < len; ++x) {
            int i, a8;
            deform_axis_inl(n, s, wc, 2ll * x, &i, &a8);
            t.push_back(w = deform_pack_inl(i, a8));
        }
        while (t.size() % kDeformPx) t.push_back(w);
    };
    axis(g.nx, g.sx, g.bw, cols);
    axis(g.ny, g.sy, g.bh, rows);
    return at;
}
size_t deform_table_rows_at(int cols) { return (size_t)(cols + kDeformPx - 1) / kDeformPx * kDeformPx; }

// The warped image of a call: byte planes of `pitch` bytes per row in blk_warp, `rows` rows each.
size_t warp_bytes(int rows, int pitch, int chans, int dtype) { return (size_t)rows * pitch * (dtype == MTM_U16 ? 2 : chans); }
ImageDev warp_view(const mtm_ctx* c, int rows, int cols, int chans) {
    ImageDev v{};
    v.u8 = c->blk_warp.as<uint8_t>();
    v.rows = rows;
    v.cols = cols;
    v.chans = chans;
    v.u8_pitch = c->u8_pitch;
    v.u8_plane = (long long)c->u8_pitch * rows;
    return v;
}

// The warp launch: `src` (its low-byte plane src_lo) warped into the call's blk_warp by the field of grid g with the
// displacements in blk_disp - q8: Q8 nodes - and the tables at word `tab` of blk_dtab.
int launch_deform(mtm_ctx* c, const ImageDev& src, const uint8_t* src_lo, int chans, int dtype, const BlockGrid& g, size_t tab,
                  bool q8 = false) {
    const ImageDev dst = warp_view(c, src.rows, src.cols, chans);
    DeformArgs a{};
    a.src = src.u8;
    a.src_lo = src_lo;
    a.src_plane = src.u8_plane;
    a.src_pitch = src.u8_pitch;
    a.dst = c->blk_warp.as<uint8_t>();
    a.dst_lo = a.dst + dst.u8_plane;
    a.dst_plane = dst.u8_plane;
    a.dst_pitch = dst.u8_pitch;
    a.rows = src.rows;
    a.cols = src.cols;
    a.disp = c->blk_disp.as<int32_t>();
    a.nx = g.nx;
    a.ny = g.ny;
    a.colw = c->blk_dtab.as<uint32_t>() + tab;
    a.roww = a.colw + deform_table_rows_at(src.cols);
    const dim3 grd((unsigned)((src.cols + kDeformLanesX * kDeformPx - 1) / (kDeformLanesX * kDeformPx)),
                   (unsigned)((src.rows + 256 / kDeformLanesX - 1) / (256 / kDeformLanesX)));
    return blocks_dispatch(dtype, chans, [&](auto ch, auto u16) -> int {
        if (q8)
            hipLaunchKernelGGL((deform_image_kernel<decltype(ch)::value, decltype(u16)::value, true>), grd, dim3(256), 0, c->stream,
                               a);
        else
            hipLaunchKernelGGL((deform_image_kernel<decltype(ch)::value, decltype(u16)::value>), grd, dim3(256), 0, c->stream, a);
        HIPC(hipGetLastError());
        return MTM_OK;
    });
}

// What a deformed call adds (mtm_match_blocks_passes_deformed): where the Q8 field at every block's centre goes, pass-major;
// steer (mtm_match_blocks_passes_steered): 0 - integer records steer the next pass -, 1 - refined positions, filtered.
struct BlockDeform {
    int32_t* predicted;
    int steer = 0;
};

// The median test a validated call runs behind every pass: its threshold, e4 = 4 epsilon (computed once, exact), and where
// the flags of every record go, pass-major.
struct BlockValidate {
    double threshold, e4;
    uint8_t* valid;
};

// The chain behind mtm_match_blocks_at (one pass over the caller's blocks, `offsets` uploaded) and
// mtm_match_blocks_passes (offsets == nullptr): both images go up once; per pass the units - pass 0 without offsets: the
// host's, of zero offsets; else blocks_unit_kernel's -, the pass's chain over its fixed tile table (blocks_pair) and
// blocks_record_kernel, all in stream order, so a pass reads the finished records of the one before and no work-group
// waits for another.  The records (and neighbourhoods) of every pass, pass-major, come back behind the call's single wait.
// V != nullptr (mtm_match_blocks_passes_validated): blocks_validate_kernel behind every pass's records, the next pass's
// units are predicted from its `steer` records instead of the raw ones, and the flags come back with the records.
// V == nullptr launches and copies exactly what the chain did before validation existed.
// X2 != nullptr (mtm_match_blocks_second, mtm_match_blocks_passes_second): every pass scores into planes and reduces them to
// second keys (blocks_pair, BlockSecondPass), blocks_second_record_kernel behind the pass's blocks_record_kernel turns them
// into records, which come back with the others and steer nothing.  X2 == nullptr: the chain as it is without.
// D != nullptr (mtm_match_blocks_passes_deformed; never with offsets or X2): a pass p >= 1 does not move its boxes - the
// records that steer it become compact displacements (deform_disp_kernel), the ORIGINAL image is warped by their field
// into blk_warp (deform_image_kernel), the pass searches the warped image over the host's units of zero offsets, and
// blocks_deform_record_kernel behind blocks_record_kernel adds the field at every block's centre to its record, which is
// what validation tests and what steers the next pass; the fields come back with the records.  D == nullptr launches and
// copies exactly what the chain did before deformation existed.
// D->steer == 1: every pass that steers another also gets its neighbourhoods (whether or not the caller asked for them),
// blocks_steer_q8_kernel behind its records and flags turns them into Q8 steering displacements and
// blocks_smooth_q8_kernel filters those into blk_disp - in place of deform_disp_kernel ahead of the next pass, whose warp
// and record kernels then read Q8 nodes.  D->steer == 0 launches exactly the kernels it did before.
struct BlockSecondOut {
    int exclusion;
    mtm_hit* second;
};
int match_block_passes(mtm_ctx* c, const BlockPair& I, const std::vector<BlockPassPlan>& Q, const int32_t* offsets, int method,
                       mtm_hit* out, float* nbhd, const BlockValidate* V = nullptr, const BlockSecondOut* X2 = nullptr,
                       const BlockDeform* D = nullptr) {
    const int rows = I.rows, cols = I.cols, chans = I.chans, dtype = I.dtype;
    // the tables of every pass, concatenated: one upload each
    std::vector<mtm_block> blocks;
    std::vector<long long> toff;
    std::vector<TrackUnit> units;
    std::vector<TrackTile> tiles;
    size_t max_bytes = 0;
    for (const BlockPassPlan& q : Q) {
        blocks.insert(blocks.end(), q.blocks.begin(), q.blocks.end());
        toff.insert(toff.end(), q.plan.toff.begin(), q.plan.toff.end());
        units.insert(units.end(), q.plan.units.begin(), q.plan.units.end());
        tiles.insert(tiles.end(), q.plan.tiles.begin(), q.plan.tiles.end());
        max_bytes = std::max(max_bytes, q.plan.max_bytes);
    }
    const size_t n = blocks.size();
    BlockStage S{blocks.data(), toff.data(), units.data(), tiles.data(), n, tiles.size(), max_bytes};
    S.nbhd = nbhd != nullptr;
    S.offsets = offsets;
    S.recs = true;
    S.validate = V != nullptr;
    // second peaks: every pass's plane sub-ranges, one table of plane offsets for the call
    std::vector<BlockSecondPass> X(X2 ? Q.size() : 0);
    std::vector<long long> poff;
    if (X2) {
        poff.reserve(n);
        for (size_t p = 0; p < Q.size(); ++p) {
            X[p].exclusion = X2->exclusion;
            plan_second_pass(Q[p].plan, Q[p].blocks.data(), Q[p].margin, rows, cols, (size_t)c->boxes_max_floats, X[p], poff,
                             &S.plane_floats);
        }
        S.poff = poff.data();
    }
    // deformation: the weight tables of every pass p >= 1 (those of pass p - 1's grid), one upload
    std::vector<uint32_t> dtab;
    std::vector<size_t> dtab_at(Q.size(), 0);
    if (D) {
        for (size_t p = 1; p < Q.size(); ++p) {
            dtab_at[p] = deform_tables(Q[p - 1].grid, rows, cols, dtab);
            S.disp_blocks = std::max(S.disp_blocks, Q[p - 1].blocks.size());
        }
        S.deform = true;
        if (D->steer && Q.size() > 1) {
            S.d8_blocks = S.disp_blocks;
            S.nbhd = true;
        }
        S.dtab = dtab.empty() ? nullptr : dtab.data();
        S.dtab_words = dtab.size();
        if (Q.size() > 1) S.warp_bytes = warp_bytes(rows, (int)round_up((size_t)cols + kPadCols, 64), chans, dtype);
    }
    MTMC(stage_block_call(c, S, [&] { return upload_block_pair(c, I); }));

    const int mode_min = method_mode_min(method) ? 1 : 0;
    size_t b0 = 0, t0 = 0;
    for (size_t p = 0; p < Q.size(); ++p) {
        const BlockPassPlan& q = Q[p];
        const int np = (int)q.blocks.size();
        const unsigned lanes_grid = (unsigned)((np + 255) / 256);
        const BlockTables B = ctx_block_tables(c, b0, t0, true);
        unsigned long long* keys = c->blk_keys.as<unsigned long long>() + b0;
        mtm_hit* recs = c->blk_recs.as<mtm_hit>() + b0;
        // what steers this pass: the previous pass's records, validated or raw
        const mtm_hit* prev = V ? c->blk_steer.as<mtm_hit>() + b0 : recs;
        const bool warped = D && p > 0, q8 = D && D->steer, steers = q8 && p + 1 < Q.size();
        ImageDev wimg{};
        if (warped) {
            const BlockGrid& g = Q[p - 1].grid;
            if (!q8) {          // (q8: the pass before left its filtered Q8 nodes in blk_disp)
                hipLaunchKernelGGL(deform_disp_kernel, dim3((unsigned)((Q[p - 1].blocks.size() + 255) / 256)), dim3(256), 0,
                                   c->stream, prev - Q[p - 1].blocks.size(), g, c->blk_disp.as<int32_t>());
                HIPC(hipGetLastError());
            }
            const ImageDev st = image_dev(c);
            MTMC(launch_deform(c, stack_view(st, rows, rows),
                               c->slot[c->cur].u8b.as<uint8_t>() + st.u8_plane + (size_t)rows * st.u8_pitch, chans, dtype, g,
                               dtab_at[p], q8));
            wimg = warp_view(c, rows, cols, chans);
        } else if (p > 0 || offsets) {
            hipLaunchKernelGGL(blocks_unit_kernel, dim3(lanes_grid), dim3(256), 0, c->stream, B.blocks, np,
                               p > 0 ? nullptr : c->blk_offs.as<int32_t>(), p > 0 ? prev - Q[p - 1].blocks.size() : nullptr,
                               p > 0 ? Q[p - 1].grid : BlockGrid{}, q.margin, rows, cols, B.units);
            HIPC(hipGetLastError());
        }
        if (X2) {
            X[p].poff = c->blk_poff.as<long long>() + b0;
            X[p].keys2 = c->blk_keys2.as<unsigned long long>() + b0;
        }
        MTMC(blocks_pair(c, q.plan, B, rows, chans, dtype, method, 0, 1, true,
                         BlockSink{keys, nbhd || steers ? c->blk_nbhd.as<float>() + 9 * b0 : nullptr, 0, 0}, X2 ? &X[p] : nullptr,
                         warped ? &wimg : nullptr, warped ? wimg.u8 + wimg.u8_plane : nullptr));
        hipLaunchKernelGGL(blocks_record_kernel, dim3(lanes_grid), dim3(256), 0, c->stream, B.units, keys, B.blocks, np, mode_min,
                           recs);
        HIPC(hipGetLastError());
        if (warped) {
            if (q8)
                hipLaunchKernelGGL(blocks_deform_record_kernel<true>, dim3(lanes_grid), dim3(256), 0, c->stream, B.blocks, np,
                                   Q[p - 1].grid, c->blk_disp.as<int32_t>(), recs, c->blk_pred.as<int32_t>() + 2 * b0);
            else
                hipLaunchKernelGGL(blocks_deform_record_kernel<false>, dim3(lanes_grid), dim3(256), 0, c->stream, B.blocks, np,
                                   Q[p - 1].grid, c->blk_disp.as<int32_t>(), recs, c->blk_pred.as<int32_t>() + 2 * b0);
            HIPC(hipGetLastError());
        }
        if (X2) {
            hipLaunchKernelGGL(blocks_second_record_kernel, dim3(lanes_grid), dim3(256), 0, c->stream, B.units, X[p].keys2,
                               B.blocks, np, mode_min, c->blk_recs2.as<mtm_hit>() + b0);
            HIPC(hipGetLastError());
        }
        if (V) {        // (np = nx ny: plan_block_passes lays out the whole grid)
            hipLaunchKernelGGL(blocks_validate_kernel, dim3(lanes_grid), dim3(256), 0, c->stream, recs, q.grid.nx, q.grid.ny,
                               q.grid.sx, q.grid.sy, V->threshold, V->e4, c->blk_valid.as<uint8_t>() + b0,
                               c->blk_steer.as<mtm_hit>() + b0);
            HIPC(hipGetLastError());
        }
        if (steers) {   // (behind this pass's last reader of blk_disp: the filter may overwrite it)
            hipLaunchKernelGGL(blocks_steer_q8_kernel, dim3(lanes_grid), dim3(256), 0, c->stream, recs,
                               c->blk_nbhd.as<float>() + 9 * b0, c->blk_pred.as<int32_t>() + 2 * b0,
                               V ? c->blk_valid.as<uint8_t>() + b0 : nullptr, V ? c->blk_steer.as<mtm_hit>() + b0 : nullptr,
                               q.grid.nx, q.grid.ny, q.grid.sx, q.grid.sy, mode_min, c->blk_d8.as<int32_t>());
            HIPC(hipGetLastError());
            hipLaunchKernelGGL(blocks_smooth_q8_kernel, dim3(lanes_grid), dim3(256), 0, c->stream, c->blk_d8.as<int32_t>(),
                               q.grid.nx, q.grid.ny, c->blk_disp.as<int32_t>());
            HIPC(hipGetLastError());
        }
        b0 += q.blocks.size();
        t0 += q.plan.tiles.size();
    }

    // the records (and neighbourhoods, and flags) come back behind the call's single wait
    return finish_block_call(c, {{out, c->blk_recs.p, sizeof(mtm_hit) * n}, {nbhd, c->blk_nbhd.p, sizeof(float) * 9 * n},
                                 {V ? V->valid : nullptr, c->blk_valid.p, n},
                                 {X2 ? X2->second : nullptr, c->blk_recs2.p, sizeof(mtm_hit) * n},
                                 {D ? D->predicted : nullptr, c->blk_pred.p, sizeof(int32_t) * 2 * n}}, n);
}

// threshold and epsilon of the median test: finite and >= 0, else MTM_E_INVALID naming the argument.
int check_validate_args(const char* who, double threshold, double epsilon) {
    for (const auto& a : {std::make_pair("threshold", threshold), std::make_pair("epsilon", epsilon)})
        if (!(a.second >= 0.0) || !std::isfinite(a.second)) {
            set_error(std::string(who) + ": " + a.first + " must be finite and >= 0 (got " + std::to_string(a.second) + ")");
            return MTM_E_INVALID;
        }
    return MTM_OK;
}

}  // namespace

extern "C" {

int mtm_match_blocks_at(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                        int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                        const int32_t* offsets, int n_blocks, int margin, int method, mtm_hit* out, float* nbhd) {
    const char* who = "mtm_match_blocks_at";
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_blocks >= 0 && margin >= 0 && (n_blocks == 0 || (blocks && offsets && out)), method, I));
    std::vector<BlockPassPlan> Q(1);
    Q[0].grid = BlockGrid{};
    Q[0].margin = margin;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, Q[0].plan,
                     false));
    if (n_blocks == 0) return MTM_OK;
    MTMC(fix_block_tiles(Q[0].plan, rows, cols, blocks, margin, who));
    Q[0].blocks.assign(blocks, blocks + n_blocks);
    return match_block_passes(c, I, Q, offsets, method, out, nbhd);
}

int mtm_match_blocks_passes(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                            const mtm_block_pass* passes, int n_passes, int method, mtm_hit* out, float* nbhd) {
    const char* who = "mtm_match_blocks_passes";
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_passes >= 1 && passes && out, method, I));
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(rows, cols, chans, dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    return match_block_passes(c, I, Q, nullptr, method, out, nbhd);
}

int mtm_match_blocks_passes_validated(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                      int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                      const mtm_block_pass* passes, int n_passes, int method, double threshold,
                                      double epsilon, mtm_hit* out, float* nbhd, uint8_t* valid) {
    const char* who = "mtm_match_blocks_passes_validated";
    MTMC(check_validate_args(who, threshold, epsilon));         // (ahead of everything else, a null context included)
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_passes >= 1 && passes && out && valid, method, I));
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(rows, cols, chans, dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    const BlockValidate V{threshold, 4.0 * epsilon, valid};
    return match_block_passes(c, I, Q, nullptr, method, out, nbhd, &V);
}

int mtm_debug_validate_blocks(mtm_ctx* c, const mtm_hit* recs, int nx, int ny, int sx, int sy, double threshold, double epsilon,
                              uint8_t* valid, mtm_hit* steer) {
    const char* who = "mtm_debug_validate_blocks";
    if (!recs || !valid || !steer || nx < 1 || ny < 1 || sx < 1 || sy < 1 || (long long)nx * ny > INT_MAX) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTMC(check_validate_args(who, threshold, epsilon));
    const size_t n = (size_t)nx * (size_t)ny;
    const double e4 = 4.0 * epsilon;
    if (!c) {           // the rule itself, on the host
        for (int k = 0; k < (int)n; ++k)
            valid[k] = blocks_steer_record_inl(recs, nx, ny, sx, sy, k, threshold, e4, &steer[k]) ? 1 : 0;
        return MTM_OK;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    HIPC(hipSetDevice(c->device));
    MTMC(c->blk_recs.ensure(sizeof(mtm_hit) * n));
    MTMC(c->blk_valid.ensure(n));
    MTMC(c->blk_steer.ensure(sizeof(mtm_hit) * n));
    HIPC(hipMemcpyAsync(c->blk_recs.p, recs, sizeof(mtm_hit) * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(blocks_validate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       c->blk_recs.as<mtm_hit>(), nx, ny, sx, sy, threshold, e4, c->blk_valid.as<uint8_t>(),
                       c->blk_steer.as<mtm_hit>());
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(valid, c->blk_valid.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipMemcpyAsync(steer, c->blk_steer.p, sizeof(mtm_hit) * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return MTM_OK;
}

int mtm_match_blocks_passes_deformed(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                     int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                     const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                     mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted) {
    const char* who = "mtm_match_blocks_passes_deformed";
    if (valid) MTMC(check_validate_args(who, threshold, epsilon));      // (ahead of everything else, as the validated call)
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_passes >= 1 && passes && out && predicted, method, I));
    // every pass moves a record by less than the image's larger side past the field that steered it
    if ((long long)n_passes * std::max(rows, cols) > kDeformMaxDisp) {
        set_error(std::string(who) + ": " + std::to_string(n_passes) + " passes over images of this size could pass the "
                  "largest displacement the field takes (2^22 pixels)");
        return MTM_E_INVALID;
    }
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(rows, cols, chans, dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    const BlockValidate V{threshold, 4.0 * epsilon, valid};
    const BlockDeform D{predicted};
    return match_block_passes(c, I, Q, nullptr, method, out, nbhd, valid ? &V : nullptr, nullptr, &D);
}

int mtm_match_blocks_passes_steered(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                    int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                    const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                    mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted, int steer) {
    const char* who = "mtm_match_blocks_passes_steered";
    if (steer != 0 && steer != 1) {
        set_error(std::string(who) + ": steer must be 0 (integer records) or 1 (refined positions) (got " + std::to_string(steer) +
                  ")");
        return MTM_E_INVALID;
    }
    if (steer == 0)
        return mtm_match_blocks_passes_deformed(c, reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans,
                                                dtype, passes, n_passes, method, threshold, epsilon, out, nbhd, valid, predicted);
    if (valid) MTMC(check_validate_args(who, threshold, epsilon));
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_passes >= 1 && passes && out && predicted, method, I));
    if ((long long)n_passes * std::max(rows, cols) > kDeformMaxDisp) {
        set_error(std::string(who) + ": " + std::to_string(n_passes) + " passes over images of this size could pass the "
                  "largest displacement the field takes (2^22 pixels)");
        return MTM_E_INVALID;
    }
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(rows, cols, chans, dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    const BlockValidate V{threshold, 4.0 * epsilon, valid};
    const BlockDeform D{predicted, 1};
    return match_block_passes(c, I, Q, nullptr, method, out, nbhd, valid ? &V : nullptr, nullptr, &D);
}

int mtm_debug_steer_q8(mtm_ctx* c, const mtm_hit* recs, const float* nbhd, const int32_t* predicted, const uint8_t* valid,
                       const mtm_hit* steer_recs, int nx, int ny, int sx, int sy, int mode_min, int smooth, int32_t* out_q8) {
    const char* who = "mtm_debug_steer_q8";
    if (!recs || !nbhd || !predicted || !out_q8 || (valid != nullptr) != (steer_recs != nullptr) || nx < 1 || ny < 1 || sx < 1 ||
        sy < 1 || (long long)nx * ny > INT_MAX / 16) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    const size_t n = (size_t)nx * (size_t)ny;
    mode_min = mode_min ? 1 : 0;
    if (!c) {           // the rule itself, on the host
        std::vector<int32_t> d8(2 * n);
        for (int k = 0; k < (int)n; ++k)
            steer_d8_inl(recs, nbhd, predicted, valid, steer_recs, nx, sx, sy, mode_min, k, &d8[2 * (size_t)k], &d8[2 * (size_t)k + 1]);
        for (int k = 0; k < (int)n; ++k) {
            if (smooth) steer_smooth_inl(d8.data(), nx, ny, k % nx, k / nx, &out_q8[2 * (size_t)k], &out_q8[2 * (size_t)k + 1]);
            else out_q8[2 * (size_t)k] = d8[2 * (size_t)k], out_q8[2 * (size_t)k + 1] = d8[2 * (size_t)k + 1];
        }
        return MTM_OK;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    HIPC(hipSetDevice(c->device));
    MTMC(c->blk_recs.ensure(sizeof(mtm_hit) * n));
    MTMC(c->blk_nbhd.ensure(sizeof(float) * 9 * n));
    MTMC(c->blk_pred.ensure(sizeof(int32_t) * 2 * n));
    MTMC(c->blk_d8.ensure(sizeof(int32_t) * 2 * n));
    MTMC(c->blk_disp.ensure(sizeof(int32_t) * 2 * n));
    if (valid) {
        MTMC(c->blk_valid.ensure(n));
        MTMC(c->blk_steer.ensure(sizeof(mtm_hit) * n));
        HIPC(hipMemcpyAsync(c->blk_valid.p, valid, n, hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(c->blk_steer.p, steer_recs, sizeof(mtm_hit) * n, hipMemcpyHostToDevice, c->stream));
    }
    HIPC(hipMemcpyAsync(c->blk_recs.p, recs, sizeof(mtm_hit) * n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->blk_nbhd.p, nbhd, sizeof(float) * 9 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->blk_pred.p, predicted, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
    const dim3 grd((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(blocks_steer_q8_kernel, grd, dim3(256), 0, c->stream, c->blk_recs.as<mtm_hit>(), c->blk_nbhd.as<float>(),
                       c->blk_pred.as<int32_t>(), valid ? c->blk_valid.as<uint8_t>() : nullptr,
                       valid ? c->blk_steer.as<mtm_hit>() : nullptr, nx, ny, sx, sy, mode_min, c->blk_d8.as<int32_t>());
    HIPC(hipGetLastError());
    if (smooth) {
        hipLaunchKernelGGL(blocks_smooth_q8_kernel, grd, dim3(256), 0, c->stream, c->blk_d8.as<int32_t>(), nx, ny,
                           c->blk_disp.as<int32_t>());
        HIPC(hipGetLastError());
    }
    HIPC(hipMemcpyAsync(out_q8, smooth ? c->blk_disp.p : c->blk_d8.p, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return MTM_OK;
}

// mtm_deform_image (q8 = false: whole-pixel displacements within +-2^22) and mtm_deform_image_q8 (Q8 ones within +-2^30).
static int deform_image_entry(const char* who, bool q8, mtm_ctx* c, const void* px, int64_t row_stride_bytes, int rows, int cols,
                              int chans, int dtype, int bw, int bh, int sx, int sy, const int32_t* displacements, void* out,
                              int64_t out_stride_bytes) {
    if (!displacements || !out) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, who));
    MTMC(check_image_args(out, rows, cols, chans, dtype, out_stride_bytes, who));
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1)) || rows > kBatchMaxRows) {
        set_error(std::string(who) + ": takes uint8 images with 1 or 3 channels and single-channel uint16 images of at most " +
                  std::to_string(kBatchMaxRows) + " rows");
        return MTM_E_INVALID;
    }
    const BlockGrid g = block_grid_of(mtm_block_pass{bw, bh, sx, sy, 0}, rows, cols);
    if (g.nx < 1 || g.ny < 1 || (long long)g.nx * g.ny > INT_MAX / 2) {
        set_error(std::string(who) + ": block and step must be >= 1 and a block must fit the image (fewer than 2^30 of them)");
        return MTM_E_INVALID;
    }
    const size_t n = (size_t)g.nx * (size_t)g.ny;
    const long long dmax = q8 ? kDeformMaxDispQ8 : kDeformMaxDisp;
    for (size_t k = 0; k < 2 * n; ++k)
        if (displacements[k] > dmax || displacements[k] < -dmax) {
            set_error(std::string(who) + ": block " + std::to_string(k / 2) + ": displacement beyond 2^22 pixels");
            return MTM_E_INVALID;
        }
    const size_t es = elem_size(dtype);
    if (!c) {           // the rule itself, on the host
        for (int y = 0; y < rows; ++y) {
            uint8_t* orow = (uint8_t*)out + (size_t)y * (size_t)out_stride_bytes;
            for (int x = 0; x < cols; ++x) {
                long long fx, fy;
                if (q8) deform_field_at_of_inl<true>(g, displacements, 2ll * x, 2ll * y, &fx, &fy);
                else deform_field_at_inl(g, displacements, 2ll * x, 2ll * y, &fx, &fy);
                int x0, x1, wx, y0, y1, wy;
                deform_sample_inl(x, fx, cols, &x0, &x1, &wx);
                deform_sample_inl(y, fy, rows, &y0, &y1, &wy);
                const uint8_t* r0 = (const uint8_t*)px + (size_t)y0 * (size_t)row_stride_bytes;
                const uint8_t* r1 = (const uint8_t*)px + (size_t)y1 * (size_t)row_stride_bytes;
                for (int ch = 0; ch < chans; ++ch) {
                    auto at = [&](const uint8_t* r, int xx) -> uint32_t {
                        const size_t e = (size_t)xx * chans + ch;
                        return es == 2 ? (uint32_t)((const uint16_t*)r)[e] : (uint32_t)r[e];
                    };
                    const uint32_t v = deform_blend_inl(at(r0, x0), at(r0, x1), at(r1, x0), at(r1, x1), wx, wy);
                    const size_t e = (size_t)x * chans + ch;
                    if (es == 2) ((uint16_t*)orow)[e] = (uint16_t)v;
                    else orow[e] = (uint8_t)v;
                }
            }
        }
        return MTM_OK;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    HIPC(hipSetDevice(c->device));
    std::vector<uint32_t> tab;
    deform_tables(g, rows, cols, tab);
    const int pitch = (int)round_up((size_t)cols + kPadCols, 64);
    const size_t wbytes = warp_bytes(rows, pitch, chans, dtype);
    MTMC(c->blk_disp.ensure(sizeof(int32_t) * 2 * n));
    MTMC(c->blk_dtab.ensure(sizeof(uint32_t) * tab.size()));
    MTMC(c->blk_warp.ensure(wbytes));
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    // ONE upload of the image; the warp reads its planes and writes planes of the same layout
    MTMC(upload_image(c, c->slot[c->cur], px, row_stride_bytes, rows, cols, chans, dtype, c->stream, 1));
    adopt_image(c, rows, cols, chans, dtype);
    HIPC(hipMemcpyAsync(c->blk_disp.p, displacements, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->blk_dtab.p, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice, c->stream));
    const ImageDev src = image_dev(c);
    HIPC(hipEventRecord(c->ev[0], c->stream));                  // (the call's time is the warp kernel's)
    MTMC(launch_deform(c, src, c->slot[c->cur].u8b.as<uint8_t>() + src.u8_plane, chans, dtype, g, 0, q8));
    HIPC(hipEventRecord(c->ev[1], c->stream));
    // the planes come back tightly packed; interleaved pixels are put together on the host
    const int np = dtype == MTM_U16 ? 2 : chans;
    const bool direct = np == 1;
    std::vector<uint8_t> planes(direct ? 0 : (size_t)np * rows * cols);
    for (int p = 0; p < np; ++p)
        HIPC(hipMemcpy2DAsync(direct ? out : (void*)(planes.data() + (size_t)p * rows * cols),
                              direct ? (size_t)out_stride_bytes : (size_t)cols, c->blk_warp.as<uint8_t>() + (size_t)p * pitch * rows,
                              (size_t)pitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    const size_t plane = (size_t)rows * cols;
    for (int y = 0; !direct && y < rows; ++y) {
        uint8_t* orow = (uint8_t*)out + (size_t)y * (size_t)out_stride_bytes;
        const uint8_t* q = planes.data() + (size_t)y * cols;
        for (int x = 0; x < cols; ++x) {
            if (dtype == MTM_U16) ((uint16_t*)orow)[x] = (uint16_t)(((uint32_t)q[x] << 8) | ((uint32_t)q[plane + x] ^ 0x80u));
            else
                for (int ch = 0; ch < chans; ++ch) orow[(size_t)x * chans + ch] = q[(size_t)ch * plane + x];
        }
    }
    return MTM_OK;
}

int mtm_deform_image(mtm_ctx* c, const void* px, int64_t row_stride_bytes, int rows, int cols, int chans, int dtype, int bw, int bh,
                     int sx, int sy, const int32_t* displacements, void* out, int64_t out_stride_bytes) {
    return deform_image_entry("mtm_deform_image", false, c, px, row_stride_bytes, rows, cols, chans, dtype, bw, bh, sx, sy,
                              displacements, out, out_stride_bytes);
}

int mtm_deform_image_q8(mtm_ctx* c, const void* px, int64_t row_stride_bytes, int rows, int cols, int chans, int dtype, int bw,
                        int bh, int sx, int sy, const int32_t* displacements_q8, void* out, int64_t out_stride_bytes) {
    return deform_image_entry("mtm_deform_image_q8", true, c, px, row_stride_bytes, rows, cols, chans, dtype, bw, bh, sx, sy,
                              displacements_q8, out, out_stride_bytes);
}

int mtm_match_blocks_second(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                            const int32_t* offsets, int n_blocks, int margin, int method, mtm_hit* out, float* nbhd,
                            int exclusion, mtm_hit* second) {
    const char* who = "mtm_match_blocks_second";
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_blocks >= 0 && margin >= 0 && exclusion >= 0 && second && (n_blocks == 0 || (blocks && out)),
                          method, I));
    std::vector<BlockPassPlan> Q(1);
    Q[0].grid = BlockGrid{};
    Q[0].margin = margin;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, Q[0].plan,
                     false));
    if (n_blocks == 0) return MTM_OK;
    MTMC(fix_block_tiles(Q[0].plan, rows, cols, blocks, margin, who));
    Q[0].blocks.assign(blocks, blocks + n_blocks);
    const BlockSecondOut X2{exclusion, second};
    return match_block_passes(c, I, Q, offsets, method, out, nbhd, nullptr, &X2);
}

int mtm_match_blocks_passes_second(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                   int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                   const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                   mtm_hit* out, float* nbhd, uint8_t* valid, int exclusion, mtm_hit* second) {
    const char* who = "mtm_match_blocks_passes_second";
    if (valid) MTMC(check_validate_args(who, threshold, epsilon));      // (ahead of everything else, as the validated call)
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_passes >= 1 && passes && out && exclusion >= 0 && second, method, I));
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(rows, cols, chans, dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    const BlockValidate V{threshold, 4.0 * epsilon, valid};
    const BlockSecondOut X2{exclusion, second};
    return match_block_passes(c, I, Q, nullptr, method, out, nbhd, valid ? &V : nullptr, &X2);
}

int mtm_debug_second_peaks(mtm_ctx* c, const float* planes, int n, const int32_t* oh, const int32_t* ow, const int32_t* firsts,
                           int mode_min, int exclusion, mtm_hit* out) {
    const char* who = "mtm_debug_second_peaks";
    bool ok = planes && oh && ow && out && n >= 1 && exclusion >= 0 && (mode_min == 0 || mode_min == 1);
    std::vector<long long> poff;
    size_t total = 0;
    for (int k = 0; ok && k < n; ++k) {
        ok = oh[k] >= 1 && ow[k] >= 1 && (long long)oh[k] * ow[k] < (1ll << 32) &&
             (!firsts || (firsts[k] >= 0 && (long long)firsts[k] < (long long)oh[k] * ow[k]));
        poff.push_back((long long)total);
        if (ok) total += (size_t)oh[k] * (size_t)ow[k];
    }
    if (!ok) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    // the first peak of every plane: the cell the caller names, or the largest key of the plane (0: a plane of NaNs)
    std::vector<unsigned long long> first((size_t)n);
    for (int k = 0; k < n; ++k) {
        const float* m = planes + poff[(size_t)k];
        first[(size_t)k] = firsts ? second_cell_key(m[firsts[k]], mode_min, (uint32_t)firsts[k])
                                  : second_scan_inl(m, oh[k], ow[k], 0ull, mode_min, 0);
    }
    if (!c) {           // the rule itself, on the host
        for (int k = 0; k < n; ++k) {
            const unsigned long long f = first[(size_t)k];
            const unsigned long long key2 = f ? second_scan_inl(planes + poff[(size_t)k], oh[k], ow[k], f, mode_min, exclusion) : 0ull;
            out[k] = second_key_record(key2, mode_min, k, 0, 0, ow[k], 0, 0);
        }
        return MTM_OK;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    HIPC(hipSetDevice(c->device));
    std::vector<TrackUnit> units((size_t)n);
    for (int k = 0; k < n; ++k) units[(size_t)k] = TrackUnit{k, 0, 0, oh[k], ow[k]};
    const std::vector<mtm_block> blocks((size_t)n, mtm_block{0, 0, 0, 0});
    const size_t nn = (size_t)n;
    const struct { DevBuf& buf; const void* src; size_t bytes; } up[] = {
        {c->blk_plane, planes, sizeof(float) * total},      {c->blk_poff, poff.data(), sizeof(long long) * nn},
        {c->blk_units, units.data(), sizeof(TrackUnit) * nn}, {c->blk_blocks, blocks.data(), sizeof(mtm_block) * nn},
        {c->blk_keys, first.data(), sizeof(unsigned long long) * nn}};
    for (const auto& u : up) MTMC(u.buf.ensure(u.bytes));
    MTMC(c->blk_keys2.ensure(sizeof(unsigned long long) * nn));
    MTMC(c->blk_recs2.ensure(sizeof(mtm_hit) * nn));
    for (const auto& u : up) HIPC(hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    MTMC(for_launch_slices(0, nn, [&](size_t k0, unsigned nk) -> int {
        hipLaunchKernelGGL(blocks_second_kernel, dim3(nk), dim3(256), 0, c->stream, c->blk_units.as<TrackUnit>(),
                           c->blk_keys.as<unsigned long long>(), c->blk_plane.as<float>(), c->blk_poff.as<long long>(), (int)k0,
                           mode_min, exclusion, c->blk_keys2.as<unsigned long long>());
        HIPC(hipGetLastError());
        return MTM_OK;
    }));
    hipLaunchKernelGGL(blocks_second_record_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, c->stream,
                       c->blk_units.as<TrackUnit>(), c->blk_keys2.as<unsigned long long>(), c->blk_blocks.as<mtm_block>(), n,
                       mode_min, c->blk_recs2.as<mtm_hit>());
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out, c->blk_recs2.p, sizeof(mtm_hit) * nn, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return MTM_OK;
}

int mtm_match_blocks(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                     int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                     int n_blocks, int margin, int method, mtm_hit* out, float* nbhd) {
    const char* who = "mtm_match_blocks";
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_blocks >= 0 && margin >= 0 && (n_blocks == 0 || (blocks && out)), method, I));
    BlockPlan P;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, P));
    if (n_blocks == 0) return MTM_OK;
    const size_t n = (size_t)n_blocks;

    BlockStage S = plan_stage(blocks, P);
    S.nbhd = nbhd != nullptr;
    MTMC(stage_block_call(c, S, [&] { return upload_block_pair(c, I); }));
    unsigned long long* keys = c->blk_keys.as<unsigned long long>();
    MTMC(blocks_pair(c, P, ctx_block_tables(c), rows, chans, dtype, method, 0, 1, true,
                     BlockSink{keys, nbhd ? c->blk_nbhd.as<float>() : nullptr, 0, 0}));

    // the keys (and neighbourhoods) come back behind the call's single wait
    std::vector<unsigned long long> hkeys(n);
    MTMC(finish_block_call(c, {{hkeys.data(), keys, sizeof(unsigned long long) * n}, {nbhd, c->blk_nbhd.p, sizeof(float) * 9 * n}},
                           n));
    decode_block_keys(P, blocks, hkeys.data(), method, out);
    return MTM_OK;
}

int mtm_match_blocks_stack(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, const mtm_block* blocks, int n_blocks, int margin, int method, int mode,
                           mtm_hit* out_hits, float* nbhd, float* planes) {
    const char* who = "mtm_match_blocks_stack";
    MTMC(check_block_entry(c, who,
                           n_frames >= 0 && n_blocks >= 0 && margin >= 0 && (n_frames == 0 || frames) &&
                               (n_blocks == 0 || (blocks && n_frames >= 2 && (out_hits || planes))) &&
                               (mode == MTM_BLOCKS_REF_PREVIOUS || mode == MTM_BLOCKS_REF_FIRST),
                           method));
    for (int f = 0; f < n_frames; ++f) MTMC(check_image_args(frames[f], rows, cols, chans, dtype, row_stride_bytes, who));
    MTMC(check_block_images(who, "frames", rows, chans, dtype));
    BlockPlan P;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, P));
    if (n_blocks == 0) return MTM_OK;
    const bool ens = planes != nullptr;
    if (ens) nbhd = nullptr;
    const size_t n = (size_t)n_blocks, np = (size_t)n_frames - 1;
    const unsigned __int128 side = 2 * (unsigned __int128)margin + 1, cells128 = (unsigned __int128)n * side * side;
    if (ens && (cells128 > (unsigned __int128)c->boxes_max_floats || side > (unsigned __int128)INT_MAX)) {
        const std::string cells_s = cells128 >> 63 ? std::string("2^63 or more") : std::to_string((long long)cells128);
        set_error(std::string(who) + ": the planes of " + std::to_string(n_blocks) + " blocks at margin " +
                  std::to_string(margin) + " hold " + cells_s + " floats, more than MTM_OPT_BOXES_MAX_FLOATS = " +
                  std::to_string((long long)c->boxes_max_floats));
        return MTM_E_INVALID;
    }
    const size_t cells = ens ? (size_t)cells128 : 0;

    // the call's clock starts ahead of the uploads: the frames go up chunk by chunk between the pairs' chains
    BlockStage S = plan_stage(blocks, P);
    S.key_rows = np;
    S.nbhd = nbhd != nullptr;
    S.cells = cells;
    S.clip = ens ? P.clip.data() : nullptr;
    MTMC(stage_block_call(c, S, [] { return MTM_OK; }));

    // mode "first" with every block in one chunk: the gathered templates outlive the pairs of a frame chunk
    const bool gather_once = mode == MTM_BLOCKS_REF_FIRST && P.chunks.size() == 1;
    std::vector<const void*> px;
    // frame chunks sized as a tracking call's, never below two frames (plan_blocks_stack: a pair's reference and image lie
    // in one stack); a frame chunk's upload, then every pair's chain (blocks_pair) in stream order: the next upload
    // overwrites the stack behind this chunk's last reader, and the host waits for none of them
    for (const StackChunk& S : plan_blocks_stack(n_frames, track_chunk_frames(c, rows, cols, chans), mode)) {
        px.assign(1, frames[S.carried]);
        px.insert(px.end(), frames + S.f0, frames + S.f0 + S.nf);
        adopt_image(c, (S.nf + 1) * rows, cols, chans, dtype);
        MTMC(upload_image_stack(c, c->slot[c->cur], px.data(), S.nf + 1, row_stride_bytes, rows, cols, chans, dtype, c->stream));
        for (int i = 0; i < S.nf; ++i) {
            const size_t p = (size_t)(S.p0 + i);
            const BlockSink sink{ens ? nullptr : c->blk_keys.as<unsigned long long>() + p * n,
                                 nbhd ? c->blk_nbhd.as<float>() + 9 * p * n : nullptr, ens ? (int)side : 0, p == 0 ? 1 : 0};
            MTMC(blocks_pair(c, P, ctx_block_tables(c), rows, chans, dtype, method, mode == MTM_BLOCKS_REF_FIRST ? 0 : i, i + 1,
                             !(gather_once && i > 0), sink));
        }
    }

    // the keys (and neighbourhoods), or the planes' sums, come back behind the call's single wait
    std::vector<unsigned long long> hkeys(ens ? 0 : np * n);
    std::vector<double> hacc(cells);
    MTMC(finish_block_call(c, {{ens ? hacc.data() : nullptr, c->blk_acc.p, sizeof(double) * cells},
                               {ens ? nullptr : hkeys.data(), c->blk_keys.p, sizeof(unsigned long long) * np * n},
                               {nbhd, c->blk_nbhd.p, sizeof(float) * 9 * np * n}}, ens ? n : np * n));
    if (ens) {
        // the mean of the pairs in float64, rounded to float32; NaN where the clipped box has no output
        const size_t sd = (size_t)side;
        const double pairs = (double)np;
        for (size_t k = 0; k < n; ++k) {
            const TrackUnit& u = P.units[k];
            const size_t ox = (size_t)P.clip[2 * k], oy = (size_t)P.clip[2 * k + 1];
            for (size_t cy = 0; cy < sd; ++cy)
                for (size_t cx = 0; cx < sd; ++cx) {
                    const size_t i = (k * sd + cy) * sd + cx;
                    const bool in = cy >= oy && cy - oy < (size_t)u.oh && cx >= ox && cx - ox < (size_t)u.ow;
                    planes[i] = in ? (float)(hacc[i] / pairs) : NAN;
                }
        }
    } else {
        for (size_t p = 0; p < np; ++p) decode_block_keys(P, blocks, hkeys.data() + p * n, method, out_hits + p * n);
    }
    return MTM_OK;
}

}  // extern "C"
