// libmtm_hip.so - templates tracked through a stack of frames in one call (mtm_track_boxes): per frame and
// track, the extremum of the track template's score map over the track's search box (what mtm_find_matches_boxes returns
// for that unit in MTM_PEAKS_GLOBAL mode: the scores are win_score_tile's, mtm_k_window.hip.h, the function that kernel
// calls), then the next frame's box from that hit - both on the device, so that the host waits once per call instead of
// twice per frame.  uint8 (1 or 3 channels) and single-channel uint16, unmasked templates
// of one mtm_set_templates call.  The five entry points are one host function, track_boxes: plan_tracks (mtm_host.cpp)
// checks the tracks and lays out the unit and tile tables, stage_tables puts them on the device, track_frame enqueues a
// frame's kernels, finish_track_call reads the results back behind the call's only wait.
// mtm_track_boxes_nbhd also scores the 3 x 3 neighbourhood of every record in its frame's own map (track_nbhd_kernel)
// while the frame is on the device: what mtm_hit_neighbourhoods returns for it.
// mtm_track_boxes_adapt gives every track a template of its own - a copy of its list template in buffers of the call,
// indexed by the track - and blends it with the window of every hit that passes (track_adopt_kernel), its statistics
// recomputed on the device: the same score, update and neighbourhood kernels on per-track tables.
// mtm_track_boxes_reacquire searches every track whose hit did not pass min_score again in the same frame, over the whole
// frame (track_reacquire_kernel over the tracks track_update_kernel listed, then track_reupdate_kernel): the lost tracks
// are found, searched and moved on the device, the host never learns which they are.
// mtm_track_boxes_sets gives every track a set of templates of one shape: one unit per (track, template), groups of up to
// kTrackNV units scored by one work-group that shares the tile's image rows and window sums (track_score_sets_kernel), and
// the frame's record the best unit's, the first in set order on ties (track_set_winner in track_update_kernel).
#include <type_traits>

#include "mtm_ctx.h"
#include "mtm_device_util.hip.h"
#include "mtm_k_nbhd.hip.h"
#include "mtm_k_window.hip.h"
#include "mtm_templ_stats.h"

using namespace mtm;
using namespace mtmi;

namespace mtm {

static_assert(kTrackTile == kWinTile, "plan_tracks tiles the maps as the window kernels walk them");

// TrackUnit, TrackTile (mtm_internal.h): the unit table holds one TrackUnit per (track, template of its set), track after
// track in set order; track k's units are set_off[k] .. set_off[k + 1] - 1, or unit k alone where a kernel is given no
// set_off.  The units of a track share box and shape and differ in `t` alone.  Rewritten by track_update_kernel.

// The state of a frame's whole-frame search (mtm_track_boxes_reacquire), in one buffer: wunits[k] = track k's whole-frame
// unit and flags[k] != 0 while k is lost in the frame being processed; list[0 .. *n_lost - 1] = the lost tracks, in any
// order.  Between two frames every flag and the count are 0.
struct TrackLostState {
    TrackUnit* wunits;
    int* list;
    int* n_lost;
    uint8_t* flags;
};
constexpr unsigned kTrackReacquireGrid = 2048;            // work-groups of a track_reacquire_kernel launch: 8 per CU

// The tile (ty0, tx0) of unit U's map in the frame at rows row_off .. of the stack: win_score_tile's sums and float32
// scores - boxes_score_kernel's bits, the same function -, and instead of a map the tile's best output goes into *slot
// (win_merge_key).  A whole-frame unit has y0 = x0 = 0.
template <int CH, bool U16>
__device__ __forceinline__ void track_score_tile(WinTemplLds (&Tl)[U16 ? 2 : 1], WinImageLds (&Il)[U16 ? 2 : 1],
                                                 const ImageDev& img, const uint8_t* __restrict__ lo_b,
                                                 const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                 const TemplDev* __restrict__ td, const TrackUnit& U, int ty0, int tx0,
                                                 int row_off, int method, int mode_min,
                                                 unsigned long long* __restrict__ slot) {
    const TemplDev T = td[U.t];
    win_score_tile<CH, U16>(Tl, Il, img, lo_b, tpx + toff[U.t], T, row_off + U.y0 + ty0, U.x0 + tx0, ty0, tx0, U.oh, U.ow,
                            method, [&](bool inside, int y, int x, auto&& score) {
                                win_merge_key(inside, win_pos_word(y, x, U.ow), mode_min, score, slot);
                            });
}

// Grid: one work-group per tile of the call's tile table (plain tracks: u0 = the track, nv = 1): the tile's best output
// into keys[u0].  The table covers the largest map the track can have during the call; tiles outside the current map
// leave at once.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_score_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                          const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                          const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units,
                                                          const TrackTile* __restrict__ tiles, int row_off, int method,
                                                          int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const TrackTile K = tiles[blockIdx.x];
    const TrackUnit U = units[K.u0];
    if (K.ty0 >= U.oh || K.tx0 >= U.ow) return;         // (the same for the whole work-group: before any barrier)
    track_score_tile<CH, U16>(Tl, Il, img, lo_b, tpx, toff, td, U, K.ty0, K.tx0, row_off, method, mode_min, keys + K.u0);
}

// The record of a key (quality_key_record, mtm_quality_key.h: what decode_quality_key gives on the host) reduced over the
// map of unit U, in frame coordinates.
__device__ __forceinline__ mtm_hit track_record(const TrackUnit& U, unsigned long long key, int w, int h, int mode_min) {
    return quality_key_record(key, mode_min, U.t, U.y0, U.x0, U.ow, w, h);
}

// U's map becomes that of the hit r widened by `margin` on every side and clipped to the frame (MTM.tracking.next_box).
__device__ __forceinline__ void track_move_box(TrackUnit& U, const mtm_hit& r, int margin, int rows, int cols) {
    const long long x0 = max(0ll, (long long)r.x - margin), y0 = max(0ll, (long long)r.y - margin);
    const long long x1 = min((long long)cols, (long long)r.x + r.w + margin);
    const long long y1 = min((long long)rows, (long long)r.y + r.h + margin);
    U.x0 = (int)x0;
    U.y0 = (int)y0;
    U.ow = (int)(x1 - x0) - r.w + 1;
    U.oh = (int)(y1 - y0) - r.h + 1;
}

// Whether a score passes min_score: below it for the difference methods, above it for the others, compared in double; a
// NaN never passes.
__device__ __forceinline__ bool track_passes(float score, int mode_min, double min_score) {
    const double s = (double)score;
    return mode_min ? s < min_score : s > min_score;
}

// Every unit u0 .. u1 - 1 of a track gets the box around the record r; each keeps its template.
__device__ __forceinline__ void track_move_units(TrackUnit* __restrict__ units, int u0, int u1, const mtm_hit& r,
                                                 int margin, int rows, int cols) {
    TrackUnit U = units[u0];
    track_move_box(U, r, margin, rows, cols);
    for (int u = u0; u < u1; ++u) {
        U.t = units[u].t;
        units[u] = U;
    }
}

// The track's keys are cleared for the next search.
__device__ __forceinline__ void track_clear_keys(unsigned long long* __restrict__ keys, int u0, int u1) {
    for (int u = u0; u < u1; ++u) keys[u] = 0ull;
}

// The unit of keys[u0 .. u1 - 1] that python's max() over the units' scores (min() for the difference methods) returns: the
// first whose quality no later one exceeds, compared as float32 - the position word of a key orders outputs within one
// unit's map and takes no part; -0 equals +0 (mf_float_order stores +0) and a NaN never replaces an earlier unit.  Over
// one unit: that unit.
// (Deliberately not a comparison of the keys' raw high words, as the feature was first specified: the raw word ranks a NaN
// above every number, python's max() / min() - the contract - never let a NaN replace an earlier hit.)
__device__ __forceinline__ int track_set_winner(const unsigned long long* __restrict__ keys, int u0, int u1) {
    int best = u0;
    unsigned long long kb = keys[u0];
    float qb = kb ? mf_order_float((uint32_t)(kb >> 32)) : __builtin_nanf("");
    for (int u = u0 + 1; u < u1; ++u) {
        const unsigned long long ku = keys[u];
        const float q = ku ? mf_order_float((uint32_t)(ku >> 32)) : __builtin_nanf("");
        if (q > qb) {
            best = u;
            qb = q;
        }
    }
    return best;
}

// One lane per track, after the frame's score launches; set_off == nullptr: track k is unit k alone.  The frame's record
// of the track is the winning unit's (track_set_winner; its templ_idx the winner's template) from its key
// (decode_quality_key, mtm_host.cpp; a zero key gives the NaN record), in frame coordinates, into out[k]; a record that
// passes (always, without use_min) moves the box of every unit of the track to the next frame's (MTM.tracking.next_box),
// one that does not leaves it; every key of the track is cleared for the next frame.  `passed` (or nullptr): passed[k] =
// whether the frame's hit moved the box, for track_adopt_kernel.  REACQ (mtm_track_boxes_reacquire): a track whose hit
// did not pass is lost - its flag is set, the whole-frame unit (0, 0, rows - h + 1, cols - w + 1) of its shape written
// and its index appended to the list, at the slot an atomic counter hands out: the list's order differs from run to run,
// the results do not (each unit's extremum is its own atomicMax key).
// (Deliberately one list entry and one whole-frame unit per lost track, capacity the track count, where the feature was
// first specified with an entry per unit and capacity the unit count: the units of a track share shape and box, so their
// whole-frame units would be copies of each other, and the item walk derives the groups from set_off.)
template <bool REACQ>
__global__ __launch_bounds__(256) void track_update_kernel(TrackUnit* __restrict__ units, const int* __restrict__ set_off,
                                                           const TemplDev* __restrict__ td,
                                                           unsigned long long* __restrict__ keys, int n, int mode_min,
                                                           int margin, int use_min, double min_score, int rows, int cols,
                                                           mtm_hit* __restrict__ out, uint8_t* __restrict__ passed,
                                                           TrackLostState L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int u0 = set_off ? set_off[k] : k, u1 = set_off ? set_off[k + 1] : k + 1;
    const int b = track_set_winner(keys, u0, u1);
    const TrackUnit U = units[b];
    const int w = td[U.t].cols, h = td[U.t].rows;
    const mtm_hit r = track_record(U, keys[b], w, h, mode_min);
    out[k] = r;
    const bool pass = !use_min || track_passes(r.score, mode_min, min_score);
    if (passed) passed[k] = pass ? 1 : 0;
    if (pass) {
        track_move_units(units, u0, u1, r, margin, rows, cols);
    } else if constexpr (REACQ) {
        L.wunits[k] = TrackUnit{U.t, 0, 0, rows - h + 1, cols - w + 1};
        L.flags[k] = 1;
        L.list[atomicAdd(L.n_lost, 1)] = k;
    }
    track_clear_keys(keys, u0, u1);
}

// Grid: kTrackReacquireGrid work-groups, whatever the frame lost; after the frame's track_update_kernel<true> on the same
// stream, so every work-group reads the finished list and none waits for another.  Items i = blockIdx.x, + gridDim.x, ..
// below *n_lost * tiles_max: item i is tile i % tiles_max (row-major over the track's own map, 16 x 16 outputs) of the
// lost track list[i / tiles_max]; tiles_max is the tile count of the call's largest whole-frame map, and a tile past
// the track's own count is skipped.  Trip count and skip are the same for the whole work-group (the sums below hold
// barriers); a frame that lost nothing costs each work-group one load.  A tile is scored as track_score_kernel scores it
// (track_score_tile) over the whole-frame unit, with the template of the table the call uses; one atomicMax per wave
// into keys[k], which the first update cleared.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_reacquire_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                              const uint8_t* __restrict__ tpx,
                                                              const long long* __restrict__ toff,
                                                              const TemplDev* __restrict__ td, TrackLostState L,
                                                              unsigned long long tiles_max, int row_off, int method,
                                                              int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const unsigned long long items = (unsigned long long)*L.n_lost * tiles_max;
    for (unsigned long long i = blockIdx.x; i < items; i += gridDim.x) {
        const int k = L.list[i / tiles_max];
        const unsigned long long tile = i % tiles_max;
        TrackUnit U = L.wunits[k];
        U.y0 = U.x0 = 0;                                    // (what a whole-frame unit holds: no origin arithmetic)
        const unsigned long long tiles_x = (unsigned long long)((U.ow + kWinTile - 1) / kWinTile);
        const unsigned long long tiles_y = (unsigned long long)((U.oh + kWinTile - 1) / kWinTile);
        if (tile >= tiles_x * tiles_y) continue;            // (the same for the whole work-group)
        track_score_tile<CH, U16>(Tl, Il, img, lo_b, tpx, toff, td, U, (int)(tile / tiles_x) * kWinTile,
                                  (int)(tile % tiles_x) * kWinTile, row_off, method, mode_min, keys + k);
    }
}

// One lane per track, after the frame's track_reacquire_kernel: a lost track's record becomes the winning unit's over the
// whole-frame keys - out[k] overwritten, passed[k] (or nullptr) evaluated again, the box of every unit of the track moved
// around the record if it passes and kept if not -, its keys and flag are cleared, and the count is reset for the next
// frame (by the first lane: no lane of this kernel reads it).  A track that was not lost is not touched.
__global__ __launch_bounds__(256) void track_reupdate_kernel(TrackUnit* __restrict__ units, const int* __restrict__ set_off,
                                                             const TemplDev* __restrict__ td,
                                                             unsigned long long* __restrict__ keys, int n, int mode_min,
                                                             int margin, double min_score, int rows, int cols,
                                                             mtm_hit* __restrict__ out, uint8_t* __restrict__ passed,
                                                             TrackLostState L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) *L.n_lost = 0;
    if (k >= n || !L.flags[k]) return;
    const int u0 = set_off ? set_off[k] : k, u1 = set_off ? set_off[k + 1] : k + 1;
    const int b = track_set_winner(keys, u0, u1);
    TrackUnit W = L.wunits[k];
    W.t = units[b].t;
    const mtm_hit r = track_record(W, keys[b], td[W.t].cols, td[W.t].rows, mode_min);
    out[k] = r;
    const bool pass = track_passes(r.score, mode_min, min_score);
    if (passed) passed[k] = pass ? 1 : 0;
    if (pass) track_move_units(units, u0, u1, r, margin, rows, cols);
    track_clear_keys(keys, u0, u1);
    L.flags[k] = 0;
}

// Grid: one 256-thread work-group per track (launch slice), after the frame's track_update_kernel: the 3 x 3 neighbourhood
// of the frame's record rec[k] - never of the track unit, which is the next frame's by now - in the frame's own map, into
// out[9 k ..]: sub_nbhd_int's sums and win_score, mtm_hit_neighbourhoods' float32 bits.  `img` is the chunk's stack and
// the frame its rows row_off .. row_off + rows - 1: the planes are entered at the frame's first row and bounded by the
// frame's `rows`, so that windows and pixels outside the frame are NaN and zero whatever its neighbours in the stack hold.
// A record whose own window is outside the frame's map (the decoded all-NaN key) gets nine NaNs and reads no pixel.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_nbhd_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                         const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                         const TemplDev* __restrict__ td, const mtm_hit* __restrict__ rec,
                                                         int row_off, int rows, int method, float* __restrict__ out) {
    constexpr int kKind = U16 ? kSubU16 : kSubU8;
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) SubImageLds Il[U16 ? 2 : 1];
    __shared__ unsigned long long red[4];
    const mtm_hit R = rec[blockIdx.x];
    const TemplDev T = td[R.templ_idx];
    const int tid = threadIdx.x;
    float score = NAN;
    // (the same for the whole work-group: before any barrier)
    if (R.x >= 0 && R.y >= 0 && R.x <= img.cols - T.cols && R.y <= rows - T.rows) {
        const size_t base = (size_t)row_off * img.u8_pitch;
        score = sub_nbhd_int<CH, kKind>(Tl, Il, red, img.u8 + base, img.u8_plane, lo_b + base, img.u8_pitch, rows, img.cols,
                                        tpx + toff[R.templ_idx], nullptr, T, R.x, R.y, method);
    }
    if (tid < 9) out[(size_t)blockIdx.x * 9 + tid] = score;
}

// Grid: one 256-thread work-group per track (launch slice), after the frame's track_update_kernel and, where there is
// one, its track_nbhd_kernel: a track whose hit passed (passed[k]) adopts the hit's window.  Every pixel of its template
// becomes (T (256 - a) + W a + 128) >> 8 in integers (MTM.tracking.blend_template), W the frame's pixel under the hit
// rec[k] - uint8: plane c of the stack at img.u8 + c * plane; uint16: high << 8 | (lo_b ^ 0x80) -, in place in the
// track's planes at tpx + toff[k] ([CH][h][w]; uint16: the high-byte plane, then the low-byte plane, unbiased).  The sums
// of the new template's pixels and of their squares per channel are reduced in uint64 (exact: at most 2^21 uint16 pixels,
// sum v^2 < 2^53) in a fixed order, and thread 0 writes the constants templ_stats_from_sums_inl gives for them - what
// mtm_set_templates would compute for the new template - into td[k]; the fields the box kernels do not read stay.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_adopt_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                          uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                          TemplDev* __restrict__ td, const mtm_hit* __restrict__ rec,
                                                          const uint8_t* __restrict__ passed, int row_off, int rows,
                                                          int method, int blend_a) {
    __shared__ unsigned long long red[4];
    const int k = blockIdx.x;
    if (!passed[k]) return;                 // (the same for the whole work-group: before any barrier)
    const mtm_hit R = rec[k];
    const int h = td[k].rows, w = td[k].cols;
    // (a record always lies inside its frame's map; a window that did not would be read out of bounds)
    if (R.x < 0 || R.y < 0 || R.x > img.cols - w || R.y > rows - h) return;
    const int tid = threadIdx.x;
    const int n = h * w;
    uint8_t* tp = tpx + toff[k];
    const size_t base = (size_t)(row_off + R.y) * img.u8_pitch + (size_t)R.x;
    const uint32_t a = (uint32_t)blend_a, b = 256u - (uint32_t)blend_a;
    unsigned long long s1[CH], s2[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        s1[c] = 0ull;
        s2[c] = 0ull;
        for (int p = tid; p < n; p += 256) {
            const size_t ip = base + (size_t)(p / w) * img.u8_pitch + (size_t)(p % w);
            uint32_t v;
            if constexpr (U16) {
                const uint32_t wv = ((uint32_t)img.u8[ip] << 8) | ((uint32_t)lo_b[ip] ^ 0x80u);
                const uint32_t tv = ((uint32_t)tp[p] << 8) | (uint32_t)tp[(size_t)n + p];
                v = (tv * b + wv * a + 128u) >> 8;
                tp[p] = (uint8_t)(v >> 8);
                tp[(size_t)n + p] = (uint8_t)(v & 255u);
            } else {
                const uint32_t wv = img.u8[(size_t)c * img.u8_plane + ip];
                const size_t tq = (size_t)c * n + p;
                v = ((uint32_t)tp[tq] * b + wv * a + 128u) >> 8;
                tp[tq] = (uint8_t)v;
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
        TemplDev& T = td[k];
#pragma unroll
        for (int c = 0; c < kMaxChans; ++c) T.mean[c] = st.mean[c];
        T.templ_norm = st.templ_norm;
        T.templ_sum2 = st.templ_sum2;
        T.all_ones = st.all_ones;
    }
}

// ---- tracks that carry a set of templates (mtm_track_boxes_sets) -----------------------------------------------------
// A group of up to kTrackNV (mtm_internal.h: 0 B scratch in every instantiation) units of a track is scored by
// one work-group that stages the tile's image rows and forms both window sums once (win_tile_sums_u8_set /
// win_tile_sums_u16_set).

// The tile (ty0, tx0) of map U for the nv templates gu[0 .. nv - 1].t (nv the same for the whole work-group): the fused
// sums, then per template win_score and the key of track_score_tile, one atomicMax per wave and template into gkeys[n].
template <int CH, bool U16>
__device__ __forceinline__ void track_set_tile(WinTemplLds (&Th)[kTrackNV], WinTemplLds (&Tlo)[U16 ? kTrackNV : 1],
                                               WinImageLds (&Il)[U16 ? 2 : 1], const ImageDev& img,
                                               const uint8_t* __restrict__ lo_b, const uint8_t* __restrict__ tpx,
                                               const long long* __restrict__ toff, const TemplDev* __restrict__ td,
                                               const TrackUnit* __restrict__ gu, int nv, const TrackUnit& U, int ty0, int tx0,
                                               int row_off, int method, int mode_min,
                                               unsigned long long* __restrict__ gkeys) {
    const int tid = threadIdx.x;
    int t[kTrackNV];
    const uint8_t* tp[kTrackNV];
#pragma unroll
    for (int n = 0; n < kTrackNV; ++n) {
        t[n] = gu[n < nv ? n : 0].t;
        tp[n] = tpx + toff[t[n]];
    }
    const int h = td[t[0]].rows, w = td[t[0]].cols;
    const double inv_area = 1.0 / ((double)h * (double)w);
    unsigned long long corr[kTrackNV], s2, s1[CH];
    if constexpr (U16)
        win_tile_sums_u16_set<kTrackNV>(Th, Tlo, Il[0], Il[1], img.u8, lo_b, img.u8_pitch, img.rows, img.cols, tp, nv, h, w,
                                        row_off + U.y0 + ty0, U.x0 + tx0, corr, s1[0], s2);
    else
        win_tile_sums_u8_set<CH, kTrackNV>(Th, Il[0], img.u8, img.u8_plane, img.u8_pitch, img.rows, img.cols, tp, nv, h, w,
                                           row_off + U.y0 + ty0, U.x0 + tx0, corr, s1, s2);
    const int y = ty0 + tid / kWinTile, x = tx0 + tid % kWinTile;
    const bool inside = y < U.oh && x < U.ow;
    const unsigned long long pos = win_pos_word(y, x, U.ow);
#pragma unroll
    for (int n = 0; n < kTrackNV; ++n) {
        if (n >= nv) break;             // (the same for the whole work-group)
        const TemplDev& Tn = td[t[n]];
        const unsigned long long cn = corr[n];          // (a scalar: capturing the array costs 8 VGPRs)
        win_merge_key(inside, pos, mode_min, [&] { return win_score<CH>(method, Tn, inv_area, cn, s1, s2); }, gkeys + n);
    }
}

// Grid: one work-group per entry of the call's (track, group, tile) table; track_score_kernel for a group of units.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_score_sets_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                               const uint8_t* __restrict__ tpx,
                                                               const long long* __restrict__ toff,
                                                               const TemplDev* __restrict__ td,
                                                               const TrackUnit* __restrict__ units,
                                                               const TrackTile* __restrict__ tiles, int row_off, int method,
                                                               int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Th[kTrackNV];
    __shared__ __attribute__((aligned(16))) WinTemplLds Tlo[U16 ? kTrackNV : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const TrackTile K = tiles[blockIdx.x];
    const TrackUnit U = units[K.u0];
    if (K.ty0 >= U.oh || K.tx0 >= U.ow) return;         // (the same for the whole work-group: before any barrier)
    track_set_tile<CH, U16>(Th, Tlo, Il, img, lo_b, tpx, toff, td, units + K.u0, K.nv, U, K.ty0, K.tx0, row_off, method,
                            mode_min, keys + K.u0);
}

// track_reacquire_kernel over sets: items i = blockIdx.x, + gridDim.x, .. below *n_lost * groups_max * tiles_max; item i is
// tile i % tiles_max of group (i / tiles_max) % groups_max of the lost track list[i / (tiles_max * groups_max)], scored
// over the track's whole-frame unit by the fused sums.  A group or a tile past the track's own count is skipped, the same
// for the whole work-group.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_reacquire_sets_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                                   const uint8_t* __restrict__ tpx,
                                                                   const long long* __restrict__ toff,
                                                                   const TemplDev* __restrict__ td,
                                                                   const TrackUnit* __restrict__ units,
                                                                   const int* __restrict__ set_off, TrackLostState L,
                                                                   unsigned long long groups_max, unsigned long long tiles_max,
                                                                   int row_off, int method, int mode_min,
                                                                   unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Th[kTrackNV];
    __shared__ __attribute__((aligned(16))) WinTemplLds Tlo[U16 ? kTrackNV : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const unsigned long long per_track = groups_max * tiles_max;
    const unsigned long long items = (unsigned long long)*L.n_lost * per_track;
    for (unsigned long long i = blockIdx.x; i < items; i += gridDim.x) {
        const int k = L.list[i / per_track];
        const unsigned long long g = (i % per_track) / tiles_max, tile = i % tiles_max;
        const int u1 = set_off[k + 1];
        if (g * kTrackNV >= (unsigned long long)(u1 - set_off[k])) continue;        // (the same for the whole work-group)
        const int u0 = set_off[k] + (int)g * kTrackNV;
        const TrackUnit W = L.wunits[k];
        const unsigned long long tiles_x = (unsigned long long)((W.ow + kWinTile - 1) / kWinTile);
        const unsigned long long tiles_y = (unsigned long long)((W.oh + kWinTile - 1) / kWinTile);
        if (tile >= tiles_x * tiles_y) continue;
        track_set_tile<CH, U16>(Th, Tlo, Il, img, lo_b, tpx, toff, td, units + u0, min(kTrackNV, u1 - u0), W,
                                (int)(tile / tiles_x) * kWinTile, (int)(tile % tiles_x) * kWinTile, row_off, method, mode_min,
                                keys + u0);
    }
}

}  // namespace mtm

namespace mtmi {

// Frames per chunk: the row bound of the stacked image (MTM_OPT_BATCH_MAX_ROWS) and the device memory of its planes (raw
// copy, uint8 / byte / float32 planes: at most 10 bytes per pixel and channel); no score maps are held.
int track_chunk_frames(const mtm_ctx* c, int rows, int cols, int chans) {
    const double pitch = (double)round_up((size_t)cols + kPadCols, 64);
    const double per_frame = (double)(rows + kPadRows) * pitch * 10.0 * chans;
    const int by_rows = std::max(1, c->batch_max_rows / rows);
    const int by_mem = (int)std::max(1.0, std::min(1e9, kBatchChunkBytes / per_frame));
    return std::min(by_rows, by_mem);
}

}  // namespace mtmi

namespace {

// The templates of the tracks as the caller holds them - interleaved pixels, tightly packed, track after track - from
// their planes `planar` (track k's at toff[k]: prepare_window_templates' layout).
void unpack_track_templates(const std::vector<uint8_t>& planar, const std::vector<long long>& toff,
                            const std::vector<BlobTempl>& tl, const mtm_box_unit* start, int n_tracks, uint8_t* dst) {
    for (int k = 0; k < n_tracks; ++k) {
        const BlobTempl& t = tl[(size_t)start[k].templ_idx];
        const size_t plane = (size_t)t.rows * t.cols;
        const uint8_t* src = planar.data() + toff[(size_t)k];
        if (t.dtype == MTM_U16) {
            for (size_t p = 0; p < plane; ++p) {
                const uint16_t v = (uint16_t)((unsigned)src[p] << 8 | src[plane + p]);
                std::memcpy(dst + 2 * p, &v, sizeof(v));
            }
            dst += 2 * plane;
        } else {
            for (size_t p = 0; p < plane; ++p)
                for (int ch = 0; ch < t.chans; ++ch) dst[p * t.chans + ch] = src[(size_t)ch * plane + p];
            dst += plane * t.chans;
        }
    }
}

// A tracking call as its entry point states it.  `sets`: mtm_track_boxes_sets (set_off / set_idx are required);
// need_nbhd: `nbhd` is required (mtm_track_boxes_nbhd), elsewhere it is optional; blend_a > 0: per-track templates,
// adopted after every passing hit (templ_out, stats_out optional); reacq: the lost tracks of every frame are searched
// again over the whole frame (use_min is required).
struct TrackArgs {
    const char* who;
    const void* const* frames;
    int n_frames, rows, cols, chans, dtype;
    int64_t row_stride_bytes;
    const mtm_box_unit* start;
    int n_tracks;
    int margin, use_min;
    double min_score;
    mtm_hit* out;
    float* nbhd = nullptr;
    bool need_nbhd = false;
    bool sets = false;
    const int32_t* set_off = nullptr;
    const int32_t* set_idx = nullptr;
    bool reacq = false;
    int blend_a = 0;
    void* templ_out = nullptr;
    double* stats_out = nullptr;
};

// The arguments every entry point has, in the order the ABI states them; an entry point names what it adds.
TrackArgs common_args(const char* who, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                      int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                      double min_score, mtm_hit* out) {
    return TrackArgs{who, frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start, n_tracks, margin, use_min,
                     min_score, out};
}

// What a call's kernels read and write, on the device: the template tables (the template set's, indexed by the list, or -
// adapt - the call's own copies, indexed by the track, with ktoff / kbytes their host layout), the plan's tables
// (set_off: nullptr without sets), keys, records, neighbourhoods, adapt's pass flags and the lost state.
struct TrackTables {
    uint8_t* tpx;
    const long long* toff;
    TemplDev* td;
    TrackUnit* units;
    const TrackTile* tiles;
    const int* set_off;
    unsigned long long* keys;
    mtm_hit* out;
    float* nbhd;
    uint8_t* passed;
    TrackLostState lost;
    std::vector<long long> ktoff;
    size_t kbytes;
};

// f(ch, u16) with the frames' pixel kind as compile-time constants, the kernels' <CH, U16>: ch() channels, u16().
template <class F>
int track_dispatch(int dtype, int chans, F&& f) {
    if (dtype == MTM_U16) return f(std::integral_constant<int, 1>{}, std::true_type{});
    if (chans == 1) return f(std::integral_constant<int, 1>{}, std::false_type{});
    return f(std::integral_constant<int, 3>{}, std::false_type{});
}

// The checks of a call ahead of its tracks.  *nothing: the call has no frame or no track and returns MTM_OK as it is.
int check_track_call(mtm_ctx* c, const TrackArgs& A, bool* nothing) {
    const std::string who = A.who;
    if (!c || A.n_frames < 0 || A.n_tracks < 0 || A.margin < 0 || (A.n_frames > 0 && !A.frames) ||
        (A.n_tracks > 0 && (!A.start || (A.sets && (!A.set_off || !A.set_idx)))) ||
        (A.n_frames > 0 && A.n_tracks > 0 && (!A.out || (A.need_nbhd && !A.nbhd)))) {
        set_error(who + ": bad arguments");
        return MTM_E_INVALID;
    }
    if (A.reacq && !A.use_min) {
        set_error(who + (A.sets ? ": reacquire needs use_min" : ": needs use_min") +
                  " (a track is searched again where its hit does not pass min_score)");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, A.who);
    *nothing = A.n_frames == 0 || A.n_tracks == 0;
    if (*nothing) return MTM_OK;
    for (int f = 0; f < A.n_frames; ++f)
        MTMC(check_image_args(A.frames[f], A.rows, A.cols, A.chans, A.dtype, A.row_stride_bytes, A.who));
    if (!((A.dtype == MTM_U8 && (A.chans == 1 || A.chans == 3)) || (A.dtype == MTM_U16 && A.chans == 1))) {
        set_error(who + ": takes uint8 frames with 1 or 3 channels and single-channel uint16 frames");
        return MTM_E_INVALID;
    }
    if (!c->have_templ) {
        set_error(who + ": no templates set");
        return MTM_E_STATE;
    }
    return MTM_OK;
}

// The lost state of a reacquiring call for n_tracks tracks, in c->trk_lost and zeroed on the stream (all zero between
// frames): [wunits | list | n_lost | flags].
int track_lost_state(mtm_ctx* c, int n_tracks, TrackLostState& lost) {
    const size_t o_list = round_up(sizeof(TrackUnit) * (size_t)n_tracks, 16);
    const size_t o_count = o_list + round_up(sizeof(int) * (size_t)n_tracks, 16);
    const size_t o_flags = o_count + 16, bytes = o_flags + (size_t)n_tracks;
    MTMC(c->trk_lost.ensure(bytes));
    uint8_t* base = c->trk_lost.as<uint8_t>();
    lost = TrackLostState{reinterpret_cast<TrackUnit*>(base), reinterpret_cast<int*>(base + o_list),
                          reinterpret_cast<int*>(base + o_count), base + o_flags};
    HIPC(hipMemsetAsync(base, 0, bytes, c->stream));
    return MTM_OK;
}

// adapt: every track's copy of its list template's planes and constants in the call's own tables, which T names from
// here on; the units name the track instead of the list template.
int stage_track_templates(mtm_ctx* c, const TrackArgs& A, const std::vector<BlobTempl>& tl, TrackPlan& P, TrackTables& T) {
    const size_t n = (size_t)A.n_tracks;
    std::vector<long long> ltoff(tl.size());         // (prepare_window_templates' offsets)
    long long at = 0;
    for (size_t i = 0; i < tl.size(); ++i) {
        ltoff[i] = at;
        at += (long long)tl[i].rows * tl[i].cols * (tl[i].dtype == MTM_U16 ? 2 : tl[i].chans);
    }
    T.ktoff.resize(n);
    for (size_t k = 0; k < n; ++k) {
        T.ktoff[k] = (long long)T.kbytes;
        T.kbytes += P.templ_bytes[k];
    }
    MTMC(c->trk_tpx.ensure(T.kbytes));
    MTMC(c->trk_toff.ensure(sizeof(long long) * n));
    MTMC(c->trk_td.ensure(sizeof(TemplDev) * n));
    MTMC(c->trk_pass.ensure(n));
    for (size_t k = 0; k < n; ++k) {
        const size_t j = (size_t)A.start[k].templ_idx;
        HIPC(hipMemcpyAsync(c->trk_tpx.as<uint8_t>() + T.ktoff[k], T.tpx + ltoff[j], P.templ_bytes[k],
                            hipMemcpyDeviceToDevice, c->stream));
        HIPC(hipMemcpyAsync(c->trk_td.as<TemplDev>() + k, T.td + j, sizeof(TemplDev), hipMemcpyDeviceToDevice, c->stream));
        P.units[k].t = (int)k;
    }
    HIPC(hipMemcpyAsync(c->trk_toff.p, T.ktoff.data(), sizeof(long long) * n, hipMemcpyHostToDevice, c->stream));
    T.tpx = c->trk_tpx.as<uint8_t>();
    T.toff = c->trk_toff.as<long long>();
    T.td = c->trk_td.as<TemplDev>();
    T.passed = c->trk_pass.as<uint8_t>();
    return MTM_OK;
}

// The call's buffers, sized by the plan, and its tables on the device: the lost state (reacq), adapt's per-track copies
// of planes and constants, then - behind the event the call's time counts from - the plan's tables and zeroed keys.
int stage_tables(mtm_ctx* c, const TrackArgs& A, const std::vector<BlobTempl>& tl, TrackPlan& P, TrackTables& T) {
    HIPC(hipSetDevice(c->device));
    MTMC(prepare_window_templates(c, tl));
    MTMC(prepare_box_td(c, tl));
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    const size_t n_out = (size_t)A.n_frames * A.n_tracks, n_sets = (size_t)A.n_tracks + 1;
    MTMC(c->trk_units.ensure(sizeof(TrackUnit) * P.n_units));
    MTMC(c->trk_tiles.ensure(sizeof(TrackTile) * P.tiles.size()));
    MTMC(c->trk_keys.ensure(sizeof(unsigned long long) * P.n_units));
    if (A.sets) MTMC(c->trk_sets.ensure(sizeof(int) * n_sets));
    MTMC(c->trk_out.ensure(sizeof(mtm_hit) * n_out));
    if (A.nbhd) MTMC(c->trk_nbhd.ensure(sizeof(float) * 9 * n_out));
    T = TrackTables{c->win_tpx.as<uint8_t>(), c->win_toff.as<long long>(), c->box_td.as<TemplDev>(),
                    c->trk_units.as<TrackUnit>(), c->trk_tiles.as<TrackTile>(), A.sets ? c->trk_sets.as<int>() : nullptr,
                    c->trk_keys.as<unsigned long long>(), c->trk_out.as<mtm_hit>(), A.nbhd ? c->trk_nbhd.as<float>() : nullptr,
                    nullptr, TrackLostState{nullptr, nullptr, nullptr, nullptr}, {}, 0};
    if (A.reacq) MTMC(track_lost_state(c, A.n_tracks, T.lost));
    if (A.blend_a > 0) MTMC(stage_track_templates(c, A, tl, P, T));
    HIPC(hipEventRecord(c->ev[0], c->stream));
    HIPC(hipMemcpyAsync(c->trk_units.p, P.units.data(), sizeof(TrackUnit) * P.n_units, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->trk_tiles.p, P.tiles.data(), sizeof(TrackTile) * P.tiles.size(), hipMemcpyHostToDevice, c->stream));
    if (A.sets) HIPC(hipMemcpyAsync(c->trk_sets.p, P.set_off.data(), sizeof(int) * n_sets, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(c->trk_keys.p, 0, sizeof(unsigned long long) * P.n_units, c->stream));
    return MTM_OK;
}

// One frame's launch chain - score, update, [reacquire, reupdate], [neighbourhoods], [adopt] - for frame `f` of the call,
// rows row_off .. row_off + rows - 1 of the stack `img`: no upload, no wait.
int track_frame(mtm_ctx* c, const TrackArgs& A, const TrackPlan& P, const TrackTables& T, const ImageDev& img,
                const uint8_t* lo_b, int row_off, int f) {
    const int mode_min = method_mode_min(c->method) ? 1 : 0;
    const int n = A.n_tracks, ublocks = (n + 255) / 256;
    const size_t r0 = (size_t)f * n;
    return track_dispatch(A.dtype, A.chans, [&](auto ch, auto u16) -> int {
        constexpr int CH = decltype(ch)::value;
        constexpr bool U16 = decltype(u16)::value;
        const auto score = A.sets ? track_score_sets_kernel<CH, U16> : track_score_kernel<CH, U16>;
        MTMC(for_launch_slices(0, P.tiles.size(), [&](size_t t0, unsigned nt) -> int {
            hipLaunchKernelGGL(score, dim3(nt), dim3(256), 0, c->stream, img, lo_b, T.tpx, T.toff, T.td, T.units,
                               T.tiles + t0, row_off, c->method, mode_min, T.keys);
            HIPC(hipGetLastError());
            return MTM_OK;
        }));
        const auto update = A.reacq ? track_update_kernel<true> : track_update_kernel<false>;
        hipLaunchKernelGGL(update, dim3(ublocks), dim3(256), 0, c->stream, T.units, T.set_off, T.td, T.keys, n, mode_min,
                           A.margin, A.use_min ? 1 : 0, A.min_score, A.rows, A.cols, T.out + r0, T.passed, T.lost);
        HIPC(hipGetLastError());
        // the frame's lost tracks over the whole frame, then their records and boxes from that search: a fixed grid that
        // finds the list on the device, no wait
        if (A.reacq) {
            if (A.sets)
                hipLaunchKernelGGL((track_reacquire_sets_kernel<CH, U16>), dim3(kTrackReacquireGrid), dim3(256), 0, c->stream,
                                   img, lo_b, T.tpx, T.toff, T.td, T.units, T.set_off, T.lost, P.groups_max, P.tiles_max,
                                   row_off, c->method, mode_min, T.keys);
            else
                hipLaunchKernelGGL((track_reacquire_kernel<CH, U16>), dim3(kTrackReacquireGrid), dim3(256), 0, c->stream, img,
                                   lo_b, T.tpx, T.toff, T.td, T.lost, P.tiles_max, row_off, c->method, mode_min, T.keys);
            HIPC(hipGetLastError());
            hipLaunchKernelGGL(track_reupdate_kernel, dim3(ublocks), dim3(256), 0, c->stream, T.units, T.set_off, T.td, T.keys,
                               n, mode_min, A.margin, A.min_score, A.rows, A.cols, T.out + r0, T.passed, T.lost);
            HIPC(hipGetLastError());
        }
        // the frame's neighbourhoods, from its records (a set's winner names its template there) and its rows of the stack
        if (T.nbhd)
            MTMC(for_launch_slices(0, (size_t)n, [&](size_t k0, unsigned nk) -> int {
                hipLaunchKernelGGL((track_nbhd_kernel<CH, U16>), dim3(nk), dim3(256), 0, c->stream, img, lo_b, T.tpx, T.toff,
                                   T.td, T.out + r0 + k0, row_off, A.rows, c->method, T.nbhd + 9 * (r0 + k0));
                HIPC(hipGetLastError());
                return MTM_OK;
            }));
        // the passing tracks adopt their hits' windows: the templates of the next frame's search
        if (A.blend_a > 0)
            MTMC(for_launch_slices(0, (size_t)n, [&](size_t k0, unsigned nk) -> int {
                hipLaunchKernelGGL((track_adopt_kernel<CH, U16>), dim3(nk), dim3(256), 0, c->stream, img, lo_b, T.tpx,
                                   T.toff + k0, T.td + k0, T.out + r0 + k0, T.passed + k0, row_off, A.rows, c->method,
                                   A.blend_a);
                HIPC(hipGetLastError());
                return MTM_OK;
            }));
        return MTM_OK;
    });
}

// Behind the last frame: the records (and neighbourhoods, adapt's templates and constants) come back behind the call's
// single wait; adapt's records name the list template again, its templates are unpacked and their statistics laid out.
int finish_track_call(mtm_ctx* c, const TrackArgs& A, const std::vector<BlobTempl>& tl, const TrackTables& T) {
    const size_t n_out = (size_t)A.n_frames * A.n_tracks;
    const bool adapt = A.blend_a > 0;
    HIPC(hipEventRecord(c->ev[1], c->stream));
    HIPC(hipMemcpyAsync(A.out, T.out, sizeof(mtm_hit) * n_out, hipMemcpyDeviceToHost, c->stream));
    if (A.nbhd) HIPC(hipMemcpyAsync(A.nbhd, T.nbhd, sizeof(float) * 9 * n_out, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> kplanar;
    std::vector<TemplDev> ktd;
    if (adapt && A.templ_out) {
        kplanar.resize(T.kbytes);
        HIPC(hipMemcpyAsync(kplanar.data(), T.tpx, T.kbytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (adapt && A.stats_out) {
        ktd.resize((size_t)A.n_tracks);
        HIPC(hipMemcpyAsync(ktd.data(), T.td, sizeof(TemplDev) * (size_t)A.n_tracks, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    c->timing.n_hits = (int64_t)n_out;
    if (adapt) {
        // the records name the track (the kernels' tables are the call's own): back to the list index
        for (size_t i = 0; i < n_out; ++i) A.out[i].templ_idx = A.start[i % (size_t)A.n_tracks].templ_idx;
        if (A.templ_out)
            unpack_track_templates(kplanar, T.ktoff, tl, A.start, A.n_tracks, static_cast<uint8_t*>(A.templ_out));
        for (int k = 0; A.stats_out && k < A.n_tracks; ++k) {
            const TemplDev& d = ktd[(size_t)k];
            double* o = A.stats_out + 7 * (size_t)k;
            for (int ch = 0; ch < 4; ++ch) o[ch] = d.mean[ch];
            o[4] = d.templ_norm;
            o[5] = d.templ_sum2;
            o[6] = (double)d.all_ones;
        }
    }
    // the stack is none of the caller's frames: no current image, no published maps
    c->have_image = false;
    return MTM_OK;
}

// The five entry points: checks, plan, tables, then chunks of frames as one stacked image (frame f of the chunk at rows
// f * rows ..), the unit table carried across them on the device: the stream orders a chunk's upload behind the previous
// chunk's launches, the host never waits before finish_track_call.
int track_boxes(mtm_ctx* c, const TrackArgs& A) {
    bool nothing = false;
    MTMC(check_track_call(c, A, &nothing));
    if (nothing) return MTM_OK;
    std::vector<BlobTempl> tl;
    MTMC(parse_templ_blob(c->templ_blob, tl, A.who, true));
    TrackPlan P;
    MTMC(plan_tracks(tl, A.rows, A.cols, A.chans, A.dtype, A.start, A.n_tracks, A.margin, A.reacq,
                     A.sets ? A.set_off : nullptr, A.set_idx, A.who, P));
    TrackTables T;
    MTMC(stage_tables(c, A, tl, P, T));
    const int per_chunk = track_chunk_frames(c, A.rows, A.cols, A.chans);
    for (int f0 = 0; f0 < A.n_frames; f0 += per_chunk) {
        const int nb = std::min(per_chunk, A.n_frames - f0);
        adopt_image(c, nb * A.rows, A.cols, A.chans, A.dtype);
        MTMC(upload_image_stack(c, c->slot[c->cur], A.frames + f0, nb, A.row_stride_bytes, A.rows, A.cols, A.chans, A.dtype,
                                c->stream));
        const ImageDev img = image_dev(c);
        const uint8_t* lo_b = c->slot[c->cur].u8b.as<uint8_t>() + img.u8_plane;     // uint16: [high ^ 0x80][low ^ 0x80]
        for (int fl = 0; fl < nb; ++fl) MTMC(track_frame(c, A, P, T, img, lo_b, fl * A.rows, f0 + fl));
    }
    return finish_track_call(c, A, tl, T);
}

}  // namespace

extern "C" {

int mtm_track_boxes(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                    int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                    double min_score, mtm_hit* out) {
    TrackArgs A = common_args("mtm_track_boxes", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                              n_tracks, margin, use_min, min_score, out);
    return track_boxes(c, A);
}

int mtm_track_boxes_nbhd(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                         int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                         double min_score, mtm_hit* out, float* nbhd) {
    TrackArgs A = common_args("mtm_track_boxes_nbhd", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                              n_tracks, margin, use_min, min_score, out);
    A.nbhd = nbhd;
    A.need_nbhd = true;
    return track_boxes(c, A);
}

int mtm_track_boxes_adapt(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                          int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                          double min_score, mtm_hit* out, float* nbhd, int blend_a, void* templ_out, double* stats_out) {
    if (blend_a < 1 || blend_a > 256) {
        set_error("mtm_track_boxes_adapt: blend_a outside 1 .. 256");
        return MTM_E_INVALID;
    }
    TrackArgs A = common_args("mtm_track_boxes_adapt", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                              n_tracks, margin, use_min, min_score, out);
    A.nbhd = nbhd;
    A.blend_a = blend_a;
    A.templ_out = templ_out;
    A.stats_out = stats_out;
    return track_boxes(c, A);
}

int mtm_track_boxes_reacquire(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                              int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                              double min_score, mtm_hit* out, float* nbhd, int blend_a, void* templ_out, double* stats_out) {
    if (blend_a < 0 || blend_a > 256) {
        set_error("mtm_track_boxes_reacquire: blend_a outside 0 .. 256");
        return MTM_E_INVALID;
    }
    TrackArgs A = common_args("mtm_track_boxes_reacquire", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                              n_tracks, margin, use_min, min_score, out);
    A.nbhd = nbhd;
    A.reacq = true;
    A.blend_a = blend_a;
    A.templ_out = templ_out;
    A.stats_out = stats_out;
    return track_boxes(c, A);
}

int mtm_track_boxes_sets(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                         int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, const int32_t* set_off,
                         const int32_t* set_idx, int margin, int use_min, double min_score, int reacquire, mtm_hit* out,
                         float* nbhd) {
    TrackArgs A = common_args("mtm_track_boxes_sets", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                              n_tracks, margin, use_min, min_score, out);
    A.nbhd = nbhd;
    A.sets = true;
    A.set_off = set_off;
    A.set_idx = set_idx;
    A.reacq = reacquire != 0;
    return track_boxes(c, A);
}

}  // extern "C"
