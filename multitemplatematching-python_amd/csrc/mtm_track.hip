// libmtm_hip.so - templates tracked through a stack of frames in one call (mtm_track_boxes): per frame and
// track, the extremum of the track template's score map over the track's search box (what mtm_find_matches_boxes returns
// for that unit in MTM_PEAKS_GLOBAL mode), then the next frame's box from that hit - both on the device, so that the host
// waits once per call instead of twice per frame.  uint8 (1 or 3 channels) and single-channel uint16, unmasked templates
// of one mtm_set_templates call.  mtm_track_boxes_nbhd also scores the 3 x 3 neighbourhood of every record in its frame's
// own map (track_nbhd_kernel) while the frame is on the device: what mtm_hit_neighbourhoods returns for it.
// mtm_track_boxes_adapt gives every track a template of its own - a copy of its list template in buffers of the call,
// indexed by the track - and blends it with the window of every hit that passes (track_adopt_kernel), its statistics
// recomputed on the device: the same score, update and neighbourhood kernels on per-track tables.
// mtm_track_boxes_reacquire searches every track whose hit did not pass min_score again in the same frame, over the whole
// frame (track_reacquire_kernel over the tracks track_update_kernel listed, then track_reupdate_kernel): the lost tracks
// are found, searched and moved on the device, the host never learns which they are.
// mtm_track_boxes_sets gives every track a set of templates of one shape: one unit per (track, template), groups of up to
// kTrackNV units scored by one work-group that shares the tile's image rows and window sums (track_score_sets_kernel), and
// the frame's record the best unit's, the first in set order on ties (track_update_sets_kernel).
#include "mtm_ctx.h"
#include "mtm_device_util.hip.h"
#include "mtm_k_nbhd.hip.h"
#include "mtm_k_window.hip.h"
#include "mtm_templ_stats.h"

using namespace mtm;
using namespace mtmi;

namespace mtm {

// A track as the kernels see it: its template, the frame pixel of its map's output (0, 0) and the map's size.  Frame
// coordinates: the score kernel adds the frame's row offset in the chunk's stack.  Rewritten by track_update_kernel.
struct TrackUnit {
    int t;
    int y0, x0;
    int oh, ow;
};

// One 16 x 16 tile of outputs of track k, first output (ty0, tx0) of its map.  The table covers the largest map the track
// can have during the call; tiles outside the current map leave at once.
struct TrackTile {
    int k, ty0, tx0;
};
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
constexpr size_t kTrackLaunchTiles = (size_t)1 << 22;     // most work-groups (tiles) of one track_score_kernel launch
constexpr size_t kTrackLaunchNbhd = (size_t)1 << 22;      // most work-groups (tracks) of one track_nbhd_kernel launch

// Grid: one work-group per tile of the call's tile table.  The tile's windows are summed and scored exactly as
// boxes_score_kernel does (win_tile_sums_u8 / win_tile_sums_u16, win_score: the same float32 bits), and instead of a map
// the tile's best output goes into keys[k]: order(quality) << 32 | ~(index in the track's current map), reduced per wave
// and merged with one atomicMax per wave, as boxes_peaks_kernel keys a unit's extremum in global mode.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_score_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                          const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                          const TemplDev* __restrict__ td, const TrackUnit* __restrict__ units,
                                                          const TrackTile* __restrict__ tiles, int row_off, int method,
                                                          int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const TrackTile K = tiles[blockIdx.x];
    const TrackUnit U = units[K.k];
    if (K.ty0 >= U.oh || K.tx0 >= U.ow) return;         // (the same for the whole work-group: before any barrier)
    const TemplDev T = td[U.t];
    const int h = T.rows, w = T.cols;
    const uint8_t* tp = tpx + toff[U.t];
    const int tid = threadIdx.x;
    const double inv_area = 1.0 / ((double)h * (double)w);
    unsigned long long corr, s2, s1[CH];
    if constexpr (U16)
        win_tile_sums_u16(Tl[0], Tl[1], Il[0], Il[1], img.u8, lo_b, img.u8_pitch, img.rows, img.cols, tp, h, w,
                          row_off + U.y0 + K.ty0, U.x0 + K.tx0, corr, s1[0], s2);
    else
        win_tile_sums_u8<CH>(Tl[0], Il[0], img.u8, img.u8_plane, img.u8_pitch, img.rows, img.cols, tp, h, w,
                             row_off + U.y0 + K.ty0, U.x0 + K.tx0, corr, s1, s2);
    const int y = K.ty0 + tid / kWinTile, x = K.tx0 + tid % kWinTile;
    unsigned long long key = 0ull;
    if (y < U.oh && x < U.ow) {
        const float s = win_score<CH>(method, T, inv_area, corr, s1, s2);
        const float v = mode_min ? -s : s;
        key = ((unsigned long long)mf_float_order(v) << 32) | (0xFFFFFFFFull - (unsigned long long)((long long)y * U.ow + x));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0 && key != 0ull) atomicMax(keys + K.k, key);
}

// The record of a key (decode_quality_key, mtm_host.cpp) reduced over the map of unit U, in frame coordinates.
__device__ __forceinline__ mtm_hit track_record(const TrackUnit& U, unsigned long long key, int w, int h, int mode_min) {
    const float q = mf_order_float((uint32_t)(key >> 32));
    const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    mtm_hit r;
    r.templ_idx = U.t;
    r.x = U.x0 + (int)(idx % (uint32_t)U.ow);
    r.y = U.y0 + (int)(idx / (uint32_t)U.ow);
    r.w = w;
    r.h = h;
    r.score = key ? (mode_min ? -q : q) + 0.0f : __builtin_nanf("");
    return r;
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

// One lane per track, after the frame's score launch: the frame's record of the track from its key (decode_quality_key,
// mtm_host.cpp), in frame coordinates, into out[k]; the next frame's box (MTM.tracking.next_box: the hit widened by
// `margin` on every side, clipped to the frame; kept when use_min is set and the score does not pass min_score - below it
// for the difference methods, above it for the others, never when NaN); the key cleared for the next frame.  `passed`
// (or nullptr): passed[k] = whether the frame's hit moved the box, for track_adopt_kernel.  REACQ
// (mtm_track_boxes_reacquire): a track whose hit did not pass is lost - its flag is set, its whole-frame unit (0, 0,
// rows - h + 1, cols - w + 1) written and its index appended to the list, at the slot an atomic counter hands out: the
// list's order differs from run to run, the results do not (each track's extremum is its own atomicMax key).
template <bool REACQ>
__global__ __launch_bounds__(256) void track_update_kernel(TrackUnit* __restrict__ units, const TemplDev* __restrict__ td,
                                                           unsigned long long* __restrict__ keys, int n, int mode_min,
                                                           int margin, int use_min, double min_score, int rows, int cols,
                                                           mtm_hit* __restrict__ out, uint8_t* __restrict__ passed,
                                                           TrackLostState L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    TrackUnit U = units[k];
    const int w = td[U.t].cols, h = td[U.t].rows;
    const mtm_hit r = track_record(U, keys[k], w, h, mode_min);
    out[k] = r;
    const double s = (double)r.score;
    const bool pass = !use_min || (mode_min ? s < min_score : s > min_score);
    if (passed) passed[k] = pass ? 1 : 0;
    if (pass) {
        track_move_box(U, r, margin, rows, cols);
        units[k] = U;
    } else if constexpr (REACQ) {
        L.wunits[k] = TrackUnit{U.t, 0, 0, rows - h + 1, cols - w + 1};
        L.flags[k] = 1;
        L.list[atomicAdd(L.n_lost, 1)] = k;
    }
    keys[k] = 0ull;
}

// Grid: kTrackReacquireGrid work-groups, whatever the frame lost; after the frame's track_update_kernel<true> on the same
// stream, so every work-group reads the finished list and none waits for another.  Items i = blockIdx.x, + gridDim.x, ..
// below *n_lost * tiles_max: item i is tile i % tiles_max (row-major over the track's own map, 16 x 16 outputs) of the
// lost track list[i / tiles_max]; tiles_max is the tile count of the call's largest whole-frame map, and a tile past
// the track's own count is skipped.  Trip count and skip are the same for the whole work-group (the sums below hold
// barriers); a frame that lost nothing costs each work-group one load.  A tile is scored as track_score_kernel scores it
// - the same sums, win_score and key - over the whole-frame unit, with the template of the table the call uses; one
// atomicMax per wave into keys[k], which the first update cleared.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_reacquire_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                              const uint8_t* __restrict__ tpx,
                                                              const long long* __restrict__ toff,
                                                              const TemplDev* __restrict__ td, TrackLostState L,
                                                              unsigned long long tiles_max, int row_off, int method,
                                                              int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const int tid = threadIdx.x;
    const unsigned long long items = (unsigned long long)*L.n_lost * tiles_max;
    for (unsigned long long i = blockIdx.x; i < items; i += gridDim.x) {
        const int k = L.list[i / tiles_max];
        const unsigned long long tile = i % tiles_max;
        const TrackUnit U = L.wunits[k];
        const unsigned long long tiles_x = (unsigned long long)((U.ow + kWinTile - 1) / kWinTile);
        const unsigned long long tiles_y = (unsigned long long)((U.oh + kWinTile - 1) / kWinTile);
        if (tile >= tiles_x * tiles_y) continue;            // (the same for the whole work-group)
        const int ty0 = (int)(tile / tiles_x) * kWinTile, tx0 = (int)(tile % tiles_x) * kWinTile;
        const TemplDev T = td[U.t];
        const int h = T.rows, w = T.cols;
        const uint8_t* tp = tpx + toff[U.t];
        const double inv_area = 1.0 / ((double)h * (double)w);
        unsigned long long corr, s2, s1[CH];
        if constexpr (U16)
            win_tile_sums_u16(Tl[0], Tl[1], Il[0], Il[1], img.u8, lo_b, img.u8_pitch, img.rows, img.cols, tp, h, w,
                              row_off + ty0, tx0, corr, s1[0], s2);
        else
            win_tile_sums_u8<CH>(Tl[0], Il[0], img.u8, img.u8_plane, img.u8_pitch, img.rows, img.cols, tp, h, w,
                                 row_off + ty0, tx0, corr, s1, s2);
        const int y = ty0 + tid / kWinTile, x = tx0 + tid % kWinTile;
        unsigned long long key = 0ull;
        if (y < U.oh && x < U.ow) {
            const float s = win_score<CH>(method, T, inv_area, corr, s1, s2);
            const float v = mode_min ? -s : s;
            key = ((unsigned long long)mf_float_order(v) << 32) |
                  (0xFFFFFFFFull - (unsigned long long)((long long)y * U.ow + x));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off);
            key = o > key ? o : key;
        }
        if ((tid & 63) == 0 && key != 0ull) atomicMax(keys + k, key);
    }
}

// One lane per track, after the frame's track_reacquire_kernel: a lost track's record becomes the one its key holds over
// its whole-frame unit - out[k] overwritten, passed[k] (or nullptr) evaluated again, the box moved around the record if it
// passes and kept if not -, its key and flag are cleared, and the count is reset for the next frame (by the first lane:
// no lane of this kernel reads it).  A track that was not lost is not touched.
__global__ __launch_bounds__(256) void track_reupdate_kernel(TrackUnit* __restrict__ units, const TemplDev* __restrict__ td,
                                                             unsigned long long* __restrict__ keys, int n, int mode_min,
                                                             int margin, double min_score, int rows, int cols,
                                                             mtm_hit* __restrict__ out, uint8_t* __restrict__ passed,
                                                             TrackLostState L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) *L.n_lost = 0;
    if (k >= n || !L.flags[k]) return;
    const TrackUnit W = L.wunits[k];
    const mtm_hit r = track_record(W, keys[k], td[W.t].cols, td[W.t].rows, mode_min);
    out[k] = r;
    const double s = (double)r.score;
    const bool pass = mode_min ? s < min_score : s > min_score;
    if (passed) passed[k] = pass ? 1 : 0;
    if (pass) {
        TrackUnit U = units[k];
        track_move_box(U, r, margin, rows, cols);
        units[k] = U;
    }
    keys[k] = 0ull;
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
// The unit table holds one TrackUnit per (track, template of its set), track after track in set order; track k's units
// are set_off[k] .. set_off[k + 1] - 1.  The templates of a set are of one shape and share the track's box, so the units
// of a track differ in `t` alone, and a group of up to kTrackNV of them is scored by one work-group that stages the
// tile's image rows and forms both window sums once (win_tile_sums_u8_set / win_tile_sums_u16_set).
constexpr int kTrackNV = 4;         // templates per group: 0 B scratch in every instantiation

// One 16 x 16 tile of outputs of the units u0 .. u0 + nv - 1 (one group of one track), first output (ty0, tx0).
struct TrackSetTile {
    int u0, nv, ty0, tx0;
};

// The tile (ty0, tx0) of map U for the nv templates gu[0 .. nv - 1].t (nv the same for the whole work-group): the fused
// sums, then per template win_score and the key of track_score_kernel, one atomicMax per wave and template into gkeys[n].
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
    const unsigned long long pos = 0xFFFFFFFFull - (unsigned long long)((long long)y * U.ow + x);
#pragma unroll
    for (int n = 0; n < kTrackNV; ++n) {
        if (n >= nv) break;             // (the same for the whole work-group)
        unsigned long long key = 0ull;
        if (inside) {
            const float s = win_score<CH>(method, td[t[n]], inv_area, corr[n], s1, s2);
            const float v = mode_min ? -s : s;
            key = ((unsigned long long)mf_float_order(v) << 32) | pos;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off);
            key = o > key ? o : key;
        }
        if ((tid & 63) == 0 && key != 0ull) atomicMax(gkeys + n, key);
    }
}

// Grid: one work-group per entry of the call's (track, group, tile) table; track_score_kernel for a group of units.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void track_score_sets_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                               const uint8_t* __restrict__ tpx,
                                                               const long long* __restrict__ toff,
                                                               const TemplDev* __restrict__ td,
                                                               const TrackUnit* __restrict__ units,
                                                               const TrackSetTile* __restrict__ tiles, int row_off, int method,
                                                               int mode_min, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Th[kTrackNV];
    __shared__ __attribute__((aligned(16))) WinTemplLds Tlo[U16 ? kTrackNV : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const TrackSetTile K = tiles[blockIdx.x];
    const TrackUnit U = units[K.u0];
    if (K.ty0 >= U.oh || K.tx0 >= U.ow) return;         // (the same for the whole work-group: before any barrier)
    track_set_tile<CH, U16>(Th, Tlo, Il, img, lo_b, tpx, toff, td, units + K.u0, K.nv, U, K.ty0, K.tx0, row_off, method,
                            mode_min, keys + K.u0);
}

// The unit of keys[u0 .. u1 - 1] that python's max() over the units' scores (min() for the difference methods) returns: the
// first whose quality no later one exceeds, compared as float32 - the position word of a key orders outputs within one
// unit's map and takes no part; -0 equals +0 (mf_float_order stores +0) and a NaN never replaces an earlier unit.
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

// One lane per track, after the frame's score launches: track_update_kernel over the track's units - the record is the
// winning unit's (track_set_winner), its templ_idx the winner's template; a passing record moves the box of every unit of
// the track; every key of the track is cleared.  REACQ: a failing track is listed once, with the whole-frame unit its
// set's shape gives (L.wunits[k]; the templates are those of the track's units).
// (Deliberately one list entry and one whole-frame unit per lost track, capacity the track count, where the feature was
// first specified with an entry per unit and capacity the unit count: the units of a track share shape and box, so their
// whole-frame units would be copies of each other, and the item walk derives the groups from set_off.)
template <bool REACQ>
__global__ __launch_bounds__(256) void track_update_sets_kernel(TrackUnit* __restrict__ units, const int* __restrict__ set_off,
                                                                const TemplDev* __restrict__ td,
                                                                unsigned long long* __restrict__ keys, int n, int mode_min,
                                                                int margin, int use_min, double min_score, int rows, int cols,
                                                                mtm_hit* __restrict__ out, TrackLostState L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int u0 = set_off[k], u1 = set_off[k + 1];
    const int b = track_set_winner(keys, u0, u1);
    TrackUnit U = units[b];
    const int w = td[U.t].cols, h = td[U.t].rows;
    const mtm_hit r = track_record(U, keys[b], w, h, mode_min);
    out[k] = r;
    const double s = (double)r.score;
    const bool pass = !use_min || (mode_min ? s < min_score : s > min_score);
    if (pass) {
        track_move_box(U, r, margin, rows, cols);
        for (int u = u0; u < u1; ++u) {
            U.t = units[u].t;
            units[u] = U;
        }
    } else if constexpr (REACQ) {
        L.wunits[k] = TrackUnit{U.t, 0, 0, rows - h + 1, cols - w + 1};
        L.flags[k] = 1;
        L.list[atomicAdd(L.n_lost, 1)] = k;
    }
    for (int u = u0; u < u1; ++u) keys[u] = 0ull;
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

// track_reupdate_kernel over sets: a lost track's record becomes the winning unit's over the whole-frame keys; a passing
// one moves every unit of the track.  A track that was not lost is not touched; flags and count are zero afterwards.
__global__ __launch_bounds__(256) void track_reupdate_sets_kernel(TrackUnit* __restrict__ units,
                                                                  const int* __restrict__ set_off,
                                                                  const TemplDev* __restrict__ td,
                                                                  unsigned long long* __restrict__ keys, int n, int mode_min,
                                                                  int margin, double min_score, int rows, int cols,
                                                                  mtm_hit* __restrict__ out, TrackLostState L) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k == 0) *L.n_lost = 0;
    if (k >= n || !L.flags[k]) return;
    const int u0 = set_off[k], u1 = set_off[k + 1];
    const int b = track_set_winner(keys, u0, u1);
    TrackUnit W = L.wunits[k];
    W.t = units[b].t;
    const mtm_hit r = track_record(W, keys[b], td[W.t].cols, td[W.t].rows, mode_min);
    out[k] = r;
    const double s = (double)r.score;
    if (mode_min ? s < min_score : s > min_score) {
        TrackUnit U = units[u0];
        track_move_box(U, r, margin, rows, cols);
        for (int u = u0; u < u1; ++u) {
            U.t = units[u].t;
            units[u] = U;
        }
    }
    for (int u = u0; u < u1; ++u) keys[u] = 0ull;
    L.flags[k] = 0;
}

}  // namespace mtm

namespace {

// Frames per chunk: the row bound of the stacked image (MTM_OPT_BATCH_MAX_ROWS) and the device memory of its planes (raw
// copy, uint8 / byte / float32 planes: at most 10 bytes per pixel and channel); no score maps are held.
int track_chunk_frames(const mtm_ctx* c, int rows, int cols, int chans) {
    const double pitch = (double)round_up((size_t)cols + kPadCols, 64);
    const double per_frame = (double)(rows + kPadRows) * pitch * 10.0 * chans;
    const int by_rows = std::max(1, c->batch_max_rows / rows);
    const int by_mem = (int)std::max(1.0, std::min(1e9, kBatchChunkBytes / per_frame));
    return std::min(by_rows, by_mem);
}

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

// A frame's neighbourhoods, from its records c->trk_out[r0 .. r0 + n_tracks - 1] and its rows of the stack, into
// c->trk_nbhd: no upload, no wait.
int track_launch_nbhd(mtm_ctx* c, const ImageDev& img, const uint8_t* lo_b, const uint8_t* tpx, const long long* toff,
                      const TemplDev* td, size_t r0, int n_tracks, int row_off, int rows, int chans, int dtype) {
#define MTM_TRACK_NBHD(CH, U16)                                                                                              \
    hipLaunchKernelGGL((track_nbhd_kernel<CH, U16>), dim3(nk), dim3(256), 0, c->stream, img, lo_b, tpx, toff, td,             \
                       c->trk_out.as<mtm_hit>() + r0 + k0, row_off, rows, c->method,                                         \
                       c->trk_nbhd.as<float>() + 9 * (r0 + k0))
    for (size_t k0 = 0; k0 < (size_t)n_tracks; k0 += kTrackLaunchNbhd) {
        const unsigned nk = (unsigned)std::min(kTrackLaunchNbhd, (size_t)n_tracks - k0);
        if (dtype == MTM_U16) MTM_TRACK_NBHD(1, true);
        else if (chans == 1) MTM_TRACK_NBHD(1, false);
        else MTM_TRACK_NBHD(3, false);
        HIPC(hipGetLastError());
    }
#undef MTM_TRACK_NBHD
    return MTM_OK;
}

// mtm_track_boxes (nbhd == nullptr, with_nbhd false), mtm_track_boxes_nbhd (with_nbhd: `nbhd` is required) and
// mtm_track_boxes_adapt (blend_a > 0: per-track templates, adopted after every passing hit; nbhd, templ_out and stats_out
// optional), and mtm_track_boxes_reacquire (reacq: any of the above - blend_a >= 0, nbhd optional - with the lost
// tracks of every frame searched again over the whole frame; use_min is required).
int track_boxes(mtm_ctx* c, const char* who, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min, double min_score,
                mtm_hit* out, float* nbhd, bool with_nbhd, int blend_a = 0, void* templ_out = nullptr,
                double* stats_out = nullptr, bool reacq = false) {
    if (!c || n_frames < 0 || n_tracks < 0 || margin < 0 || (n_frames > 0 && !frames) ||
        (n_tracks > 0 && !start) || (n_frames > 0 && n_tracks > 0 && (!out || (with_nbhd && !nbhd)))) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    if (reacq && !use_min) {
        set_error(std::string(who) + ": needs use_min (a track is searched again where its hit does not pass min_score)");
        return MTM_E_INVALID;
    }
    const bool adapt = blend_a > 0;
    MTM_NOT_IN_FLIGHT(c, who);
    if (n_frames == 0 || n_tracks == 0) return MTM_OK;
    for (int f = 0; f < n_frames; ++f) MTMC(check_image_args(frames[f], rows, cols, chans, dtype, row_stride_bytes, who));
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        set_error(std::string(who) + ": takes uint8 frames with 1 or 3 channels and single-channel uint16 frames");
        return MTM_E_INVALID;
    }
    if (!c->have_templ) {
        set_error(std::string(who) + ": no templates set");
        return MTM_E_STATE;
    }
    std::vector<BlobTempl> tl;
    MTMC(parse_templ_blob(c->templ_blob, tl, who, true));
    // the track table, and the tile table that covers every map a track can have: the frame-0 map, or one of at most
    // (2 margin + 1) outputs per side (a box is the hit widened by the margin), neither larger than the frame's own map
    std::vector<TrackUnit> tu((size_t)n_tracks);
    std::vector<TrackTile> tiles;
    unsigned long long tiles_max = 0;           // (reacq) the tiles of the largest whole-frame map
    for (int k = 0; k < n_tracks; ++k) {
        const mtm_box_unit& s = start[k];
        const std::string where = std::string(who) + ": track " + std::to_string(k);
        if (s.templ_idx < 0 || s.templ_idx >= (int)tl.size()) {
            set_error(where + ": template index out of range");
            return MTM_E_INVALID;
        }
        if (s.y0 < 0 || s.x0 < 0 || s.rows < 1 || s.cols < 1 || s.rows > rows - s.y0 || s.cols > cols - s.x0) {
            set_error(where + ": box outside the frame");
            return MTM_E_INVALID;
        }
        const BlobTempl& t = tl[(size_t)s.templ_idx];
        if (t.dtype != dtype || t.chans != chans) {
            set_error(where + ": template and frames differ in pixel type or channel count");
            return MTM_E_INVALID;
        }
        if (t.rows > s.rows || t.cols > s.cols) {
            set_error(where + ": template larger than the box");
            return MTM_E_INVALID;
        }
        if (dtype == MTM_U16 && (long long)t.rows * t.cols > (1ll << 21)) {
            set_error(where + ": uint16 template of more than 2^21 pixels");
            return MTM_E_INVALID;
        }
        if (reacq) {
            const long long wh = rows - t.rows + 1, ww = cols - t.cols + 1;
            if (wh * ww >= (1ll << 32)) {
                set_error(where + ": whole-frame map of 2^32 outputs or more");
                return MTM_E_INVALID;
            }
            tiles_max = std::max(tiles_max, (unsigned long long)((wh + kWinTile - 1) / kWinTile) *
                                                (unsigned long long)((ww + kWinTile - 1) / kWinTile));
        }
        TrackUnit& u = tu[(size_t)k];
        u.t = s.templ_idx;
        u.y0 = s.y0;
        u.x0 = s.x0;
        u.oh = s.rows - t.rows + 1;
        u.ow = s.cols - t.cols + 1;
        const long long side = 2ll * margin + 1;
        const int th = (int)std::min<long long>(std::max<long long>(u.oh, side), rows - t.rows + 1);
        const int tw = (int)std::min<long long>(std::max<long long>(u.ow, side), cols - t.cols + 1);
        for (int ty = 0; ty < th; ty += kWinTile)
            for (int tx = 0; tx < tw; tx += kWinTile) tiles.push_back(TrackTile{k, ty, tx});
    }
    HIPC(hipSetDevice(c->device));
    MTMC(prepare_window_templates(c, tl));
    MTMC(prepare_box_td(c, tl));

    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    const bool mode_min = c->method == MTM_TM_SQDIFF || c->method == MTM_TM_SQDIFF_NORMED;
    const size_t n_out = (size_t)n_frames * n_tracks;
    MTMC(c->trk_units.ensure(sizeof(TrackUnit) * tu.size()));
    MTMC(c->trk_tiles.ensure(sizeof(TrackTile) * tiles.size()));
    MTMC(c->trk_keys.ensure(sizeof(unsigned long long) * (size_t)n_tracks));
    MTMC(c->trk_out.ensure(sizeof(mtm_hit) * n_out));
    if (nbhd) MTMC(c->trk_nbhd.ensure(sizeof(float) * 9 * n_out));
    // (reacq) the lost state, all zero between frames: [wunits | list | n_lost | flags]
    TrackLostState lost{nullptr, nullptr, nullptr, nullptr};
    if (reacq) MTMC(track_lost_state(c, n_tracks, lost));
    // the tables the kernels read: the template set's (indexed by the list), or the call's own copies (indexed by the track)
    uint8_t* tpx = c->win_tpx.as<uint8_t>();
    const long long* toff = c->win_toff.as<long long>();
    TemplDev* td = c->box_td.as<TemplDev>();
    uint8_t* passed = nullptr;
    std::vector<long long> ktoff;
    size_t kbytes = 0;
    if (adapt) {
        std::vector<long long> ltoff(tl.size());         // (prepare_window_templates' offsets)
        long long at = 0;
        for (size_t i = 0; i < tl.size(); ++i) {
            ltoff[i] = at;
            at += (long long)tl[i].rows * tl[i].cols * (tl[i].dtype == MTM_U16 ? 2 : tl[i].chans);
        }
        ktoff.resize((size_t)n_tracks);
        for (int k = 0; k < n_tracks; ++k) {
            const BlobTempl& t = tl[(size_t)start[k].templ_idx];
            ktoff[(size_t)k] = (long long)kbytes;
            kbytes += (size_t)t.rows * t.cols * (t.dtype == MTM_U16 ? 2 : t.chans);
        }
        MTMC(c->trk_tpx.ensure(kbytes));
        MTMC(c->trk_toff.ensure(sizeof(long long) * (size_t)n_tracks));
        MTMC(c->trk_td.ensure(sizeof(TemplDev) * (size_t)n_tracks));
        MTMC(c->trk_pass.ensure((size_t)n_tracks));
        for (int k = 0; k < n_tracks; ++k) {
            const size_t j = (size_t)start[k].templ_idx;
            const size_t bytes = (size_t)(k + 1 < n_tracks ? ktoff[(size_t)k + 1] : (long long)kbytes) - (size_t)ktoff[(size_t)k];
            HIPC(hipMemcpyAsync(c->trk_tpx.as<uint8_t>() + ktoff[(size_t)k], tpx + ltoff[j], bytes, hipMemcpyDeviceToDevice,
                                c->stream));
            HIPC(hipMemcpyAsync(c->trk_td.as<TemplDev>() + k, td + j, sizeof(TemplDev), hipMemcpyDeviceToDevice, c->stream));
            tu[(size_t)k].t = k;
        }
        HIPC(hipMemcpyAsync(c->trk_toff.p, ktoff.data(), sizeof(long long) * (size_t)n_tracks, hipMemcpyHostToDevice,
                            c->stream));
        tpx = c->trk_tpx.as<uint8_t>();
        toff = c->trk_toff.as<long long>();
        td = c->trk_td.as<TemplDev>();
        passed = c->trk_pass.as<uint8_t>();
    }
    HIPC(hipEventRecord(c->ev[0], c->stream));
    HIPC(hipMemcpyAsync(c->trk_units.p, tu.data(), sizeof(TrackUnit) * tu.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->trk_tiles.p, tiles.data(), sizeof(TrackTile) * tiles.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(c->trk_keys.p, 0, sizeof(unsigned long long) * (size_t)n_tracks, c->stream));

    // chunks of frames as one stacked image (frame f of the chunk at rows f * rows ..), the track table carried across
    // them on the device: the stream orders a chunk's upload behind the previous chunk's launches, the host never waits
    const int per_chunk = track_chunk_frames(c, rows, cols, chans);
    const int ublocks = (n_tracks + 255) / 256;
    for (int f0 = 0; f0 < n_frames; f0 += per_chunk) {
        const int nb = std::min(per_chunk, n_frames - f0);
        adopt_image(c, nb * rows, cols, chans, dtype);
        MTMC(upload_image_stack(c, c->slot[c->cur], frames + f0, nb, row_stride_bytes, rows, cols, chans, dtype, c->stream));
        const ImageDev img = image_dev(c);
        const uint8_t* lo_b = c->slot[c->cur].u8b.as<uint8_t>() + img.u8_plane;     // uint16: [high ^ 0x80][low ^ 0x80]
        for (int fl = 0; fl < nb; ++fl) {
#define MTM_TRACK_LAUNCH(CH, U16)                                                                                            \
    hipLaunchKernelGGL((track_score_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, lo_b, tpx, toff, td,            \
                       c->trk_units.as<TrackUnit>(), c->trk_tiles.as<TrackTile>() + t0, fl * rows, c->method,                \
                       mode_min ? 1 : 0, c->trk_keys.as<unsigned long long>())
            for (size_t t0 = 0; t0 < tiles.size(); t0 += kTrackLaunchTiles) {
                const unsigned nt = (unsigned)std::min(kTrackLaunchTiles, tiles.size() - t0);
                if (dtype == MTM_U16) MTM_TRACK_LAUNCH(1, true);
                else if (chans == 1) MTM_TRACK_LAUNCH(1, false);
                else MTM_TRACK_LAUNCH(3, false);
                HIPC(hipGetLastError());
            }
#undef MTM_TRACK_LAUNCH
#define MTM_TRACK_UPDATE(REACQ)                                                                                               \
    hipLaunchKernelGGL(track_update_kernel<REACQ>, dim3(ublocks), dim3(256), 0, c->stream, c->trk_units.as<TrackUnit>(), td,  \
                       c->trk_keys.as<unsigned long long>(), n_tracks, mode_min ? 1 : 0, margin, use_min ? 1 : 0, min_score, \
                       rows, cols, c->trk_out.as<mtm_hit>() + (size_t)(f0 + fl) * n_tracks, passed, lost)
            if (reacq) MTM_TRACK_UPDATE(true);
            else MTM_TRACK_UPDATE(false);
#undef MTM_TRACK_UPDATE
            HIPC(hipGetLastError());
            const size_t r0 = (size_t)(f0 + fl) * n_tracks;
            // the frame's lost tracks over the whole frame, then their records and boxes from that search: a fixed grid
            // that finds the list on the device, no wait
#define MTM_TRACK_REACQUIRE(CH, U16)                                                                                         \
    hipLaunchKernelGGL((track_reacquire_kernel<CH, U16>), dim3(kTrackReacquireGrid), dim3(256), 0, c->stream, img, lo_b, tpx, \
                       toff, td, lost, tiles_max, fl * rows, c->method, mode_min ? 1 : 0,                                     \
                       c->trk_keys.as<unsigned long long>())
            if (reacq) {
                if (dtype == MTM_U16) MTM_TRACK_REACQUIRE(1, true);
                else if (chans == 1) MTM_TRACK_REACQUIRE(1, false);
                else MTM_TRACK_REACQUIRE(3, false);
                HIPC(hipGetLastError());
                hipLaunchKernelGGL(track_reupdate_kernel, dim3(ublocks), dim3(256), 0, c->stream,
                                   c->trk_units.as<TrackUnit>(), td, c->trk_keys.as<unsigned long long>(), n_tracks,
                                   mode_min ? 1 : 0, margin, min_score, rows, cols, c->trk_out.as<mtm_hit>() + r0, passed,
                                   lost);
                HIPC(hipGetLastError());
            }
#undef MTM_TRACK_REACQUIRE
            // the frame's neighbourhoods, from its records and its rows of the stack: no upload, no wait
            if (nbhd) MTMC(track_launch_nbhd(c, img, lo_b, tpx, toff, td, r0, n_tracks, fl * rows, rows, chans, dtype));
            // the passing tracks adopt their hits' windows: the templates of the next frame's search
#define MTM_TRACK_ADOPT(CH, U16)                                                                                             \
    hipLaunchKernelGGL((track_adopt_kernel<CH, U16>), dim3(nk), dim3(256), 0, c->stream, img, lo_b, tpx, toff + k0, td + k0,  \
                       c->trk_out.as<mtm_hit>() + r0 + k0, passed + k0, fl * rows, rows, c->method, blend_a)
            for (size_t k0 = 0; adapt && k0 < (size_t)n_tracks; k0 += kTrackLaunchNbhd) {
                const unsigned nk = (unsigned)std::min(kTrackLaunchNbhd, (size_t)n_tracks - k0);
                if (dtype == MTM_U16) MTM_TRACK_ADOPT(1, true);
                else if (chans == 1) MTM_TRACK_ADOPT(1, false);
                else MTM_TRACK_ADOPT(3, false);
                HIPC(hipGetLastError());
            }
#undef MTM_TRACK_ADOPT
        }
    }
    HIPC(hipEventRecord(c->ev[1], c->stream));
    HIPC(hipMemcpyAsync(out, c->trk_out.p, sizeof(mtm_hit) * n_out, hipMemcpyDeviceToHost, c->stream));
    if (nbhd) HIPC(hipMemcpyAsync(nbhd, c->trk_nbhd.p, sizeof(float) * 9 * n_out, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> kplanar;
    std::vector<TemplDev> ktd;
    if (adapt && templ_out) {
        kplanar.resize(kbytes);
        HIPC(hipMemcpyAsync(kplanar.data(), tpx, kbytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (adapt && stats_out) {
        ktd.resize((size_t)n_tracks);
        HIPC(hipMemcpyAsync(ktd.data(), td, sizeof(TemplDev) * (size_t)n_tracks, hipMemcpyDeviceToHost, c->stream));
    }
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    c->timing.n_hits = (int64_t)n_out;
    if (adapt) {
        // the records name the track (the kernels' tables are the call's own): back to the list index
        for (size_t i = 0; i < n_out; ++i) out[i].templ_idx = start[i % (size_t)n_tracks].templ_idx;
        if (templ_out) unpack_track_templates(kplanar, ktoff, tl, start, n_tracks, static_cast<uint8_t*>(templ_out));
        for (int k = 0; stats_out && k < n_tracks; ++k) {
            const TemplDev& d = ktd[(size_t)k];
            double* o = stats_out + 7 * (size_t)k;
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

// mtm_track_boxes_sets: track_boxes' chunks, stream order and single wait, over the unit table of the tracks' sets.
int track_boxes_sets(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                     int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, const int32_t* set_off,
                     const int32_t* set_idx, int margin, int use_min, double min_score, bool reacq, mtm_hit* out, float* nbhd) {
    const char* who = "mtm_track_boxes_sets";
    if (!c || n_frames < 0 || n_tracks < 0 || margin < 0 || (n_frames > 0 && !frames) ||
        (n_tracks > 0 && (!start || !set_off || !set_idx)) || (n_frames > 0 && n_tracks > 0 && !out)) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    if (reacq && !use_min) {
        set_error(std::string(who) + ": reacquire needs use_min (a track is searched again where its hit does not pass min_score)");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    if (n_frames == 0 || n_tracks == 0) return MTM_OK;
    for (int f = 0; f < n_frames; ++f) MTMC(check_image_args(frames[f], rows, cols, chans, dtype, row_stride_bytes, who));
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        set_error(std::string(who) + ": takes uint8 frames with 1 or 3 channels and single-channel uint16 frames");
        return MTM_E_INVALID;
    }
    if (!c->have_templ) {
        set_error(std::string(who) + ": no templates set");
        return MTM_E_STATE;
    }
    std::vector<BlobTempl> tl;
    MTMC(parse_templ_blob(c->templ_blob, tl, who, true));
    if (set_off[0] != 0) {
        set_error(std::string(who) + ": set_off[0] must be 0");
        return MTM_E_INVALID;
    }
    // the unit table (track after track, set order) and the (track, group, tile) table over the largest map a track can
    // have during the call, as track_boxes sizes it
    std::vector<TrackUnit> tu;
    std::vector<TrackSetTile> tiles;
    unsigned long long tiles_max = 0, groups_max = 0;       // (reacq) of the largest whole-frame map / the largest set
    for (int k = 0; k < n_tracks; ++k) {
        const mtm_box_unit& s = start[k];
        const std::string where = std::string(who) + ": track " + std::to_string(k);
        const long long n_set = (long long)set_off[k + 1] - set_off[k];
        if (n_set < 1) {
            set_error(where + (n_set == 0 ? ": empty set" : ": set_off is not ascending"));
            return MTM_E_INVALID;
        }
        if (s.templ_idx != set_idx[set_off[k]]) {
            set_error(where + ": start's template is not the first of its set");
            return MTM_E_INVALID;
        }
        if (s.y0 < 0 || s.x0 < 0 || s.rows < 1 || s.cols < 1 || s.rows > rows - s.y0 || s.cols > cols - s.x0) {
            set_error(where + ": box outside the frame");
            return MTM_E_INVALID;
        }
        for (int i = set_off[k]; i < set_off[k + 1]; ++i) {
            if (set_idx[i] < 0 || set_idx[i] >= (int)tl.size()) {
                set_error(where + ": template index out of range");
                return MTM_E_INVALID;
            }
            const BlobTempl& t = tl[(size_t)set_idx[i]];
            if (t.dtype != dtype || t.chans != chans) {
                set_error(where + ": template and frames differ in pixel type or channel count");
                return MTM_E_INVALID;
            }
            if (t.rows != tl[(size_t)s.templ_idx].rows || t.cols != tl[(size_t)s.templ_idx].cols) {
                set_error(where + ": the templates of a set must be of one shape");
                return MTM_E_INVALID;
            }
        }
        const BlobTempl& t = tl[(size_t)s.templ_idx];
        if (t.rows > s.rows || t.cols > s.cols) {
            set_error(where + ": template larger than the box");
            return MTM_E_INVALID;
        }
        if (dtype == MTM_U16 && (long long)t.rows * t.cols > (1ll << 21)) {
            set_error(where + ": uint16 template of more than 2^21 pixels");
            return MTM_E_INVALID;
        }
        const unsigned long long groups = (unsigned long long)((n_set + kTrackNV - 1) / kTrackNV);
        if (reacq) {
            const long long wh = rows - t.rows + 1, ww = cols - t.cols + 1;
            if (wh * ww >= (1ll << 32)) {
                set_error(where + ": whole-frame map of 2^32 outputs or more");
                return MTM_E_INVALID;
            }
            tiles_max = std::max(tiles_max, (unsigned long long)((wh + kWinTile - 1) / kWinTile) *
                                                (unsigned long long)((ww + kWinTile - 1) / kWinTile));
            groups_max = std::max(groups_max, groups);
        }
        const int oh = s.rows - t.rows + 1, ow = s.cols - t.cols + 1;
        for (int i = set_off[k]; i < set_off[k + 1]; ++i) tu.push_back(TrackUnit{set_idx[i], s.y0, s.x0, oh, ow});
        const long long side = 2ll * margin + 1;
        const int th = (int)std::min<long long>(std::max<long long>(oh, side), rows - t.rows + 1);
        const int tw = (int)std::min<long long>(std::max<long long>(ow, side), cols - t.cols + 1);
        for (int u0 = set_off[k]; u0 < set_off[k + 1]; u0 += kTrackNV)
            for (int ty = 0; ty < th; ty += kWinTile)
                for (int tx = 0; tx < tw; tx += kWinTile)
                    tiles.push_back(TrackSetTile{u0, std::min(kTrackNV, set_off[k + 1] - u0), ty, tx});
    }
    const size_t n_units = tu.size();
    HIPC(hipSetDevice(c->device));
    MTMC(prepare_window_templates(c, tl));
    MTMC(prepare_box_td(c, tl));

    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    const bool mode_min = c->method == MTM_TM_SQDIFF || c->method == MTM_TM_SQDIFF_NORMED;
    const size_t n_out = (size_t)n_frames * n_tracks;
    MTMC(c->trk_units.ensure(sizeof(TrackUnit) * n_units));
    MTMC(c->trk_tiles.ensure(sizeof(TrackSetTile) * tiles.size()));
    MTMC(c->trk_keys.ensure(sizeof(unsigned long long) * n_units));
    MTMC(c->trk_sets.ensure(sizeof(int) * ((size_t)n_tracks + 1)));
    MTMC(c->trk_out.ensure(sizeof(mtm_hit) * n_out));
    if (nbhd) MTMC(c->trk_nbhd.ensure(sizeof(float) * 9 * n_out));
    // (reacq) the lost state per track, all zero between frames: [wunits | list | n_lost | flags]
    TrackLostState lost{nullptr, nullptr, nullptr, nullptr};
    if (reacq) MTMC(track_lost_state(c, n_tracks, lost));
    const uint8_t* tpx = c->win_tpx.as<uint8_t>();
    const long long* toff = c->win_toff.as<long long>();
    const TemplDev* td = c->box_td.as<TemplDev>();
    TrackUnit* d_units = c->trk_units.as<TrackUnit>();
    const int* d_sets = c->trk_sets.as<int>();
    unsigned long long* d_keys = c->trk_keys.as<unsigned long long>();
    HIPC(hipEventRecord(c->ev[0], c->stream));
    HIPC(hipMemcpyAsync(c->trk_units.p, tu.data(), sizeof(TrackUnit) * n_units, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->trk_tiles.p, tiles.data(), sizeof(TrackSetTile) * tiles.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->trk_sets.p, set_off, sizeof(int) * ((size_t)n_tracks + 1), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(c->trk_keys.p, 0, sizeof(unsigned long long) * n_units, c->stream));

    const int per_chunk = track_chunk_frames(c, rows, cols, chans);
    const int ublocks = (n_tracks + 255) / 256;
    for (int f0 = 0; f0 < n_frames; f0 += per_chunk) {
        const int nb = std::min(per_chunk, n_frames - f0);
        adopt_image(c, nb * rows, cols, chans, dtype);
        MTMC(upload_image_stack(c, c->slot[c->cur], frames + f0, nb, row_stride_bytes, rows, cols, chans, dtype, c->stream));
        const ImageDev img = image_dev(c);
        const uint8_t* lo_b = c->slot[c->cur].u8b.as<uint8_t>() + img.u8_plane;     // uint16: [high ^ 0x80][low ^ 0x80]
        for (int fl = 0; fl < nb; ++fl) {
            const size_t r0 = (size_t)(f0 + fl) * n_tracks;
#define MTM_TRACK_LAUNCH(CH, U16)                                                                                            \
    hipLaunchKernelGGL((track_score_sets_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, lo_b, tpx, toff, td,       \
                       d_units, c->trk_tiles.as<TrackSetTile>() + t0, fl * rows, c->method, mode_min ? 1 : 0, d_keys)
            for (size_t t0 = 0; t0 < tiles.size(); t0 += kTrackLaunchTiles) {
                const unsigned nt = (unsigned)std::min(kTrackLaunchTiles, tiles.size() - t0);
                if (dtype == MTM_U16) MTM_TRACK_LAUNCH(1, true);
                else if (chans == 1) MTM_TRACK_LAUNCH(1, false);
                else MTM_TRACK_LAUNCH(3, false);
                HIPC(hipGetLastError());
            }
#undef MTM_TRACK_LAUNCH
#define MTM_TRACK_UPDATE(REACQ)                                                                                               \
    hipLaunchKernelGGL(track_update_sets_kernel<REACQ>, dim3(ublocks), dim3(256), 0, c->stream, d_units, d_sets, td, d_keys,  \
                       n_tracks, mode_min ? 1 : 0, margin, use_min ? 1 : 0, min_score, rows, cols,                           \
                       c->trk_out.as<mtm_hit>() + r0, lost)
            if (reacq) MTM_TRACK_UPDATE(true);
            else MTM_TRACK_UPDATE(false);
#undef MTM_TRACK_UPDATE
            HIPC(hipGetLastError());
#define MTM_TRACK_REACQUIRE(CH, U16)                                                                                         \
    hipLaunchKernelGGL((track_reacquire_sets_kernel<CH, U16>), dim3(kTrackReacquireGrid), dim3(256), 0, c->stream, img, lo_b, \
                       tpx, toff, td, d_units, d_sets, lost, groups_max, tiles_max, fl * rows, c->method, mode_min ? 1 : 0,   \
                       d_keys)
            if (reacq) {
                if (dtype == MTM_U16) MTM_TRACK_REACQUIRE(1, true);
                else if (chans == 1) MTM_TRACK_REACQUIRE(1, false);
                else MTM_TRACK_REACQUIRE(3, false);
                HIPC(hipGetLastError());
                hipLaunchKernelGGL(track_reupdate_sets_kernel, dim3(ublocks), dim3(256), 0, c->stream, d_units, d_sets, td,
                                   d_keys, n_tracks, mode_min ? 1 : 0, margin, min_score, rows, cols,
                                   c->trk_out.as<mtm_hit>() + r0, lost);
                HIPC(hipGetLastError());
            }
#undef MTM_TRACK_REACQUIRE
            // the frame's neighbourhoods: track_nbhd_kernel as it is - it reads the winner's template from the record
            if (nbhd) MTMC(track_launch_nbhd(c, img, lo_b, tpx, toff, td, r0, n_tracks, fl * rows, rows, chans, dtype));
        }
    }
    HIPC(hipEventRecord(c->ev[1], c->stream));
    HIPC(hipMemcpyAsync(out, c->trk_out.p, sizeof(mtm_hit) * n_out, hipMemcpyDeviceToHost, c->stream));
    if (nbhd) HIPC(hipMemcpyAsync(nbhd, c->trk_nbhd.p, sizeof(float) * 9 * n_out, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    c->timing.n_hits = (int64_t)n_out;
    // the stack is none of the caller's frames: no current image, no published maps
    c->have_image = false;
    return MTM_OK;
}

}  // namespace

extern "C" {

int mtm_track_boxes(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                    int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                    double min_score, mtm_hit* out) {
    return track_boxes(c, "mtm_track_boxes", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start, n_tracks,
                       margin, use_min, min_score, out, nullptr, false);
}

int mtm_track_boxes_nbhd(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                         int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                         double min_score, mtm_hit* out, float* nbhd) {
    return track_boxes(c, "mtm_track_boxes_nbhd", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                       n_tracks, margin, use_min, min_score, out, nbhd, true);
}

int mtm_track_boxes_adapt(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                          int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                          double min_score, mtm_hit* out, float* nbhd, int blend_a, void* templ_out, double* stats_out) {
    if (blend_a < 1 || blend_a > 256) {
        set_error("mtm_track_boxes_adapt: blend_a outside 1 .. 256");
        return MTM_E_INVALID;
    }
    return track_boxes(c, "mtm_track_boxes_adapt", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                       n_tracks, margin, use_min, min_score, out, nbhd, false, blend_a, templ_out, stats_out);
}

int mtm_track_boxes_reacquire(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                              int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                              double min_score, mtm_hit* out, float* nbhd, int blend_a, void* templ_out, double* stats_out) {
    if (blend_a < 0 || blend_a > 256) {
        set_error("mtm_track_boxes_reacquire: blend_a outside 0 .. 256");
        return MTM_E_INVALID;
    }
    return track_boxes(c, "mtm_track_boxes_reacquire", frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start,
                       n_tracks, margin, use_min, min_score, out, nbhd, false, blend_a, templ_out, stats_out, true);
}

int mtm_track_boxes_sets(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                         int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, const int32_t* set_off,
                         const int32_t* set_idx, int margin, int use_min, double min_score, int reacquire, mtm_hit* out,
                         float* nbhd) {
    return track_boxes_sets(c, frames, n_frames, rows, cols, chans, dtype, row_stride_bytes, start, n_tracks, set_off, set_idx,
                            margin, use_min, min_score, reacquire != 0, out, nbhd);
}

}  // extern "C"
