// Internal declarations shared by the host-only translation unit (mtm_host.cpp) and the HIP
// translation units (mtm_context / _placement / _launch / _api / _comm .hip).  Not part of the ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mtm_hip.h"
#include "mtm_blocks_predict.h"    // BlockGrid, the shared predict and box functions
#include "mtm_quality_key.h"       // the keys' decoders, shared with the device
#include "mtm_route.h"
#include "mtm_templ_stats.h"       // TemplStats, templ_stats_from_sums_inl

namespace mtm {

void set_error(const std::string& msg);   // thread-local message behind mtm_last_error()

// Whether the best match of `method` is the map's minimum (the difference methods): hits are then ranked by -score.
constexpr bool method_mode_min(int method) { return method == MTM_TM_SQDIFF || method == MTM_TM_SQDIFF_NORMED; }

// px: planar float64 copies of the template (and mask weights, or nullptr), chans planes of
// rows*cols each.  `integer` = values are exact integers (uint8 source).
TemplStats compute_templ_stats(const double* px, const double* mask, int rows, int cols, int chans,
                               int method, bool integer);

// the same from the per-channel sums (sum v, sum v^2), or - masked - from sum((v*m)^2) alone (templ_stats_from_sums_inl)
TemplStats templ_stats_from_sums(const double* sum, const double* sumsq, double templ2_mask2_sum, bool masked, int rows,
                                 int cols, int chans, int method);

// exact sum v / sum v^2 of n bytes, added to *sum / *sumsq
void u8_run_sums(const uint8_t* p, size_t n, unsigned long long* sum, unsigned long long* sumsq);
// The tail screen's split for an h x w class at the candidate threshold thr_lo (see the definition; 0 = no screen)
int tail_split_rule(int h, int w, double thr_lo);
// ... its measured constants, and the threshold whose split a class's tail constants are computed for at placement
constexpr double kTailSplitZ = 6.5;
constexpr double kTailSplitMaxFrac = 0.94;
constexpr double kTailDefaultThr = 0.5;

// scipy.signal.find_peaks(x, height=h)[0]
std::vector<int> find_peaks_1d(const float* x, int n, int stride, float height, bool negate);

// The peaks of a 1-D or 1x1 score map (MTM/__init__.py:25-41) as records of template `templ_idx` (a w x h box), appended to
// `out`: a 1x1 map is a peak when its quality reaches `thr`, a longer line goes through find_peaks_1d.  `line` holds the map's
// max(oh, ow) values contiguously; the record's x runs along a row (oh == 1), its y down a column.
void line_map_peaks(const float* line, int oh, int ow, float thr, bool mode_min, int templ_idx, int w, int h,
                    std::vector<mtm_hit>& out);

// the float32 of an order key's high word (key_order_float, mtm_quality_key.h)
float order_to_float(uint32_t o);

// Hit records from the 64-bit extremum keys of a map ow outputs wide (order << 32 | ~row-major index), both built on
// mtm_quality_key.h:
//  - decode_extremum_key: one of the max / min pair of extremum_kernel / extremum_batch_kernel (the minimum's order is
//    stored complemented); key == 0 (no output) -> score NaN at (0, 0)
//  - decode_quality_key: the window kernels' key over the quality (quality_key_record at origin (0, 0));
//    key == 0 -> score NaN, the index as the key reads
mtm_hit decode_extremum_key(unsigned long long key, bool mode_min, int templ_idx, int ow, int w, int h);
mtm_hit decode_quality_key(unsigned long long key, bool mode_min, int templ_idx, int ow, int w, int h);

// A call's result: `hits` becomes `last_hits` (what mtm_last_hits / mtm_group_last_hits hand out afterwards), *n_out its
// size; MTM_E_OVERFLOW with `msg` when it exceeds `capacity`, else it is copied to `out`.  copy_out_hits: the copy alone.
int copy_out_hits(const std::vector<mtm_hit>& hits, mtm_hit* out, int64_t capacity, int64_t* n_out, const std::string& msg);
int publish_hits(std::vector<mtm_hit>& hits, std::vector<mtm_hit>& last_hits, mtm_hit* out, int64_t capacity,
                 int64_t* n_out, const std::string& msg);

// ---- mtm_find_matches' synchronising half (fm_end, mtm_api.hip; its peak pass: mtm_peaks.hip): its host-only pieces

// (oh, ow) of template t's map, read in place from any array of records that holds both (`stride` bytes apart)
struct MapDims {
    const int* oh0;
    const int* ow0;
    size_t stride;
    int oh(int t) const { return *reinterpret_cast<const int*>(reinterpret_cast<const char*>(oh0) + stride * (size_t)t); }
    int ow(int t) const { return *reinterpret_cast<const int*>(reinterpret_cast<const char*>(ow0) + stride * (size_t)t); }
};
// The 3x3 test of a complete candidate list `cd[0 .. ncand)`: every pixel whose quality (score, or -score with mode_min)
// exceeds thr_q is in the list, so a neighbour that is not is <= thr_q < candidate - the list alone decides.  A candidate
// is a hit when its quality exceeds thr_q and is no less than any listed neighbour's, nor than `padv` (0 for the constant
// border, -INFINITY else) where a neighbour lies outside the map; of a duplicated record the first counts.  Hits are
// appended to `hits` in list order and counted per template in tflags[t] (+= 1 each).  hk / hv: scratch the caller keeps
// between calls (an open-addressing table, rebuilt here; they need not be cleared).
void verify_candidates_3x3(const mtm_hit* cd, size_t ncand, const MapDims& dims, bool mode_min, float thr_q, float padv,
                           std::vector<unsigned long long>& hk, std::vector<int>& hv, std::vector<mtm_hit>& hits, int* tflags);

// skimage: a map in which every pixel equals its local maximum has no peaks at all.  The scans' per-template flag word:
// byte 0 = "some pixel differs from its local maximum" (peaks_kernel), bytes 1 and 2 = "a segment above / below the
// threshold exists" (peaks_sparse_kernel, which never looks at the unflagged ones).  The candidate routes count a template's
// peaks instead: every pixel a peak <=> trivial.
bool scan_flags_trivial(unsigned flags);
bool fused_count_trivial(long long n_peaks, int oh, int ow);

// The overflow ladder of fm_end.  A pass reports what overflowed; ladder_next names the step that follows (today's route
// and the number of the pass decide it), ladder_apply makes the step's changes to the route.  The effects of a step -
// re-running the score pass, clearing lists, the context's back-off counters, a longer hit list - are fm_end's.
enum class LadderStep {
    Done,                   // the pass's list is the result
    ThreeProducts,          // float32 refinement, the one-product screen listed too much: three piece products
    MapScan,                // ... the kernel candidates overflowed: the potential peaks of a map scan
    Float64,                // ... those too, a bound too wide for the scan, raw sums, the global extremum: the float64 kernel
    Maps,                   // integer candidates overflowed: maps in memory, full peak pass
    GrowList,               // more peaks than the hit list holds: once more with room for all of them
    GrowListLeaveSegments,  // ... and the flagged segments' bounded lists were the reason: the full scan's single list
};
struct PassOutcome {
    bool rig_wide;          // map scan: a bound beyond its tolerances; map scan and refined global extremum: an output not finite
    bool cands_overflow;    // more candidates (global extremum: outputs within the margin of the best) than the list holds
    bool hits_overflow;     // more peaks than the hit list holds
};
LadderStep ladder_next(const mtmi::CallRoute& R, const PassOutcome& o, int attempt);
void ladder_apply(mtmi::CallRoute& R, LadderStep s);

// ---- the host plan of a tracking call (mtm_track_boxes*, mtm_track.hip)

// One template of the last mtm_set_templates as its bytes in mtm_ctx::templ_blob (interleaved, tightly packed rows of
// `dtype` pixels); parse_templ_blob (mtm_placement.hip) lists them - unmasked uint8 templates, with `u16_ok` also unmasked
// single-channel uint16 ones - for mtm_find_matches_pyramid, mtm_find_matches_boxes and the tracking calls.
struct BlobTempl {
    int rows, cols, chans, dtype;
    const uint8_t* px;
};
constexpr int kTrackTile = 16;      // a tile of 16 x 16 outputs: the window kernels' kWinTile (mtm_track.hip asserts it)
constexpr int kTrackNV = 4;         // templates of a set that one work-group scores together (a group)
// A unit as the kernels see it: its template, the frame pixel of its map's output (0, 0) and the map's size.  Frame
// coordinates: the score kernels add the frame's row offset in the chunk's stack.
struct TrackUnit {
    int t;
    int y0, x0;
    int oh, ow;
};
// One 16 x 16 tile of outputs of the units u0 .. u0 + nv - 1 (one group of one track), first output (ty0, tx0) of their map.
struct TrackTile {
    int u0, nv, ty0, tx0;
};
struct TrackPlan {
    std::vector<TrackUnit> units;           // one per (track, template of its set), track after track in set order
    std::vector<int> set_off;               // track k's units: set_off[k] .. set_off[k + 1] - 1
    std::vector<TrackTile> tiles;           // per track and group, row-major over the largest map the track can have
    unsigned long long tiles_max = 0;       // (reacq) the tiles of the call's largest whole-frame map
    unsigned long long groups_max = 0;      // (reacq) the groups of the call's largest set
    size_t n_units = 0;
    std::vector<size_t> templ_bytes;        // the bytes of each track's template planes (the start template's)
};
// The tracks of a call checked and laid out: templates `tl`, frames of rows x cols x chans `dtype` pixels, frame-0 boxes
// and templates start[0 .. n_tracks - 1]; track k's set is set_idx[set_off[k] .. set_off[k + 1] - 1], or - set_off ==
// nullptr - its start template alone.  A track's tiles cover every map it can have during the call: the frame-0 map, or
// one of 2 margin + 1 outputs per side, clipped to the whole-frame map.  MTM_OK, or the code and message (set_error,
// prefixed `who`) of the first track that is not valid.
int plan_tracks(const std::vector<BlobTempl>& tl, int rows, int cols, int chans, int dtype, const mtm_box_unit* start,
                int n_tracks, int margin, bool reacq, const int32_t* set_off, const int32_t* set_idx, const char* who,
                TrackPlan& plan);

// ---- the host plan of a block-matching call (mtm_match_blocks, mtm_blocks.hip)

// Blocks b0 .. b1 - 1 run together: their tiles are tiles[t0 .. t1 - 1], their gathered template planes fill `bytes`.
struct BlockChunk {
    int b0, b1;
    size_t t0, t1;
    size_t bytes;
};
struct BlockPlan {
    std::vector<TrackUnit> units;           // block k: t = k, the image pixel of its map's output (0, 0), the map's size
    std::vector<long long> toff;            // byte offset of block k's template planes in its chunk's buffer
    std::vector<TrackTile> tiles;           // {k, 1, ty0, tx0}: block after block, row-major over each block's map
    std::vector<BlockChunk> chunks;         // whole blocks, in order, each within the budget (a single block may pass it)
    size_t max_bytes = 0;                   // the largest chunk's template bytes
    // block k: (ox, oy) = clip[2 k], clip[2 k + 1], how far its box was clipped at the left and at the top - output (y, x)
    // of its map is displacement (x + ox - margin, y + oy - margin), cell (y + oy, x + ox) of its (2 margin + 1)^2 plane
    std::vector<int32_t> clip;
};
// The blocks of a call checked and laid out: images of rows x cols x chans `dtype` pixels; block k's search box is its own
// box widened by `margin` on every side and clipped to the image (MTM.blocks.search_box), its map that of a template of
// the block's size over the box.  Chunks hold whole blocks while their template bytes - w h chans, uint16: 2 w h - stay
// within budget_bytes.  MTM_OK, or the code and message (set_error, prefixed `who`) of the first block that is not valid.
// with_tiles = false leaves the tile table empty, for fix_block_tiles to fill.  masked (mtm_match_blocks_masked): a block's
// planes are those of T M and, behind them, as many of its mask - 2 w h chans bytes.
int plan_blocks(int rows, int cols, int chans, int dtype, const mtm_block* blocks, int n_blocks, int margin,
                long long budget_bytes, const char* who, BlockPlan& plan, bool with_tiles = true, bool masked = false);

// ---- block matching with boxes the device computes (mtm_match_blocks_at, mtm_match_blocks_passes, mtm_blocks.hip)

// The plan's tile table replaced by the fixed one: T^2 tiles per block, T = ceil((2 margin + 1) / 16), row-major, whatever
// the block's clipped map - the kernel leaves the tiles that lie outside the map the device computed.  (Per axis never
// more tiles than the whole image's map of the block has: no moved box has a larger one.)  The chunks keep
// their blocks and get the new tile ranges; the units stay those of zero offsets.  MTM_E_INVALID (set_error, prefixed
// `who`) when the table would hold 2^31 tiles or more, or a moved block could have a map of 2^32 outputs or more.
int fix_block_tiles(BlockPlan& plan, int rows, int cols, const mtm_block* blocks, int margin, const char* who);

// One pass of a mtm_match_blocks_passes call: its grid, the grid's blocks in row-major order and their plan with the
// fixed tile table.
struct BlockPassPlan {
    BlockGrid grid;
    int margin;
    std::vector<mtm_block> blocks;
    BlockPlan plan;
};
// The passes of a call checked and laid out (plan_blocks and fix_block_tiles per pass).  MTM_OK, or the code and message
// (set_error, prefixed `who`) of the first pass that is not valid; a pass whose grid is empty is not.
int plan_block_passes(int rows, int cols, int chans, int dtype, const mtm_block_pass* passes, int n_passes,
                      long long budget_bytes, const char* who, std::vector<BlockPassPlan>& plans);

// ---- the frame chunks of a block-matching call over a frame stack (mtm_match_blocks_stack, mtm_blocks.hip)

// One upload: the stack [frame `carried`, frames f0 .. f0 + nf - 1] - the carried frame brings the reference into the
// chunk - and the pairs p0 .. p0 + nf - 1 it runs: pair p searches frame p + 1 (stack slot p + 2 - f0); its reference is
// frame p (slot p + 1 - f0; slot 0 for p = p0) or, mode "first", frame 0 (slot 0).
struct StackChunk {
    int f0, nf, carried, p0;
};
// n_frames >= 2 frames in stacks of at most frames_per_chunk >= 2 frames each; mode: MTM_BLOCKS_REF_PREVIOUS / _FIRST.
// Frame 0 is the first chunk's carried frame: every frame is uploaded once, plus one carried frame per later chunk.
std::vector<StackChunk> plan_blocks_stack(int n_frames, int frames_per_chunk, int mode);

// float32-faithful restatement of cv2.dnn.NMSBoxes as called by MTM.NMS
void nms_boxes(const mtm_hit* hits, int64_t n, const float* scores, float score_threshold,
               float nms_threshold, std::vector<int32_t>& keep);

// the same selection from a list in any order, returned in NMSBoxes' order (score ties as mtm_find_matches' order resolves them)
// (`n_sure`: the first n_sure hits are known to be kept - no earlier hit overlaps them beyond the threshold -: they are not tested)
void nms_select(const mtm_hit* hits, int64_t n, int ascending, float score_threshold, float nms_threshold,
                std::vector<int32_t>& keep, int64_t n_sure = 0);

// The order in which mtm_find_matches returns its records: template, then descending quality (score, or -score for the
// difference methods), then row-major position.  Deterministic whatever order the GPU appended them in; thousands
// of records (smooth images at a low threshold) are sorted by an LSD radix sort on the same key.
void sort_hits(std::vector<mtm_hit>& hits, bool mode_min);

}  // namespace mtm
