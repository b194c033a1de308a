// Internal header of libmtm_hip.so's GPU side: the context, the size classes of a template set, and the functions the
// translation units share.  Units: mtm_context.hip (context, options, image upload), mtm_placement.hip (template sets ->
// size classes, packs, constants), mtm_stats.hip (window statistics: their launchers and test-support entries),
// mtm_launch.hip (score-map launches and the score pass of a call, plain and banded), mtm_api.hip
// (mtm_find_matches and friends: a call's route, its ladder, hit lists), mtm_peaks.hip (the peak pass: its launchers and
// fetches, the device's share of the NMS), mtm_comm.hip (RCCL hit exchange), mtm_pyramid.hip (the
// coarse-to-fine search), mtm_boxes.hip (many searchBoxes in one call), mtm_subpixel.hip (hit neighbourhoods), mtm_blocks.hip (block matching
// between two images).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "mtm_kernels.h"
#include "mtm_mfma_params.h"
#include "mtm_bf16_params.h"
#include "mtm_score_params.h"
#include "mtm_templates_params.h"
#include "mtm_internal.h"
#include "mtm_route.h"
#include "mtm_peak_sizing.h"
#include "mtm_stats_route.h"

struct ncclComm;

namespace mtmi {

using namespace mtm;

#define HIPC(expr)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                   \
            return MTM_E_HIP;                                                               \
        }                                                                                   \
    } while (0)

#define MTMC(expr)                                                                          \
    do {                                                                                    \
        int r_ = (expr);                                                                    \
        if (r_ != MTM_OK) return r_;                                                        \
    } while (0)
// between mtm_find_matches_async and mtm_find_matches_wait the context belongs to that call
#define MTM_NOT_IN_FLIGHT(c, who)                                                                         \
    do {                                                                                                  \
        if ((c)->fm_in_flight) {                                                                          \
            set_error(std::string(who) + ": a mtm_find_matches_async call is in flight (collect it with " \
                      "mtm_find_matches_wait first)");                                                    \
            return MTM_E_INVALID;                                                                         \
        }                                                                                                 \
    } while (0)


inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The window units (boxes, tracking, blocks) launch one work-group per entry of a table; a launch takes at most this many,
// so that one dispatch stays far below 2^32 work-items however long the table is.
constexpr size_t kLaunchGroups = (size_t)1 << 22;
// launch(first, count) for [begin, end) in slices of at most kLaunchGroups entries, in order; the first status that is
// not MTM_OK ends the walk and is returned.
template <class Launch>
int for_launch_slices(size_t begin, size_t end, Launch&& launch) {
    for (size_t at = begin; at < end; at += kLaunchGroups) MTMC(launch(at, (unsigned)std::min(kLaunchGroups, end - at)));
    return MTM_OK;
}

// mtm_find_matches_batch stacks its images into one tall image.  The rows of one chunk are bounded by the tightest packing a
// tall map can reach: launches with one grid row per map row (masksq_combine_kernel, slab_combine_kernel, the
// masked float32 kernels: grid.y = oh) stay within 16 bits.  Looser ones: the candidate key (cand_key, the host's 3x3 table)
// packs y into 21 bits; sort_hits' radix path needs y < 2^16 (per image after the split: it falls back to std::sort
// otherwise); mtm_hit, map_off (64-bit) and the statistics pitch (columns) do not depend on the row count.
constexpr int kBatchMaxRows = 65535;
// ... and the device memory of a chunk (score maps of every template + image planes + statistics, per pixel) stays below this
constexpr double kBatchChunkBytes = 8.0 * (1ull << 30);

inline size_t elem_size(int dtype) { return dtype == MTM_U8 ? 1 : dtype == MTM_U16 ? 2 : 4; }

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    // Grows to at least `bytes` (contents are NOT preserved).  The new block is allocated before the old one
    // is released: a failed allocation leaves the buffer as it was.
    int ensure(size_t bytes) {
        if (bytes <= cap) return MTM_OK;
        const size_t want = round_up(bytes + bytes / 8, 256);
        void* fresh = nullptr;
        HIPC(hipMalloc(&fresh, want));
        if (p) (void)hipFree(p);
        p = fresh;
        cap = want;
        return MTM_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct HostTempl {
    int rows = 0, cols = 0, chans = 0, dtype = 0;
    bool masked = false;
    std::vector<double> px;     // planar [C][h][w]
    std::vector<double> mask;   // planar weights (binarised for uint8 masks) or empty
    TemplStats st;
    int cls = -1;
    // uint8 template sets: the pixels live on the device as a view of a source in the arena (mtm_templates.hip.h);
    // px / mask above stay empty until a kernel that needs host-packed weights asks for them (ensure_host_pixels)
    bool on_device = false;
    UnitSrc src{};
    double sum_t = 0.0;                 // sum over all channels of T (masked: T * M): bias term of the MFMA path
    double mask_ones = 0.0;             // set mask pixels (channel 0)
    unsigned long long mask_key = 0;    // identifies the (transformed) mask: equal keys = equal masks
};

struct SizeClass {
    int h = 0, w = 0;
    bool masked = false;
    bool all_u8 = true;
    bool all_u16 = true;
    bool all_f32 = true;
    int kernel = MTM_KERNEL_AUTO;   // the kernel that runs the class, decided (and packed for) by place_templates
    int rm_nt = 0, rm_R = 0;    // > 0: row-multiplexed MFMA mode (<= 16 templates: nt x R = 16 A rows)
    int kp_nseg = 0;            // > 0: packed K (MfmaParams::kp_nseg): ceil(w / 16) segments per template row, 4 per MFMA step
    // large templates (w > 256 or w*h*C > 131071) on the MFMA kernel: cut into slabs (slab_combine_kernel)
    struct Slab {
        int r0, r1, c0, c1, ch;
        long long apack_off;    // this slab's packs in the apack arena
        int tlist_off;          // its view list (unit-table indices) in the device tlist
    };
    std::vector<Slab> slabs;
    int slab_nt = 0, slab_R = 0;    // > 0: row-multiplexed raw launches (<= 16 templates); 0: plain raw launches
    int r2 = 0;                 // multi-row MFMA variant (> 16 templates, w <= 64, one channel, methods 2..5): 2 or 3 consecutive
                                // output rows x 16 templates per wave; packs of h + r2 - 1 rows per 16-template group (the
                                // extra rows zero); 0 = off
    bool tail_ok = false;       // two-row variant in one K chunk, h >= 8: its hits-only launches can screen their K loop
    int tail_split = 0;         // ... the split (MfmaParams::tail_split) the class's tail constants are computed for at placement:
                                // tail_split_rule at the default threshold, or the forced one (mtm_ctx::tail_split_force); 0 = none
    long long mask_rm_off = -1; // masked class: row-multiplexed pack (1 "template" = the binary mask, R = 16) in apacks
    double mask_ones = 0.0;     // number of set mask pixels
    int n_pad = 0;              // members rounded up to a multiple of 16 (uint16 packs)
    long long tsum_off = -1;    // doubles: [sum(T_hi) per member][sum(T_lo) per member] in the tsum arena
    std::vector<int> members;
    int tlist_off = 0;          // offset into the device tlist array
    bool masked_int = false;    // masked class on the integer path: binary uint8 mask shared by all members
    unsigned long long mask_hash = 0;
    long long mask_pack_off = -1;   // dot4 pack of the mask bytes (0xFF / 0) in the pack arena (MTM_ROW_MUX=0 / MTM_FUSE_STATS=0 only)
    // float32 class with masks on the bf16 matrix cores as a screen (mtm_maskf32.hip.h, round 6): bf16 packs of U = T M^2 and
    // V = M^2 in the apack arena (the class itself stays a float64-kernel class: weights, fallback, exact re-scoring)
    bool mask_bf16 = false;
    long long mbf_off_u = -1, mbf_off_v = -1, mbf_group_bytes = 0;
    long long apack_off = 0;    // byte offset of this class's A packs in the apack arena
    long long group_bytes = 0;
};

}  // namespace mtmi

struct mtm_ctx {
    using DevBuf = mtmi::DevBuf;
    using HostTempl = mtmi::HostTempl;
    using SizeClass = mtmi::SizeClass;
    using CallRoute = mtmi::CallRoute;
    using TemplDev = mtm::TemplDev;
    using UnitSrc = mtm::UnitSrc;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ncc_ev;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> sq_ev;       // event pairs of the sum I^2 M passes (timing.masked_stat_ms)
    int cand_pinned = 1;        // MTM_CAND_PINNED: the score kernel writes the first records of its candidate list into the pinned
                                // landing buffer itself (MfmaParams::cand_pin) - no fetch kernel behind the score launch (0: round 4)
    int fuse_layout = 1;        // MTM_FUSE_LAYOUT: banded uploads convert a band's rows inside its statistics launch (0: planarize kernel)
    int masksq_fused = 1;       // MTM_MASKSQ_FUSED: sum I^2 M of a masked class as ONE launch over both byte planes of I^2 that
                                // writes the sum2 plane itself (0: round 3's two raw launches + masksq_combine_kernel)

    // image
    bool have_image = false;
    int rows = 0, cols = 0, chans = 0, dtype = 0;
    int u8_pitch = 0, f32_pitch = 0, rows_alloc = 0;
    // Device copies of an image: raw (as uploaded), planar padded u8 / int8-biased u8 / f32.  Two slots:
    // `cur` is what the kernels read; the other one receives the next image of a stream
    // (mtm_find_matches_next) on copy_stream while the kernels run.
    struct ImageSlot {
        DevBuf raw, u8, u8b, f32;
        long long geom = -1;        // (rows, cols, chans, dtype) the padding was initialised for
        bool f32_valid = true;      // false after a banded uint8 upload: the float32 plane was skipped (ensure_f32_plane)
    } slot[2];
    int cur = 0;
    DevBuf sq_planes;           // two planes: [high byte of I^2 ^ 0x80][low byte ^ 0x80] of the current uint8 image
    bool sq_valid = false;
    hipStream_t copy_stream = nullptr;
    long long nms_device_min = 4096;        // CallRoute::nms: fewer peaks than this are pruned on the host (as fast)
    DevBuf nms_buf;
    DevBuf nms_dbg;             // mtm_debug_device_nms: [the count][the records] of the list under test
    DevBuf peak_dbg;            // mtm_debug_peak_pass: the table, maps, flags, lists and counters of the maps under test
    DevBuf stats_dbg;           // mtm_debug_window_stats: the image, its planes, the statistics planes and records under test
    // segment flags (MTM_SPARSE_MAPS, default 1): the route of a call on dense maps (candidate list overflowed recently)
    // when every class runs the lean MFMA epilogue - maps in memory, one flag per row segment that holds something above the
    // threshold, peaks_sparse_kernel over the flagged segments instead of the full scan (MfmaParams::seg_flags)
    int sparse_maps = 1;
    DevBuf seg_flags, hits_t;               // (hits_t: per-template peak lists of peaks_sparse_kernel + their counters)
    hipEvent_t next_ready = nullptr;
    // mtm_find_matches_image: the image arrives in row bands on copy_stream (copy, layout conversion, window
    // statistics of the rows that became computable); the score kernel of a band waits for its event
    int screen_l1 = 1;                      // MTM_SCREEN_L1: the hits-only screen starts with the per-lane bound (0: round 2's screen alone)
    int tail_screen = 1;                    // MTM_TAIL_SCREEN: the two-row variant's hits-only K loop stops early where a bound on the
                                            // template rows still missing rules out every candidate (MfmaParams::tail_split)
    int tail_split_force = 0;               // MTM_TAIL_SPLIT=<s>: that split (clamped to [6, h - 2]) wherever the route allows a
                                            // screen, instead of tail_split_rule's (tests, measurements)
    std::vector<int> tail_valid;            // per size class: the split TemplDev::tail_* on the device hold the constants of
                                            // (ensure_tail_consts re-derives them when a call's split differs), 0 = none
    std::vector<int> tail_last;             // per size class: the split its last score launch carried, 0 = unscreened
                                            // (test support: mtm_debug_class_tilings)
    std::vector<int> dot_last;              // per size class: the kDotVariants entry its last dot4 launch took, -1 = none yet
                                            // (test support: mtm_debug_class_tilings)
    int f32_mfma = 1;                      // MTM_F32_MFMA / MTM_OPT_F32_MFMA: unmasked float32 classes on the bf16 matrix cores:
                                            // 0 = float64 kernel, 1 = bf16 screen + exact float64 re-scoring of everything
                                            // that could be a peak (hit lists of the float64 kernel), 2 = bf16 scores as they are,
                                            // 3 = as 1 without the one-product tier (every screen with three piece products),
                                            // 4 = (diagnostic) as 2 with ONE piece product: the screen's raw scores, what
                                            // tests/test_gpu_parity.py measures its bound on - never a result
    // Round 6: the hits-only refined routes screen with ONE piece product first (ncc_bf16_kernel<MB, 1>, a third of the
    // matrix-core work, bound 2^-7 instead of 2^-15 of the norms' product); a list that overflows repeats the launch with
    // three products, and the next np1_backoff calls start there
    int np1_backoff = 0, np1_backoff_len = 16;
    int seg_skip = 1;                       // MTM_SEG_SKIP: dense route - outputs that cannot pass the threshold are not finished (MfmaParams::seg_skip)
    int templ_on_device = 1;                // MTM_TEMPL_ON_DEVICE: uint8 template sets live on the device (views + device packing); 0 = packed on
                                            // the host (the independent restatement test_template_sets_on_device compares with)
    int mfma_r2 = 1;                        // MTM_MFMA_R2: 1 = two-row variant of the MFMA kernel where it applies, 0 = off
    // lanes of a multi-class call: size classes are independent (their own statistics, launches, scratch); consecutive
    // classes go to alternating lanes - a stream plus the per-class scratch buffers - so that the statistics / combine
    // kernels and the tail of one class run under the score kernel of the next.  Lane 0 is the context's own stream and
    // buffers.
    struct Lane {
        DevBuf stats, stats_rsq, stats_blk, hs1, hs2, raw16, slab_raw, stats_hi, mask_td, sched;
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        // the lane's own side streams for a slab class (two slab classes on two lanes must neither share fork / join
        // events nor serialise on one set of side streams)
        std::vector<hipStream_t> slab_streams;
        std::vector<hipEvent_t> slab_done;
        hipEvent_t slab_fork = nullptr;
    };
    std::vector<Lane> lanes;                // lanes 1 .. n - 1
    bool slab_fork_early = false;           // run_score_classes recorded slab_fork ahead of the class's statistics pass
    hipEvent_t lane_fork = nullptr;
    hipEvent_t f32_built = nullptr;         // multi-lane calls: the float32 plane rebuilt after a banded upload (run_score_classes)
    int class_lanes = 2;                    // MTM_CLASS_LANES (1: classes one after another on the main stream)
    // side streams of a slab class: its raw launches are independent and (few templates, small images) far too small to
    // fill the chip one at a time
    std::vector<hipStream_t> slab_streams;
    std::vector<hipEvent_t> slab_done;
    hipEvent_t slab_fork = nullptr;
    std::vector<hipEvent_t> band_ev;
    int banded_cls = -1;                    // the size class a banded call runs under the upload (banded_ok)
    std::vector<double> upload_bands{0.25, 1.0};   // cumulative row fractions (MTM_UPLOAD_BANDS; 0.25 re-measured against
                                                   // 0.15 .. 0.35 with the tail-screened score kernel: still the fastest)
    // MTM_HOST_TRACE=1: host time stamps at the phases of a fused call, averaged and printed when the context is destroyed
    bool host_trace = false;
    double trace_acc[24] = {0};
    long long trace_n[24] = {0};
    long long trace_calls = 0;
    double trace_t0 = 0.0;

    // templates
    bool have_templ = false;
    bool placed = false;
    int method = MTM_TM_CCOEFF_NORMED;
    std::vector<HostTempl> templs;
    std::vector<SizeClass> classes;
    std::vector<TemplDev> td_host;
    std::vector<int> tlist_host;
    std::vector<int> list2d;        // templates with a 2-D score map
    int list2d_off = 0;
    size_t maps_floats = 0;
    std::vector<UnitSrc> usrc_host;                 // the unit views (device copy: usrc_dev), slab views appended at placement
    size_t usrc_units = 0;                          // entries that are units (the rest are slab views)
    std::vector<uint8_t> tstage;                    // host image of the source arena's prefix (set_templates_device)
    bool stage_pending = false;                     // copies from tstage / usrc_host may be in flight on `stream`
    bool place_pending = false;                     // copies from td_host / tlist_host may be in flight on `stream`
    DevBuf slab_raw;                                // raw int32 maps of the slabs
    // masked float32 classes screened on the bf16 matrix cores: the U / V template tables, the approximate c1 / c2 maps,
    // J = I^2, the window sums of I and J, the launches' tile constants, the list of outputs to re-score exactly
    DevBuf td_u, td_v, mbf_maps, f32_sq, mbf_stats, mbf_mu, mbf_list, mbf_best;
    bool f32_sq_valid = false;                      // f32_sq holds the square of the current float32 plane
    long long mbf_cap_debug = 0;                    // test support (mtm_debug_maskf32_screen): a list capacity below the production one; 0: none
    DevBuf mbf_dbg;                                 // ... and that entry's dump of the bounds
    DevBuf tsrc, usrc_dev, tsums_dev, tgather;      // template source arena, unit views, source sums, gather scratch
    DevBuf td, tlist, weights, packs, apacks, maps, hs1, hs2, stats, hits, counters, sched, cands, mask_td, chash, raw16, stats_hi, tsum, stats_rsq, stats_blk;

    // options
    int opt_kernel = MTM_KERNEL_AUTO;
    int opt_border = MTM_BORDER_NEAREST;   // scikit-image >= 0.19 (maximum_filter mode='nearest'); MTM_PEAK_BORDER=constant: <= 0.18
    // Capacity (records) of the candidate list and of the hit list.  2^18: measured in round 4 against 2^20 on a
    // photograph-like 4K image x 32 templates at threshold 0.5 (~1e6 outputs above the threshold): a list that holds them
    // all keeps the call in hits-only mode, but a million emissions cost the score kernel +0.64 ms (1.32 against 0.68 ms,
    // one atomic per wave and item) - more than map mode + the candidate test of the dense route; up to ~2.6e5
    // candidates the list is the cheaper way, and that is where it overflows.
    int64_t hit_cap = 1 << 18;
    int dot_variant = 0;
    int fuse_stats = 1;        // MTM_FUSE_STATS: single-kernel window statistics (0 = the two-pass kernels, which large windows and float32
                               // images use anyway: test_uint16_fused_window_statistics_bit_for_bit compares the two)
    int row_mux = 1;           // MTM_ROW_MUX: row-multiplexed MFMA tiling for classes of <= 16 templates (0 = the plain tiling:
                               // test_fused_global_extremum runs both)
    double band_min_fill = 1.0;   // MTM_BAND_MIN_FILL: a band is only worth a launch of its own if its work items fill the resident
                               // work-group slots this many times (0 lets the band tests use small images)
    int n_cus = 0;
    int hits_only = 1;         // MTM_OPT_HITS_ONLY: mtm_find_matches does not materialise the score maps when
                               // every class runs the single-channel MFMA kernel (candidates + hash verify)
    int backoff_len = 16;      // length of the next back-off period: doubles with every overflow in a row (<= 1024), reset by a
                               // call whose candidates fitted
    int fuse_backoff = 0;      // calls left without fused candidates (map mode + full peak pass: maps known to be dense)
    bool maps_valid = false;   // the map arena holds every score map of the last mtm_find_matches (mtm_last_score_map)
    CallRoute fm;                       // the route of the mtm_find_matches_async call in flight (mtm_find_matches_wait)
    bool fm_in_flight = false;
    const void* cands_zeroed = nullptr;   // candidate buffer whose counter was cleared after the previous call's fetch
    int exact_div = 1;         // MTM_OPT_EXACT_DIV: 1 (default since round 5) = IEEE division in the MFMA epilogue, bit-identical to the
                               // oracle; 0 = correctly rounded reciprocals (<= 1 ulp(float32) on ~1e-8 of the outputs); 2 = strict: also
                               // the fused extremum of masked classes (reciprocal-only kernels) goes through maps + extremum_kernel
    int auto_kernel = MTM_KERNEL_MFMA;   // what MTM_KERNEL_AUTO resolves to for uint8 classes (dot4 when not eligible)
    int batch_max_rows = mtmi::kBatchMaxRows;  // MTM_OPT_BATCH_MAX_ROWS: most stacked image rows in one chunk of mtm_find_matches_batch

    mtm_timing timing{};
    std::vector<mtm_hit> last_hits;     // result of the last mtm_find_matches (for mtm_last_hits)
    void* pin_small = nullptr;          // 64 page-locked bytes: landing place of small device-to-host copies (device NMS counters)
    void* pinned = nullptr;             // pinned host buffer the candidate records land in
    size_t pinned_cap = 0;
    void* comm_pin = nullptr;           // pinned staging of the hit exchange: [my slot | gathered slots]
    size_t comm_pin_cap = 0;
    std::vector<uint8_t> templ_blob;    // bytes of the templates of the last mtm_set_templates (unchanged-input test)
    uint64_t templ_gen = 0;             // bumped whenever templ_blob changes: what caches of the template set are keyed on
    // The window searches (mtm_find_matches_pyramid, mtm_find_matches_boxes): the templates' byte planes at win_toff[t] in
    // win_tpx (prepare_window_templates; made for the template set win_gen, whose bytes win_blob keeps so that the set
    // set again after others finds them), and the per-call score buffer, hit list and flags of the peak pass
    // (window_peak_pass).
    uint64_t win_gen = 0;
    std::vector<uint8_t> win_blob;
    DevBuf win_tpx, win_toff, win_buf, win_hits, win_flags;
    // mtm_find_matches_pyramid (mtm_pyramid.hip): the coarse level runs in a context of its own on the same device (its
    // templates are the downscaled ones, its image the downscaled planes made from this context's upload); pyr_gen /
    // pyr_factor: the template set and factor its templates were made for.  pyr_wins: the call's window table.
    mtm_ctx* pyr_sub = nullptr;
    uint64_t pyr_gen = 0;
    int pyr_factor = 0;
    DevBuf pyr_wins;
    // mtm_find_matches_boxes (mtm_boxes.hip): the templates' epilogue constants (box_td, made for the template set
    // box_gen), the per-call unit and tile tables.  boxes_max_floats: MTM_OPT_BOXES_MAX_FLOATS.
    uint64_t box_gen = 0;
    DevBuf box_td, box_units, box_tiles;
    int64_t boxes_max_floats = 1ll << 26;
    // mtm_track_boxes* (mtm_track.hip, stage_tables): the per-call unit table (TrackPlan::units, rewritten on the device
    // every frame), tile table (TrackPlan::tiles), one extremum key per unit and the records; the records' 3 x 3
    // neighbourhoods where a call returns them (nine floats per record).
    DevBuf trk_units, trk_tiles, trk_keys, trk_out, trk_nbhd;
    // mtm_track_boxes_adapt (stage_track_templates): the call's own templates, indexed by the track - byte planes (track
    // k's at trk_toff[k] in trk_tpx, prepare_window_templates' layout), epilogue constants (trk_td) - and each track's pass
    // flag of the frame.  Copies of win_tpx / box_td made at the start of the call and rewritten by track_adopt_kernel:
    // the template set's own tables and their generations are never touched.
    DevBuf trk_tpx, trk_toff, trk_td, trk_pass;
    // mtm_track_boxes_reacquire: the state of a frame's whole-frame search - per track its whole-frame unit and its lost
    // flag, the compacted list of the lost tracks and their count (TrackLostState, mtm_track.hip) - written by
    // track_update_kernel, read by track_reacquire_kernel, cleared by track_reupdate_kernel.
    DevBuf trk_lost;
    // mtm_track_boxes_sets: the first unit of every track's set in trk_units (TrackPlan::set_off, n_tracks + 1 offsets);
    // the other entry points hand the update kernels no offsets (track k is unit k).
    DevBuf trk_sets;
    // mtm_match_blocks (mtm_blocks.hip): the call's own templates - byte planes gathered from the reference image (block k's
    // at blk_toff[k] in blk_tpx, prepare_window_templates' layout, one chunk of blocks at a time) and the constants
    // blocks_gather_kernel computes for them (blk_td) -, the block records, the unit and tile tables (BlockPlan), one
    // extremum key per block and the records' 3 x 3 neighbourhoods.  The template set's tables (win_tpx, win_toff, box_td)
    // and their generations are never touched.  mtm_match_blocks_stack: one row of keys and neighbourhoods per pair, the
    // blocks' clip offsets (BlockPlan::clip) and the float64 sums of the ensemble planes (blk_acc: zeroed at the start of
    // a call, one writer per cell and launch).
    DevBuf blk_tpx, blk_toff, blk_td, blk_blocks, blk_units, blk_tiles, blk_keys, blk_nbhd, blk_clip, blk_acc;
    // mtm_match_blocks_at / _passes: the records of every pass (24 B per block, resident for the call) and the uploaded offsets
    DevBuf blk_recs, blk_offs;
    // mtm_match_blocks_passes_validated / mtm_debug_validate_blocks: blocks_validate_kernel's flag per record (1 B) and the
    // records that steer the next pass (the raw ones with every outlier's position replaced), pass-major as blk_recs
    DevBuf blk_valid, blk_steer;
    // mtm_match_blocks_second / mtm_match_blocks_passes_second / mtm_debug_second_peaks: the float32 scores of one launch
    // sub-range's maps (block k's oh x ow plane at blk_poff[k] floats, written by blocks_score_plane_kernel and read by
    // blocks_second_kernel behind it), the second-peak key per block and its record, pass-major as blk_recs
    DevBuf blk_plane, blk_poff, blk_keys2, blk_recs2;
    // mtm_match_blocks_passes_deformed / mtm_deform_image: the warped image's byte planes in the image
    // layout (plane c at c * u8_pitch * rows; uint16: the high-byte plane, then the low-byte plane XOR 0x80), the coarse
    // displacements of the pass that steers (8 B per block), the per-column and per-row weight tables of every deformed pass
    // and the field at every block's centre (Q8, 8 B per block, pass-major as blk_recs)
    DevBuf blk_warp, blk_disp, blk_dtab, blk_pred;
    // mtm_match_blocks_passes_steered with steer = 1: the unfiltered Q8 steering displacements of the pass that steers (8 B
    // per block; the filtered ones go into blk_disp)
    DevBuf blk_d8;
    // mtm_match_blocks_masked: the call's mask plane, rows x cols bytes, tightly packed - a buffer of its
    // own, not a third frame of the stack
    DevBuf blk_mask;
    // mtm_hit_neighbourhoods (mtm_subpixel.hip): the templates' operands (bytes, float64 weights, constants; made for the
    // template set sub_gen) and the per-call point table and scores.
    uint64_t sub_gen = 0;
    DevBuf sub_bytes, sub_wts, sub_td, sub_pts, sub_out;

    // RCCL
    void* rccl_lib = nullptr;
    ncclComm* comm = nullptr;           // ncclComm_t
    int n_ranks = 1, rank = 0;
    long long comm_slot_hits = 512;
    double comm_timeout_s = 300.0;      // deadline of one hit exchange (MTM_COMM_TIMEOUT_S; 0 = none)
    std::vector<unsigned long long> vh_keys;   // host verification of the candidate list: open-addressing table
    std::vector<int> vh_vals;
    DevBuf comm_send, comm_recv;
    std::vector<long long> comm_last_counts;   // per-rank counts of the last exchange (mtm_comm_last_gather)
    size_t comm_last_slot = 0;                 //   and its slot size in bytes; the slots are still in comm_pin
};

namespace mtmi {

inline double host_now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// phase `k` of the current call reached (k = 0: the call starts)
inline void host_trace(mtm_ctx* c, int k) {
    if (!c->host_trace) return;
    const double t = host_now_us();
    if (k == 0) {
        c->trace_t0 = t;
        ++c->trace_calls;
    }
    if (c->trace_calls <= 8) return;        // (the first calls create streams, events and buffers: not the steady state)
    c->trace_acc[k] += t - c->trace_t0;
    ++c->trace_n[k];
}

inline ImageDev image_dev(const mtm_ctx* c) {
    ImageDev d;
    d.u8 = c->slot[c->cur].u8.as<uint8_t>();
    d.f32 = c->slot[c->cur].f32.as<float>();
    d.rows = c->rows;
    d.cols = c->cols;
    d.chans = c->chans;
    d.u8_pitch = c->u8_pitch;
    d.f32_pitch = c->f32_pitch;
    d.u8_plane = (long long)c->u8_pitch * c->rows_alloc;
    d.f32_plane = (long long)c->f32_pitch * c->rows_alloc;
    return d;
}

// ---- geometry of the operand packs (shared by the placement and the launches)
constexpr int kMfmaMaxW = 256;          // widest template of one MFMA launch (wider: slabs)
// sum I^2 M of a masked class in ONE launch (MfmaParams::sq_fused): the int32 accumulator holds 256 a_h + a_l,
// a_x = sum (J_x - 128) M over the byte planes J_h, J_l of I^2, which reaches down to -(256 + 1) 128 n = -32896 n under a
// mask of n set taps over black pixels (and up to 126 * 256 - 127 = 32129 n over saturated ones: 255^2 = 0xFE01).  That fits an int32 up to
// n = 65280 - fewer than the 66051 taps mfma_class_ok admits, the uint16 path's kMfma16MaxArea over again
// (tests/test_gpu_masked_cores.py ran 256 x 256 and 258 x 256 full masks over dark scenes).  Masks with more set taps
// take the two raw launches + masksq_combine_kernel, which combines a_h and a_l in float64 (launch_masked_sumsq).
constexpr long long kMasksqFusedMaxOnes = 65280;
static_assert(32896 * kMasksqFusedMaxOnes <= 2147483648LL && 32896 * (kMasksqFusedMaxOnes + 1) > 2147483648LL,
              "256 a_h + a_l of the fused sum I^2 M pass must fit an int32");
inline long long mfma_group_bytes(int h, int w, int chans) { return (long long)chans * h * ((w + 63) / 64) * 1024; }
// packed K: MFMA steps (1 KiB of A operand each) of `rows` stream rows of nseg 16-tap segments
inline int kp_blocks(int rows, int nseg) { return (rows * nseg + 3) / 4; }
inline int mfma_groups_alloc(int n) { return (((n + 15) / 16) + 1) & ~1; }     // multiple of MB = 2
// Row-multiplexed packs (<= 16 uint8 templates, one channel, no mask): steps sp' = 0 .. h + 3R - 2, A row
// i = (template i % nt, row offset i / nt) holds template row sp' - R - i / nt (zero outside 0..h-1).
// MFMA group 0 of step s reads pack step s + R, group 1 (the wave's next R output rows) pack step s.
inline long long rm_pack_bytes(int h, int w, int R) { return (long long)(h + 3 * R - 1) * ((w + 63) / 64) * 1024; }
// bytes of one channel of a class's row-multiplexed pack.  Packed K: the two MFMA groups have packs of their own
// (group g, image row r of the h + 2R - 1 a wave walks: template row r - g R - rho), kp_blocks steps each - the shifted
// reuse of one pack (classic layout) would need R rows to be a whole number of 4-segment steps.
inline long long class_rm_pack_bytes(const SizeClass& sc) {
    return sc.kp_nseg ? 2LL * kp_blocks(sc.h + 2 * sc.rm_R - 1, sc.kp_nseg) * 1024 : rm_pack_bytes(sc.h, sc.w, sc.rm_R);
}
inline int bf16_nkb(int w) { return (w + 31) / 32; }
inline long long bf16_group_bytes(int h, int w, int chans) { return (long long)chans * h * bf16_nkb(w) * 1024; }
// bytes per LDS image-tile row of an ncc_mfma_kernel work-group over `nb` 64-tap blocks (MfmaParams::lds_pitch)
inline int mfma_lds_pitch(int nb) { return (16 + 4 * nb + 1) * 16; }
// image rows of a row-multiplexed tile (R output rows per MFMA group): a chunk of the h + 2R - 1 rows a wave walks, and
// 2R more for each further wave
inline int rm_tile_rows(int h, int R) { return std::min(h + 2 * R - 1, kMfChunkH) + (kMfRows - 1) * 2 * R; }
// templates per MFMA group of a row-multiplexed launch of n <= 16 templates h x w (R = 16 / nt rows each): the next power of
// two, doubled while the tile needs more than 72 KB - two work-groups per CU need <= ~76 KB of LDS each
inline int rm_group_templates(int n, int h, int w) {
    int nt = 1;
    while (nt < n) nt <<= 1;
    const size_t lds_pitch = (size_t)mfma_lds_pitch((w + 63) / 64);
    while (nt < 16 && (size_t)rm_tile_rows(h, 16 / nt) * lds_pitch > 72 * 1024) nt <<= 1;
    return nt;
}
// longest candidate list a score kernel appends to (mtm_ctx::cands; a larger hit_cap only sizes the hit buffers)
constexpr int64_t kCandListMax = 4096LL * 256;
inline unsigned long long cand_list_cap(const mtm_ctx* c) { return (unsigned long long)std::min<int64_t>(c->hit_cap, kCandListMax); }

// the image of a fused "upload + search" call (mtm_find_matches_image)
struct ImageArgs {
    const void* px;
    int rows, cols, chans, dtype;
    int64_t stride;
};
// Geometry of the planar device copies of an image (after an optional integer downscale).
struct SlotGeom {
    int rows, cols, rows_alloc, pitch;
    size_t u8_bytes;
};

// Error of a bf16-piece correlation relative to sqrt(sum (I - mu)^2 * sum (T - centre)^2) (Cauchy-Schwarz): 2^-15 covers the
// dropped piece products and the two 16-bit representations (3 * 2^-18 + the float32 rounding of I - mu), the rest the
// float32 accumulation - three MFMAs per 32-tap block, counted as TWO roundings of 2^-24 each (the matrix core's own
// 32-term sum is not documented as a single rounding; tests/test_gpu_parity.py::test_float32_error_bound_holds measures
// the whole bound against the float64 kernel on adversarial and random data).
// Round 6 (advisor): the whole is doubled.  The "two roundings per MFMA" is an assumption about undocumented hardware; the
// measured worst case is 0.16 of the undoubled bound, so the factor costs a few more exact re-scores and buys a guarantee that
// survives an ASIC or compiler whose accumulation is a little worse than assumed.
// (Round 6, second look at the first term: bfloat16 carries 8 significant bits, unit roundoff 2^-8, so two pieces represent a
// float to 2^-16 and the three neglected terms - I's residual, T's residual, I1 T1 - are 3 * 2^-16 = 4.6e-5 of |I||T| per tap,
// not the "3 * 2^-18" the 2^-15 above was written for; the doubled total, 6.1e-5 + ..., still covers it.)
// np == 1 (the one-product screen, ncc_bf16_kernel<MB, 1>): only I0 T0 is summed.  |I T - I0 T0| <= |I - I0||T| + |I0||T - T0|
// <= (2^-8 + 2^-8 (1 + 2^-8)) |I||T| = 2^-7 (1 + 2^-9) |I||T| per tap, Cauchy-Schwarz over the taps; ONE MFMA per 32-tap block,
// two roundings each, doubled like the rest for the undocumented accumulation.
inline bool f32_refined(const mtm_ctx* c) { return c->f32_mfma == 1 || c->f32_mfma == 3; }
inline float bf16_rig_eps(int chans, int h, int nkb, int np = 3) {
    if (np == 1) return (float)(0.0078125 * 1.002 + 2.0 * (2.0 * 1.0 * (double)chans * h * nkb * 5.97e-8));
    return (float)(2.0 * (3.0518e-5 + 2.0 * 3.0 * (double)chans * h * nkb * 5.97e-8));
}
// ... and what the refined raw-sum extremum (Bf16Params::ext_eps) works with
inline float bf16_ext_eps(int chans, int h, int nkb, int np = 3) {
    if (np == 1) return bf16_rig_eps(chans, h, nkb, 1);
    return (float)(3.0518e-5 + 3.0 * (double)chans * h * nkb * 5.97e-8);
}

// ---- mtm_context.hip
int prepare_slot(mtm_ctx* c, mtm_ctx::ImageSlot& sl, int src_rows, int src_cols, int chans, int dtype, hipStream_t stream,
                 int factor, SlotGeom* out);
int upload_rows_u8c1(mtm_ctx::ImageSlot& sl, const SlotGeom& g, const void* src, int64_t src_stride, int r0, int r1,
                     hipStream_t stream, bool skip_f32, hipEvent_t copy_done = nullptr, hipEvent_t before_kernels = nullptr,
                     bool convert = true);
int upload_rows_u16c1(mtm_ctx::ImageSlot& sl, const SlotGeom& g, const void* src, int64_t src_stride, int r0, int r1,
                      hipStream_t stream, hipEvent_t copy_done = nullptr, hipEvent_t before_kernels = nullptr);
int upload_image(mtm_ctx* c, mtm_ctx::ImageSlot& sl, const void* src, int64_t src_stride, int src_rows, int src_cols,
                 int chans, int dtype, hipStream_t stream, int factor = 1);
int upload_image_stack(mtm_ctx* c, mtm_ctx::ImageSlot& sl, const void* const* px, int n, int64_t src_stride, int rows,
                       int cols, int chans, int dtype, hipStream_t stream);
// Two images of one shape as one image of 2 * rows rows, each copied from its own rows and stride (mtm_match_blocks).
int upload_image_pair(mtm_ctx* c, mtm_ctx::ImageSlot& sl, const void* px0, int64_t stride0, const void* px1, int64_t stride1,
                      int rows, int cols, int chans, int dtype, hipStream_t stream);
void adopt_image(mtm_ctx* c, int rows, int cols, int chans, int dtype);
// Frames of rows x cols x chans pixels per stacked chunk of a tracking call (mtm_track.hip; mtm_match_blocks_stack sizes
// its chunks with it): MTM_OPT_BATCH_MAX_ROWS and the device memory of the stack's planes, at least one.
int track_chunk_frames(const mtm_ctx* c, int rows, int cols, int chans);
// (BlobTempl: mtm_internal.h)
int parse_templ_blob(const std::vector<uint8_t>& b, std::vector<BlobTempl>& out, const char* who, bool u16_ok);
int prepare_window_templates(mtm_ctx* c, const std::vector<BlobTempl>& tl);
// The templates' epilogue constants (TemplDev, statistics of the last mtm_set_templates and the sizes of `tl`) in
// mtm_ctx::box_td, uploaded once per template set (mtm_boxes.hip; the boxes and tracking searches).
int prepare_box_td(mtm_ctx* c, const std::vector<BlobTempl>& tl);
// The planes of `dst`'s current slot from the raw uint8 image already in `src` (src_rows x src_cols, tightly packed),
// area-downscaled by `factor` on `stream`; `dst` adopts the downscaled image (mtm_find_matches_pyramid's coarse level).
int derive_downscaled_u8(mtm_ctx* dst, const mtm_ctx::ImageSlot& src, int src_rows, int src_cols, int chans, int factor,
                         hipStream_t stream);
int check_image_args(const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes, const char* who);
int ensure_f32_plane(mtm_ctx* c);
int upload_rows_f32c1(mtm_ctx::ImageSlot& sl, const SlotGeom& g, const void* src, int64_t src_stride, int r0, int r1, hipStream_t stream);
int ensure_copy_stream(mtm_ctx* c);
int ensure_lanes(mtm_ctx* c, int n);
// ---- mtm_comm.hip
int comm_allgather_hits_flagged(mtm_ctx* c, const mtm_hit* local, int64_t n_local, int32_t my_flag, mtm_hit* out,
                                int64_t capacity, int64_t* counts_out, int64_t* n_out, std::vector<int32_t>* flags_out);
// ---- mtm_placement.hip
int place_templates(mtm_ctx* c);
// ---- mtm_stats.hip: the host side of the window statistics (the only unit that launches mtm_k_stats.hip.h)
// What the launchers of the two-pass chains take - a stream, device pointers and these, nothing of a context:
struct StatGeom {           // an h x w window over `chans` planes of rows x cols pixels
    int rows, cols, chans, h, w, oh, ow;
    double inv_area;
};
inline StatGeom stat_geom(int rows, int cols, int chans, int h, int w) {
    return StatGeom{rows, cols, chans, h, w, rows - h + 1, cols - w + 1, 1.0 / ((double)h * (double)w)};
}
struct StatScratch {        // the row sums between the two passes: `chans` planes of rows x pitch (uint32 or double) each
    void* hs1;
    void* hs2;
    int pitch;
    long long plane;
};
struct StatOut {            // the planes to write (st_pitch doubles a row, oh rows); a null plane goes with its flag off
    int num_type = 0, want_sq = 0, want_t = 0, want_sum2 = 1;       // (the two-pass chains write sum2 whatever is asked)
    double* t[kMaxChans] = {nullptr, nullptr, nullptr, nullptr};
    long long t_plane = 0;  // the fused RGB kernel: doubles from t[0] to t[1] to t[2]
    double* sum2 = nullptr;
    double* sq = nullptr;
    int st_pitch = 0;
};
// F64_LDS: hsum_lds_kernel (w <= kStatsHsumLdsMaxW) over the image rows [r0, r1) + vsum over the output rows [o0, o1) - the
// whole image, or the rows a band of a banded upload brought and the windows they complete (launch_stats; mbf_prepare)
int launch_stats_f64_lds(hipStream_t stream, const float* f32, int pitch, long long plane, const StatGeom& g,
                         const StatScratch& s, const StatOut& o, int r0, int r1, int o0, int o1);
// What a band of a banded upload asks of launch_stats; the default: the whole image, on the context's stream.
struct StatBand {
    hipStream_t stream = nullptr;   // the stream of a banded call's statistics launches (null: no banded call, c->stream)
    int sb0 = 0, sb1 = -1;          // the kStatBand4-row units of output rows to compute (fused kernels, F64_LDS), sb1 < 0 = all
    int lay_r0 = 0, lay_r1 = 0;     // the image rows that have just arrived - fused uint8: the rows whose layout this launch
                                    // converts; F64_LDS: the rows whose horizontal sums it adds
};
// Window statistics of one size class into c->stats; *out: the plane table its score launch reads.
int launch_stats(mtm_ctx* c, CallRoute& R, const SizeClass& sc, StatPlanes* out, const StatBand& band = {});
// ---- mtm_launch.hip
bool dot_variant_ok(int64_t v);
// the tail screen's split for a launch of class `sc` on route R (MfmaParams::tail_split), 0 = off
int tail_split_for(const mtm_ctx* c, CallRoute& R, const SizeClass& sc);
// ... and the templates' tail constants for it, re-derived on the score stream where the last ones were another split's
int ensure_tail_consts(mtm_ctx* c, const SizeClass& sc, int split);
// sum I^2 M of a masked class on the int8 matrix cores into `sum2`, the sum2 plane of `st` (launch_stats' last step)
int launch_masked_sumsq(mtm_ctx* c, const SizeClass& sc, bool fused_stats, const StatPlanes& st, double* sum2);
// the tail constants of class `sc` for `split` (tail_consts_kernel -> TemplDev::tail_*), queued on `stream`
int launch_tail_consts(mtm_ctx* c, const SizeClass& sc, int split, hipStream_t stream);
int launch_ncc(mtm_ctx* c, CallRoute& R, const SizeClass& sc, int list_off, int n_list, const StatPlanes& st, int only_li = -1,
               int yb0 = 0, int yb1 = -1);
int ensure_maps(mtm_ctx* c);
int run_score_all(mtm_ctx* c, CallRoute& R);
bool banded_ok(mtm_ctx* c, const ImageArgs& a, bool* single_band);
int run_score_banded(mtm_ctx* c, CallRoute& R, const ImageArgs& a);
int collect_ncc_time(mtm_ctx* c);

// ---- mtm_peaks.hip: the host side of the peak pass (the only unit that launches mtm_k_peaks.hip.h and mtm_k_nms.hip.h)
constexpr size_t kHitPrefetch = 1024;       // candidate / hit records fetched together with the counters
// The hit buffer of a peak pass (mtm_ctx::hits), as the kernels read it: [hit count | candidate count | spare word of the
// candidate header (float32 map mode: the "bound too wide" flag) | one int per template] [records].  The header and the
// first kHitPrefetch records come back in ONE copy.
struct HitBuffer {
    size_t hdr_bytes;
    uint8_t* base = nullptr;        // on the device
    explicit HitBuffer(int n) : hdr_bytes(round_up(3 * sizeof(unsigned long long) + sizeof(int) * (size_t)std::max(1, n), 16)) {}
    unsigned long long* count() const { return reinterpret_cast<unsigned long long*>(base); }
    unsigned long long* cand_header() const { return count() + 1; }        // two words, as the candidate buffer starts
    int* flags() const { return reinterpret_cast<int*>(count() + 3); }
    mtm_hit* records() const { return reinterpret_cast<mtm_hit*>(base + hdr_bytes); }
    // a host copy of the header
    struct Header {
        unsigned long long count, ncand;
        unsigned rig_wide;
    };
    Header decode(const uint8_t* host, int n, int* tflags) const {
        Header h{};
        std::memcpy(&h.count, host, sizeof(h.count));
        std::memcpy(&h.ncand, host + sizeof(h.count), sizeof(h.ncand));
        std::memcpy(&h.rig_wide, host + 2 * sizeof(h.count), sizeof(h.rig_wide));
        std::memcpy(tflags, host + 3 * sizeof(h.count), sizeof(int) * (size_t)n);
        return h;
    }
    const uint8_t* host_records(const uint8_t* host) const { return host + hdr_bytes; }
};
// The device's share of the non-maxima suppression (mtm_k_nms.hip.h), queued right behind the peak pass: the length of the
// peak list is still on the device, the launches read it there and do nothing unless it lies in [nms_device_min, n_max].
// What a neighbourhood's best hit suppresses stays on the device; fetch_peak_list brings the rest: first the hits that are
// certainly kept (nothing earlier overlaps them), then the undecided ones.
struct DeviceNms {
    bool queued = false;
    unsigned n_max = 0;
    const unsigned long long* cnt_pin = nullptr;   // landing buffer of the two counters (champions, undecided), page-locked
    const mtm_hit* out = nullptr;
};
// fm_begin: the first max_records records of the candidate buffer `cands` and its header -> the pinned landing buffer
int queue_cand_fetch(hipStream_t stream, const void* cands, void* pinned, size_t max_records);
// One attempt of the device's peak pass, queued: the candidate list verified (against the hash table of its positions, or
// the maps), else the maps scanned (the flagged segments, with compaction and the device's share of a suppression request,
// or everything).
int queue_peak_pass(mtm_ctx* c, const CallRoute& R, HitBuffer& hb, DeviceNms* dnms);
// The one copy behind a peak pass - header + first kHitPrefetch records into host_buf - and what it says: the number of
// peaks, the per-template ints, what overflowed.  Records ev[2].
int fetch_pass_outcome(mtm_ctx* c, const CallRoute& R, const HitBuffer& hb, std::vector<uint8_t>& host_buf, int* tflags,
                       unsigned long long* count, PassOutcome* o);
// The `count` peaks of a pass whose lists held everything: from host_buf and, beyond the prefetched ones, the device.
// Thousands of peaks and a suppression request: decided on the device, only the kept ones are fetched.
int fetch_peak_list(mtm_ctx* c, CallRoute& R, const HitBuffer& hb, const std::vector<uint8_t>& host_buf, unsigned long long count,
                    const int* tflags, const DeviceNms& dnms, std::vector<mtm_hit>& hits);
// MTM_PEAKS_GLOBAL without the fused extremum (R.ext: nothing to do): mtm_ctx::counters cleared, extremum_kernel over the maps
int queue_extremum_pass(mtm_ctx* c, const CallRoute& R);
// mtm_find_matches_batch, the maps of a stack of nb images of `rows` rows in memory: the per-image extremum, or the
// seam-aware scan (a list that overflows grows mtm_ctx::hit_cap and runs once more) -> image b's records, unsorted, appended
// to per_img[b].  Records ev[2].
int batch_peak_pass(mtm_ctx* c, int mode, float thr, bool mode_min, int nb, int rows, std::vector<mtm_hit>* per_img);
// The peak pass of the window searches over n slots (pyramid: templates, boxes: units).  Flags laid out as
// [u64 record count][u64 best key x n][int nontrivial x n] are zeroed, `launch` enqueues the peak kernels (and anything that
// must follow them before the read-back) writing records to (hits, cap), the flags come back in one copy; a list that
// overflowed runs once more with room for every record.  Global mode: the best key per slot into `best`.  Local mode: the
// records of the slots flagged nontrivial, unsorted, appended to `recs`.  The list starts at mtm_ctx::hit_cap records and
// grows for this call only: hit_cap is left as it is (later mtm_find_matches routes size candidate lists by it).
using WindowPeakLaunch = std::function<int(mtm_hit* hits, unsigned long long cap, unsigned long long* counter,
                                           unsigned long long* best, int* nontrivial)>;
int window_peak_pass(mtm_ctx* c, int n, bool global, const WindowPeakLaunch& launch, std::vector<unsigned long long>& best,
                     std::vector<mtm_hit>& recs, const char* who);
// ---- mtm_api.hip
int ladder_exhausted();        // the error of a call whose overflow fallbacks ran out of passes

}  // namespace mtmi
