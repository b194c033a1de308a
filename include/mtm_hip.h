/*
 * mtm_hip.h - C ABI of libmtm_hip.so, the MI355X (gfx950) implementation of the
 * Multi-Template-Matching hot path.
 *
 * The reference (multi-template-matching/MultiTemplateMatching-Python) has no FFI of its own: it
 * is pure Python calling OpenCV / scikit-image / scipy.  The boundary this library sits behind is
 * therefore the set of third-party calls on the reference's hot path; each entry point below
 * names the reference call site(s) it replaces (file:line in the reference tree).  The Python
 * host layer (multitemplatematching-python_amd/MTM) binds these with ctypes and re-exposes the
 * reference's module-level API unchanged; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 on success or a negative MTM_E_* code;
 *     mtm_last_error() returns a thread-local message for the last failure on this thread.
 *   - the caller owns every host buffer for the duration of a call; the library owns all device
 *     memory, freed in mtm_ctx_destroy().
 *   - images are row-major, (rows, cols) or (rows, cols, chans) interleaved, with an explicit row
 *     stride in bytes (numpy views with contiguous pixels are passed without a copy).
 *   - a context is bound to one GPU and is single-caller (not re-entrant); calls block until
 *     their results are on the host unless documented otherwise.
 */
#ifndef MTM_HIP_H
#define MTM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when a declaration below changes.  Entry points added since 9 - mtm_find_matches_pyramid,
 * mtm_find_matches_boxes, mtm_track_boxes, mtm_hit_neighbourhoods, mtm_track_boxes_nbhd, mtm_track_boxes_adapt,
 * mtm_debug_templ_stats, mtm_track_boxes_reacquire, mtm_track_boxes_sets, mtm_debug_device_nms, mtm_debug_peak_pass, mtm_debug_window_stats, mtm_match_blocks, mtm_debug_plan_blocks, mtm_match_blocks_stack, mtm_debug_plan_blocks_stack, mtm_debug_window_stats_route, mtm_match_blocks_at, mtm_match_blocks_passes, mtm_debug_plan_blocks_passes, mtm_match_blocks_passes_validated, mtm_debug_validate_blocks, mtm_match_blocks_second, mtm_match_blocks_passes_second, mtm_debug_second_peaks, mtm_deform_image, mtm_match_blocks_passes_deformed, mtm_debug_maskf32_screen, mtm_match_blocks_passes_steered, mtm_deform_image_q8, mtm_debug_steer_q8, mtm_debug_tail_consts, mtm_match_blocks_masked - are new symbols only and left it at 9: a caller built against an older 9 finds every function it knows unchanged (resolve the new ones by name). */
#define MTM_ABI_VERSION 9

/* pixel types (after the dtype policy of MTM/__init__.py:71-74: uint8 stays, all else float32) */
#define MTM_U8  0
#define MTM_F32 1
#define MTM_U16 2   /* the reference casts uint16 to float32 (exactly) before cv2; passing the uint16 pixels as they
                       are gives the same results (every sum is an exact integer) and lets single-channel
                       uint16 image + uint16 templates run on the int8 matrix cores (byte-plane decomposition)
                       instead of the float64 kernel */

/* OpenCV's TemplateMatchModes values, used as raw ints by the reference
 * (MTM/__init__.py:56,95,247 defaults; :78,:216,:227,:232 comparisons) */
#define MTM_TM_SQDIFF        0
#define MTM_TM_SQDIFF_NORMED 1
#define MTM_TM_CCORR         2
#define MTM_TM_CCORR_NORMED  3
#define MTM_TM_CCOEFF        4
#define MTM_TM_CCOEFF_NORMED 5

/* peak extraction mode */
#define MTM_PEAKS_LOCAL  0   /* MTM/__init__.py:231-235: local maxima (methods 2-5) / minima (0,1) */
#define MTM_PEAKS_GLOBAL 1   /* MTM/__init__.py:225-230: N_object == 1, cv2.minMaxLoc              */

/* 3x3 maximum-filter border rule of skimage.feature.peak_local_max (MTM/__init__.py:45; the reference leaves
 * scikit-image unpinned, setup.py:24).  The two rules differ only where the filtered map is negative at its
 * border: local MINIMA (methods 0/1, the map is negated, MTM/__init__.py:53) and negative thresholds. */
#define MTM_BORDER_CONSTANT 0  /* skimage <= 0.18: pad with 0 (border minima are never peaks) */
#define MTM_BORDER_NEAREST  1  /* skimage >= 0.19: replicate the edge - the default */

/* kernel selection for the uint8 score-map path (mtm_set_option MTM_OPT_KERNEL) */
#define MTM_KERNEL_AUTO  0
#define MTM_KERNEL_NAIVE 1   /* one thread per output pixel, scalar loop: the in-library cross-check */
#define MTM_KERNEL_DOT4  2   /* LDS-tiled sliding window on v_dot4_u32_u8 */
#define MTM_KERNEL_MFMA  3   /* implicit-GEMM sliding window on v_mfma_i32_16x16x64_i8 */
#define MTM_KERNEL_MFMA16 4  /* reported in mtm_timing.kernel_used only: uint16 pixels as four byte-plane
                                correlations on the MFMA kernel (selected by MTM_KERNEL_AUTO / _MFMA) */

#define MTM_KERNEL_MFMA_F32 5 /* reported in mtm_timing.kernel_used only: float32 pixels as two bfloat16 pieces on the
                                bf16 matrix cores, ~1e-5 of the normalised score (selected by MTM_KERNEL_AUTO /
                                _MFMA for unmasked float32 image + templates; MTM_F32_MFMA=0: float64 kernel) */

#define MTM_OPT_KERNEL      1
#define MTM_OPT_PEAK_BORDER 2
#define MTM_OPT_HIT_CAPACITY 3
#define MTM_OPT_DOT4_VARIANT 4  /* register-blocking variant of the dot4 kernel (tuning) */
#define MTM_OPT_EXACT_DIV 5     /* 1 (default since round 5: measured free on the hits-only path): IEEE division in the MFMA
                                   epilogue, bit-identical to the other kernels and to the oracle;
                                   0: correctly rounded reciprocals, <= 1 ulp(float32) on ~1e-8 of the pixels (round 1-4's
                                   default; what the fused global extremum of MASKED classes still uses under 1);
                                   2: strict - that extremum too goes through maps + extremum_kernel */
#define MTM_OPT_HITS_ONLY 6     /* 1 (default): mtm_find_matches does not write the score maps to memory when every
                                   template runs the int8 MFMA kernel: in local-extrema mode the peaks come from
                                   the in-kernel candidate list, in global-extremum mode (unmasked 1- or
                                   3-channel templates) the per-template best is kept inside the score kernel;
                                   0: always materialise the maps.  Results are identical either way. */
#define MTM_OPT_F32_MFMA 7      /* float32 images (every non-uint8, non-uint16 input: MTM/__init__.py:71-74), unmasked
                                   templates; the normalised methods, and the raw-sum methods for the global extremum
                                   and for local extrema against a threshold (listed by rigorous per-pixel error bounds
                                   of the sum, re-scored exactly; the raw sums' maps always take the float64 kernel).
                                   1 (default): scores on the bf16 matrix cores (within ~1e-5 of cv2's float64 result)
                                   as a SCREEN - every output whose exact score COULD be a peak, the global extremum or
                                   pass the threshold is re-scored with the float64 arithmetic of the exact kernel.
                                   Since round 5 "could" is decided by a per-output error bound, not by margins:
                                   |bf16 ratio - exact ratio| <= eps sqrt(sum (I - mu)^2) / sq * (sqrt(sum (T - mean)^2) /
                                   templ_norm), large where it has to be (a low-contrast window beside a much brighter
                                   region) and ~5e-5 on textured windows (one hardware assumption, stated in
                                   bf16_rig_eps and measured by tests/test_gpu_parity.py::test_float32_error_bound_holds);
                                   mtm_find_matches then returns the exact kernel's hit lists.  Round 6: where only a list
                                   leaves the kernel (hits-only mode: local extrema against a threshold, the global
                                   extremum, templates with masks) the screen first runs with ONE bfloat16 piece product
                                   instead of three - a third of the matrix-core work, eps ~2^-7 instead of ~2^-15, the
                                   same bound and the same exact re-scoring, so the same lists; a list that overflows
                                   repeats the launch with three products and the next calls start there
                                   (mtm_timing.f32_pieces says which ran).  Score maps read back with mtm_score_map keep
                                   the ~1e-5 tolerance (three products, always);
                                   0: the float64 kernel for everything (10x slower, maps exact to rounding);
                                   2: bf16 scores as they are, no re-scoring;
                                   3: as 1 without the one-product tier;
                                   4: diagnostic - as 2 with one piece product (the screen's raw scores: what the tests
                                   measure its bound on; never a result).  Environment: MTM_F32_MFMA. */
#define MTM_OPT_BATCH_MAX_ROWS 8 /* mtm_find_matches_batch: the most stacked image rows in one chunk (1 .. 65535, the default:
                                   the tightest bound a tall map has to respect, kBatchMaxRows in csrc/mtm_ctx.h).  A chunk
                                   holds at least one image; smaller values only split a batch into more chunks. */
#define MTM_OPT_BOXES_MAX_FLOATS 9 /* mtm_find_matches_boxes: the most unit score-map floats held on the device at once
                                   (default 2^26, 256 MB).  Units whose maps together exceed it run in chunks of whole units
                                   (a chunk holds at least one unit); results do not depend on it. */

/* error codes */
#define MTM_OK            0
#define MTM_E_INVALID    -1  /* bad argument */
#define MTM_E_HIP        -2  /* a HIP runtime call failed (message has the hipError string) */
#define MTM_E_NO_DEVICE  -3  /* no usable GPU */
#define MTM_E_STATE      -4  /* call order: image / templates not set */
#define MTM_E_OVERFLOW   -5  /* output buffer too small; *n_out holds the required capacity */
#define MTM_E_COMM       -6  /* RCCL failure */

typedef struct mtm_ctx mtm_ctx;

/* One template ("unit": a template, or a rotation/scale variant the caller appended to
 * listTemplates).  mask == NULL for no mask; a mask has the template's shape and dtype
 * (the policy of MTM/__init__.py:76-88 is applied by the host layer before this call). */
typedef struct mtm_templ {
    const void* px;
    const void* mask;
    int32_t rows, cols, chans, dtype;
    int64_t row_stride;       /* bytes */
    int64_t mask_row_stride;  /* bytes */
} mtm_templ;

/* One detection: the record MTM builds at MTM/__init__.py:241 (label replaced by the template's
 * index in the list).  24 bytes; also the record exchanged between ranks. */
typedef struct mtm_hit {
    int32_t templ_idx;
    int32_t x, y, w, h;
    float   score;
} mtm_hit;

/* One (region, template) pair of mtm_find_matches_boxes: a template of the last mtm_set_templates and the region of the
 * image it is searched in, rows y0 .. y0 + rows - 1 and columns x0 .. x0 + cols - 1 (already clipped to the image). */
typedef struct mtm_box_unit {
    int32_t templ_idx;
    int32_t y0, x0, rows, cols;
} mtm_box_unit;

/* One hit of mtm_hit_neighbourhoods: a template of the last mtm_set_templates and the window (x, y) of its score map at the
 * centre of the neighbourhood. */
typedef struct mtm_point {
    int32_t templ_idx, x, y;
} mtm_point;

/* timing of the last mtm_find_matches call, measured with HIP events on the context's stream */
typedef struct mtm_timing {
    float total_ms;      /* first kernel launch -> last kernel done.  Calls whose image arrives in row bands
                            (mtm_find_matches_image, one bandable size class) start this clock once the FIRST band's copy is
                            on its way - with a pageable source that copy call blocks the host while the rows are staged -
                            so total_ms of a banded call excludes up to that band's upload (25 % of the image by default);
                            unbanded calls include the whole upload.  Wall-clock figures (bench.py `value`) are not affected. */
    float score_ms;      /* window statistics + score-map kernels                        */
    float peaks_ms;      /* peak-extraction kernels                                      */
    float ncc_kernel_ms; /* the dominant score-map kernel(s) alone: time during which at least one launch ran */
    int32_t ncc_launches;
    int32_t kernel_used; /* MTM_KERNEL_* actually dispatched for the uint8 path           */
    int64_t n_hits;
    int32_t hits_only;   /* 1: the last mtm_find_matches ran without materialising the score maps; 2: maps in memory and
                            the peak pass over the flagged row segments only (dense images) */
    float   sclk_mhz;    /* shader clock the score kernel ran at, measured inside it (s_memtime ticks per
                            s_memrealtime tick x 100 MHz) by one mid-grid work-group; 0 when not measured */
    float   ncc_sum_ms;  /* plain sum of the score-kernel launch durations (= ncc_kernel_ms unless launches of a
                            banded call overlapped; what a profiler's per-launch average times the count gives) */
    int32_t f32_route;   /* float32 images on the bf16 matrix cores (MTM_OPT_F32_MFMA = 1), how the exact decisions were
                            reached: 0 not such a call, 1 kernel candidates re-scored, 2 map scan + neighbourhoods
                            re-scored, 3 the float64 kernel after all (lists overflowed, or classes it has to run anyway), 4 (round 6)
                            templates with masks: two raw bf16 correlations as a screen, every output that could pass the threshold
                            re-scored with the float64 kernel's own chains, "below" placeholders elsewhere (maps not published) */
    int32_t sq_launches; /* masked classes on the matrix cores: launches of the sum I^2 M pass (one per masked class) ... */
    float   masked_stat_ms; /* ... and the time they took (sum of the passes' own event pairs; 0 without masked classes) */
    int32_t f32_pieces;  /* (ABI 8) float32 images: bfloat16 piece products of the last matrix-core launch - 3 (scores to ~1e-5), or 1:
                            the one-product screen of the hits-only refined routes (f32_route 1 and 4; listing by a bound of
                            2^-7 of the norms' product, exact re-scoring decides; an overflowing list repeats the launch with 3);
                            0: no such launch */
} mtm_timing;

/* ---- device / context ------------------------------------------------------------------- */
int         mtm_abi_version(void);
int         mtm_device_count(void);                 /* 0 when no GPU is visible */
const char* mtm_last_error(void);
int         mtm_ctx_create(mtm_ctx** out, int device_id);
void        mtm_ctx_destroy(mtm_ctx* ctx);
int         mtm_set_option(mtm_ctx* ctx, int option, int64_t value);
int         mtm_get_option(mtm_ctx* ctx, int option, int64_t* value);     /* the current value of an MTM_OPT_* option */
/* Test support (ABI 7; nothing of the reference's interface corresponds to it).  The reference's functions are pure
 * functions of their arguments (MTM/__init__.py:92, :238-241); a kernel that reads memory it did not write in this call -
 * register-spill slots, LDS, a recycled work buffer - breaks that silently, depending on what earlier launches of the
 * process left behind (round 5's uint16 finding).  This call leaves a byte pattern (0xFF: NaN as float32 /
 * float64; 0x7F: huge finite values) in the places such a read would hit: every wave slot's scratch memory, every CU's
 * LDS, and the context's per-call work buffers.  tests/test_gpu_parity.py runs it ahead of every parity test. */
#define MTM_POISON_SCRATCH 1
#define MTM_POISON_LDS     2
#define MTM_POISON_ARENAS  4
int         mtm_debug_poison(mtm_ctx* ctx, int pattern_byte, int what);
/* Test support (ABI 9).  The IEEE-division epilogues of the single-channel uint8 score kernel obtain (float)(num / t) -
 * the value OpenCV's common_matchTemplate stores, SURVEY 8a-5 - from a reciprocal product plus an integer test that sends the
 * quotients next to a float32 rounding boundary through the division itself (csrc/mtm_device_util.hip.h,
 * quotient_as_float).  This call runs that function against the division on n_cases operand triples shaped like the
 * epilogue's, half of them constructed to straddle a rounding boundary (both instantiations of the function: the general
 * one, which also guards quotients in the float32 denormal range, and the epilogues', whose operands cannot produce
 * those): out4 = {cases run, results that differ in any
 * bit (must be 0), cases that took the division, largest |num * rr - num / t| seen in ulp(double) (the bound in the
 * source is 6, the test's margin 32)}. */
int         mtm_debug_quotient_check(mtm_ctx* ctx, uint64_t n_cases, uint64_t seed, uint64_t* out4);
/* Test support (added under ABI 9; host only, needs no GPU).  The number of K steps after which the two-row score kernel
 * of an h x w uint8 class screens its waves against the tail bound, as the library derives it from a call's candidate
 * threshold thr: the smallest s in [6, h - 2] with thr - (h - s + 1) / h >= z sqrt(s / h) / sqrt(w h), or 0 where the call
 * runs unscreened (no such s, a negative threshold, s / h above the measured cut-off).  The environment variable
 * MTM_TAIL_SPLIT=<s> (read when a context is created) forces a split instead, clamped to [6, h - 2]. */
int         mtm_debug_tail_split(int h, int w, double thr);
/* Test support (added under ABI 9; host only, needs no GPU).  The constants mtm_set_templates computes for an unmasked
 * template under `method` (0..5): px = rows x cols pixels of `chans` interleaved channels (1..4), tightly packed, dtype
 * MTM_U8, MTM_U16 or MTM_F32.  out7 = mean[0..3] (the channel means, zeroed where the method does not centre), templ_norm,
 * templ_sum2, all_ones (1.0: TM_CCOEFF_NORMED with a constant template, whose map is 1 everywhere) - the record
 * mtm_track_boxes_adapt returns per track in stats_out, computed there on the device by the same inline function. */
int         mtm_debug_templ_stats(const void* px, int rows, int cols, int chans, int dtype, int method, double* out7);
/* Test support (added under ABI 9; launches nothing).  The tiling place_templates chose for every size class of the
 * template set placed on the context (after a search, mtm_find_matches or mtm_score_map), in placement order:
 * MTM_CLASS_TILING_FIELDS int32 per class - h, w, n_templates, kernel (MTM_KERNEL_*), rm_nt, rm_R (row-multiplexed: templates
 * and output rows per MFMA group, 0 = not), kp_nseg (packed K: 16-tap segments per template row, 0 = not), r2 (2 = two-row
 * tiling), tail_ok (the two-row class can screen its K loop), tail_split (the split the class's last score launch carried,
 * 0 = it ran unscreened), n_slabs, slab_nt (slabs of a large-template class; templates per MFMA group of their
 * row-multiplexed launches, 0 = plain launches), dot_variant (the variant of the dot4 kernel the class's last dot4 launch
 * took: 0 .. 6 as MTM_OPT_DOT4_VARIANT numbers them, 7 = the one with uint64 totals, which the launcher takes where
 * chans w h 65025 >= 2^32; -1 = the class has not run on the dot4 kernel since it was placed).  Records of the first
 * cap_classes classes go to `out`; returns the number of classes, or a negative MTM_E_* code (no template set placed). */
#define MTM_CLASS_TILING_FIELDS 13
int         mtm_debug_class_tilings(mtm_ctx* ctx, int32_t* out, int cap_classes);
/* Test support (added under ABI 9).  The tail screen's constants (csrc/mtm_kernels.h: TemplDev::tail_k / tail_d / tail_g,
 * written on the device by tail_consts_kernel) of every template of the set placed on the context, copied back from the
 * device: MTM_TAIL_CONST_FIELDS doubles per template, in the order of the template list - k0, k1, d0, d1, g0, g1 ([0]: the
 * wave's first output row, template rows 0 .. split - 1 accumulated; [1]: its second, rows 0 .. split - 2), valid_split (the
 * split the context takes them to hold for: a launch with another one re-derives them first; 0 = none).  split == 0
 * launches nothing and reports what the device holds.  split > 0: every placed class that can screen its K loop (tail_ok)
 * first re-derives its constants for that split, clamped to [6, h - 2], on the context's stream, and the context records
 * that split as the one they hold for - what a search call with that split does ahead of its first score launch, so a later
 * search re-derives or re-uses them exactly as it would behind such a call.  Templates of classes without a screen: NaN in
 * the six constants, valid_split -1.  MTM_E_STATE: no template set is placed (run a search first); MTM_E_INVALID: a
 * mtm_find_matches_async call is in flight, split < 0; MTM_E_OVERFLOW: n_out (the doubles `out` holds) is below
 * MTM_TAIL_CONST_FIELDS times the number of templates. */
#define MTM_TAIL_CONST_FIELDS 7
int         mtm_debug_tail_consts(mtm_ctx* ctx, int split, double* out, int64_t n_out);
/* Test support (added under ABI 9; needs no image and no templates on the context).  The device's share of the non-maxima
 * suppression of mtm_find_matches_image_nms - the counting sort by grid cell, the champion pass, the prune pass - on a hit
 * list the caller hands over: the n records of `hits` and the count n go to device memory, the grid is the one a
 * rows x cols image with boxes of at most max_side a side gets (cell = max(32, max_side), cols / cell + 3 by rows / cell + 3
 * cells), and the very chain the search call queues behind its peak pass (queue_nms_chain, csrc/mtm_peaks.hip) runs on them: n_min plays the part of the
 * context's device-NMS minimum, n_max that of min(hit capacity, 2^18) - it sizes the work buffers and the launches (1 ..
 * 2^18).  score_threshold, ascending and max_overlap (>= 0) are those of mtm_nms.  out = the champions (hits no earlier hit
 * overlaps beyond max_overlap: kept for certain), then the undecided hits (neither champions nor overlapped by one), in no
 * particular order inside either part; what a champion overlaps is not returned.  mtm_nms' selection from `out` is its
 * selection from `hits`.  A list shorter than n_min or longer than n_max is left alone, as in the search call: both counts
 * 0, `out` untouched.  capacity >= n for a list inside [n_min, n_max].  The hits' boxes are expected inside the image; a
 * box elsewhere is filed in the nearest cell. */
int         mtm_debug_device_nms(mtm_ctx* ctx, const mtm_hit* hits, int64_t n, int rows, int cols, int max_side,
                                 double score_threshold, int ascending, double max_overlap, int64_t n_min, int64_t n_max,
                                 mtm_hit* out, int64_t capacity, int64_t* n_champions, int64_t* n_undecided);
/* Test support (added under ABI 9; needs no image and no templates on the context, leaves a placed template set and the
 * options as they are).  The peak pass of the search calls on score maps the caller hands over: the n_maps maps (dims: oh, ow
 * and the template's h, w per map - the last two only fill the records -, maps: their oh * ow float32 values, tightly packed,
 * map after map) go to a map arena laid out as placement lays it out (pitch = ow rounded up to 4, map after map) that was
 * filled with pattern_byte first - the pitch padding and, under `holes`, whatever the caller leaves out -, and the
 * kernels of `route` run on them through the launchers the search calls go through (csrc/mtm_peaks.hip: one launch site per
 * kernel, grids and capacities from csrc/mtm_peak_sizing.h):
 *   MTM_PEAK_SCAN            peaks_kernel
 *   MTM_PEAK_SCAN_BATCH      peaks_batch_kernel: every map is that of a stack of (oh + h - 1) / img_rows images of img_rows
 *                            rows (the same number for every map, img_rows - h >= 1)
 *   MTM_PEAK_SEGMENTS        peaks_sparse_kernel + compact_hits_kernel: flags = one byte per (map, row, strip column of 256),
 *                            n_maps x max oh x ceil(max ow / 256) bytes; holes = 1: the rows of unflagged segments are not
 *                            copied (they keep pattern_byte) and the kernel is told so
 *   MTM_PEAK_VERIFY_MAPS     verify_peaks_kernel on the candidate list cands[0 .. n_cands)
 *   MTM_PEAK_VERIFY_HASH     cand_hash_insert_kernel + verify_hash_kernel on that list
 *   MTM_PEAK_EXTREMUM        extremum_kernel
 *   MTM_PEAK_EXTREMUM_BATCH  extremum_batch_kernel (img_rows as above)
 * thr is the call's threshold on the score (a hit's quality - score, or -score with mode_min - exceeds thr, or -thr), border
 * an MTM_BORDER_* value, hit_cap the hit capacity (>= 1).  The verify routes: cand_count is the list's length as the device
 * counter holds it (it may exceed cand_cap; the first min(cand_count, cand_cap) <= n_cands records are judged, every one of
 * them inside its map), thr_q the quality a hit must exceed; their launch covers max(hit_cap, cand_cap) candidates (the
 * search call always has cand_cap <= hit_cap).
 * Results: `records` (capacity >= hit_cap records) is copied to the device's record list before the launches and back after
 * them - what the kernels did not write is what the caller put there; *count = the device's count, as it reports it;
 * raw[n_ints] = the per-map int (the scans' flag word - per (image, map), image-major, for the batch scan -, the verifiers'
 * peak count), trivial[n_ints] = the host's reading of it (scan_flags_trivial / fused_count_trivial; per image:
 * raw == 0); the extremum routes: keys[2 * n_ints] = the (max, min) key pairs, ext_hits[2 * n_ints] = their records
 * (decode_extremum_key); MTM_PEAK_SEGMENTS: list_counts[n_lists] = the per-(map, strip column) counters before compaction
 * (list = map * strip columns + strip column).  info[8] = {grid x, grid y, grid z, records per list (SEGMENTS), lists,
 * verifier work-groups, hash slots, work-groups per map of the extremum launch}.  Pointers of routes not taken may be
 * NULL; n_ints and list_cap are the lengths of raw / trivial (keys, ext_hits: twice that) and of list_counts. */
#define MTM_PEAK_SCAN           0
#define MTM_PEAK_SCAN_BATCH     1
#define MTM_PEAK_SEGMENTS       2
#define MTM_PEAK_VERIFY_MAPS    3
#define MTM_PEAK_VERIFY_HASH    4
#define MTM_PEAK_EXTREMUM       5
#define MTM_PEAK_EXTREMUM_BATCH 6
typedef struct mtm_peak_pass {
    int32_t        n_maps, route, mode_min, border;
    float          thr, thr_q;
    int32_t        img_rows, holes, pattern_byte, reserved;
    int64_t        hit_cap;
    const int32_t* dims;
    const float*   maps;
    const uint8_t* flags;
    const mtm_hit* cands;
    int64_t        n_cands, cand_count, cand_cap;
    mtm_hit*       records;
    int64_t        capacity;
    uint64_t*      count;
    int32_t*       raw;
    int32_t*       trivial;
    int64_t        n_ints;
    uint64_t*      keys;
    mtm_hit*       ext_hits;
    uint64_t*      list_counts;
    int64_t        list_cap;
    int64_t*       info;
} mtm_peak_pass;
int         mtm_debug_peak_pass(mtm_ctx* ctx, const mtm_peak_pass* args);
/* Test support (added under ABI 9; needs no templates on the context and leaves its image, template set and options as
 * they are).  The fused window statistics of single-channel uint8 images (stats_u8_kernel) on an image the caller hands
 * over, through the very function the search calls launch it with: window h x w (w <= 768, w h 255^2 < 2^32) over the
 * rows x cols pixels of `image` (tightly packed), num_type 0 / 1 / 2 (1: the window's mean is taken out - the TM_CCOEFF
 * methods), row units [sb0, sb1) of 8 output rows each (sb1 < 0 or beyond the last unit: up to the last), in form `form`
 * (output rows per work-group: 1 = 8 rows, 2 = 4 rows - MTM_STATS_FORMS of them; 0 = the launcher's choice
 * for this launch).  Everything lives in a buffer of the entry's own that is filled with pattern_byte first: the image
 * plane as the context holds it (pitch = cols + 512 rounded up to 64, zero padding), the raw copy of the image, the
 * statistics planes (pitch = ow rounded up to 4, oh rows) and the block records (4 doubles per 16 output columns and row).
 * lay_r1 > lay_r0 (cols a multiple of 4): the launch reads the raw copy instead and converts image rows [lay_r0, lay_r1)
 * into the uint8 plane and its int8 view on the way, as the banded upload has it do - both planes then start out as
 * pattern_byte.  tail_s in 1 .. h - 1 (needs blk and blkq): the tail boxes of split tail_s.  zero_header != 0: the launch
 * clears the 16-byte header, which starts out as pattern_byte too.
 * Results, each optional (NULL = not wanted, and for t0 / sum2 / sq / rsq / blk the kernel is told so): t0, sum2, sq, rsq -
 * st_pitch * oh doubles; blk, blkq - 4 * blk_pitch * oh doubles; u8, u8b - rows * pitch bytes of the two planes; header - 2
 * words; info[8] = {st_pitch, blk_pitch, plane pitch, the form that ran, grid x, grid y, the device's compute units (what the launcher's choice goes by), the
 * launch's time in nanoseconds between two events}. */
#define MTM_STATS_FORMS 2
typedef struct mtm_window_stats {
    int32_t        rows, cols, h, w, num_type, form;
    int32_t        tail_s, sb0, sb1, lay_r0, lay_r1, pattern_byte, zero_header, reserved;
    const uint8_t* image;
    double*        t0;
    double*        sum2;
    double*        sq;
    double*        rsq;
    double*        blk;
    double*        blkq;
    uint8_t*       u8;
    uint8_t*       u8b;
    uint64_t*      header;
    int64_t*       info;
} mtm_window_stats;
int         mtm_debug_window_stats(mtm_ctx* ctx, const mtm_window_stats* args);
/* Test support (added under ABI 9; as above).  The window statistics on the six OTHER kernel chains the library chooses
 * from (csrc/mtm_stats_route.h: stats_route), each through the launcher the search calls use: window h x w over the rows x
 * cols x chans pixels of `image` (interleaved, tightly packed; dtype MTM_U8 / MTM_U16 / MTM_F32), num_type 0 / 1 / 2.
 * route: 0 = the one stats_route gives this image and window (refused where that is the fused single-channel uint8 kernel:
 * mtm_debug_window_stats), else MTM_STATS_ROUTE_*, forced - refused with MTM_E_INVALID where the route's kernels are not
 * built for the image or window.  The two float64 routes take images of any dtype (they read the float32 plane).
 * want: bits 1 = the window sums t, 2 = sum2, 4 = sq, 8 = blk (MTM_STATS_ROUTE_U16 only: the records per 16 output columns),
 * 16 = hand the kernels NULL for the planes not wanted instead of a plane with its flag off.  The two-pass chains (routes
 * 3 .. 6) write sum2 whatever is asked.  sb0, sb1: row units of 8 output rows as above - MTM_STATS_ROUTE_U16, and
 * MTM_STATS_ROUTE_F64_LDS with lay_r1 > lay_r0: the launch of a band of a banded upload, row sums of image rows [lay_r0,
 * lay_r1) only, then the windows of the units (sb0 * 8 a multiple of 32, lay_r0 <= sb0 * 8, lay_r1 >= the last window's
 * last row + 1).  Everything lives in the buffer of mtm_debug_window_stats, filled with pattern_byte first; the image
 * planes are laid out by the host as an upload leaves them (pitch = cols + 512 rounded up to 64, zero padding, 0x80 in the
 * biased byte planes of a uint16 image); a call that would need more than 256 MB of it is refused.
 * Results, each optional and copied back whether wanted or not (a plane that was not wanted holds pattern_byte): t0 .. t3,
 * sum2, sq - st_pitch * oh doubles; blk - 4 * blk_pitch * oh doubles; info[12] = {the route that ran, st_pitch, blk_pitch,
 * plane pitch, the first kernel's grid x, y, z, the second kernel's grid x, y (0: a fused route), the row sums' pitch, the
 * first kernel's dynamic LDS bytes, the chain's time in nanoseconds between two events}. */
#define MTM_STATS_ROUTE_U8         0
#define MTM_STATS_ROUTE_U8MC       1
#define MTM_STATS_ROUTE_U16        2
#define MTM_STATS_ROUTE_U8_2P      3
#define MTM_STATS_ROUTE_U8_2P_WIDE 4
#define MTM_STATS_ROUTE_F64_LDS    5
#define MTM_STATS_ROUTE_F64        6
typedef struct mtm_window_stats_route {
    int32_t        rows, cols, chans, dtype, h, w, num_type, route;
    int32_t        want, sb0, sb1, lay_r0, lay_r1, pattern_byte;
    const void*    image;
    double*        t0;
    double*        t1;
    double*        t2;
    double*        t3;
    double*        sum2;
    double*        sq;
    double*        blk;
    int64_t*       info;
} mtm_window_stats_route;
int         mtm_debug_window_stats_route(mtm_ctx* ctx, const mtm_window_stats_route* args);
/* Test support (added under ABI 9; as above).  The screen of a masked float32 size class (two raw bf16 correlations, a
 * rigorous interval of every output's quality, placeholders below the threshold, exact re-scoring of the rest), stage by
 * stage through the functions a search call runs, with what each stage leaves behind.  After mtm_set_image and
 * mtm_set_templates (the method is the template set's) on a context whose templates form ONE size class the screen takes:
 * single channel, float32 image and templates with masks, w <= 256, TM_SQDIFF or TM_CCORR_NORMED, MTM_OPT_F32_MFMA 1 or 3 -
 * anything else is refused with MTM_E_INVALID.
 * pieces: 1 or 3 piece products in the raw launches; mode: MTM_PEAKS_LOCAL (listing against thr, the score threshold as a
 * search call takes it) or MTM_PEAKS_GLOBAL (against the templates' best lower bounds); rescore: run the exact re-scoring
 * of the list (not when the list overflowed: a search call repeats the screen then); list_cap: 0 = the capacity a search
 * call gives the list, else a smaller one.  set_cap != 0: nothing runs - list_cap becomes the capacity the NEXT search
 * calls of this context give the list (0: their own again).
 * n_templ, oh, ow: what the caller sized its planes by (checked).  Results, each optional, planes tightly packed
 * [n_templ][oh][ow]: c1, c2 - the float32 sums the raw launches wrote; lb, ub - the bounds of the quality (the score;
 * minima: minus the score) the listing pass computes; map_listed, map_rescored - the score maps after the listing pass and
 * after re-scoring (outputs no stage wrote hold what the buffer held); mu_i, mu_j - the launches' tile constants,
 * [nyb][nseg], `tiles` floats of room each; records (capacity >= min(capacity of the list, n_templ * oh * ow) + 8) - the
 * records written, min(count, capacity of the list) of them, then the 8 records behind the list's capacity, which were
 * filled with the byte 0xC5 before the listing pass; best - n_templ ordered-float keys (MTM_PEAKS_GLOBAL).
 * info[12] = {n_templ, h, w, oh, ow, nyb, nseg, template groups per work item, a search call's list capacity, the capacity
 * used, the count as the device counted it, 1 if the list was re-scored}. */
typedef struct mtm_maskf32_screen {
    int32_t   pieces, mode, rescore, set_cap;
    float     thr;
    int32_t   reserved;
    int64_t   list_cap;
    int64_t   n_templ, oh, ow, tiles;
    float*    c1;
    float*    c2;
    double*   lb;
    double*   ub;
    float*    map_listed;
    float*    map_rescored;
    float*    mu_i;
    float*    mu_j;
    mtm_hit*  records;
    int64_t   capacity;
    uint32_t* best;
    int64_t*  info;
} mtm_maskf32_screen;
int         mtm_debug_maskf32_screen(mtm_ctx* ctx, const mtm_maskf32_screen* args);
/* Page-locked host memory for pixel buffers (optional).  The reference's caller hands over whatever numpy holds
 * (MTM/__init__.py:247 `image`) - pageable memory, which the runtime stages through its own pinned buffers while the
 * upload call blocks.  An image kept in memory from mtm_host_alloc crosses PCIe as a plain DMA transfer behind the call
 * (MTM.pinned_empty wraps it as a numpy array).  NULL on failure (message in mtm_last_error). */
void*       mtm_host_alloc(size_t bytes);
void        mtm_host_free(void* p);

/* ---- inputs ------------------------------------------------------------------------------ */
/* Upload the search image (already cropped to searchBox by the host layer, MTM/__init__.py:140-144)
 * and build its integral images.  Replaces the per-template image handling inside
 * cv2.matchTemplate (MTM/__init__.py:92). */
int mtm_set_image(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                  int64_t row_stride_bytes);
/* Same, but the image is area-downscaled by an integer factor on the device while it is laid out
 * (the search image becomes rows/factor x cols/factor; remainder rows/columns are dropped).  Replaces
 * the host-side cv2.resize(image, smallDim, interpolation=cv2.INTER_AREA) the reference's speed-up
 * recipe runs before matching (tutorials/Tutorial3-SpeedingUp.ipynb:395).  uint8 rounding follows
 * OpenCV's integer-factor INTER_AREA path: factor 2 -> (sum + 2) >> 2, else
 * rint((float)sum * (1.f / factor^2)). */
int mtm_set_image_downscaled(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                             int64_t row_stride_bytes, int factor);

/* Upload all templates of one matchTemplates/findMatches call and fix the method.  Template
 * statistics (cv::meanStdDev) are computed here.  Replaces the per-template arguments of
 * cv2.matchTemplate (MTM/__init__.py:92). */
int mtm_set_templates(mtm_ctx* ctx, const mtm_templ* templs, int n_templ, int method);

/* The caller's step BEFORE the hot path, on the device: the reference's users append rotated / flipped / rescaled
 * copies of their templates to listTemplates on the host (tutorials/Tutorial2-Template_Augmentation.ipynb:313,
 * np.rot90; multi-scale copies).  Here the caller hands over the BASES and a list of variants; every
 * (base, variant) pair becomes one unit, base-major (unit index = base * n_variants + variant), exactly as if
 * the copies had been passed to mtm_set_templates.  A unit is a view of a source kept on the device - the base,
 * or an area-resized copy a kernel makes of it - read through the variant's reflection / rotation, and the
 * operand packs of the score kernel are gathered from those views: no per-unit pixel work on the host, no
 * per-unit upload.  uint8 bases (1-4 channels), uint8 masks (transformed like their template).
 * Order of the steps of a variant: resize, np.fliplr, np.flipud, np.rot90(k). */
typedef struct mtm_variant {
    int32_t rot90;     /* 0..3 quarter turns counter-clockwise (np.rot90(a, k))                                   */
    int32_t flip_lr;   /* 1: np.fliplr                                                                          */
    int32_t flip_ud;   /* 1: np.flipud                                                                          */
    int32_t rows, cols;/* > 0: area-resize the base to rows x cols first (exact rational area average, rounded
                          half up: MTM.augment.resize_area); 0, 0 = keep the size                               */
    int32_t down;      /* > 1: integer-factor area downscale first, OpenCV INTER_AREA rounding
                          (MTM.augment.downscale); exclusive with rows / cols                                   */
} mtm_variant;
int mtm_set_templates_augmented(mtm_ctx* ctx, const mtm_templ* bases, int n_bases,
                                const mtm_variant* variants, int n_variants, int method);

/* ---- the hot path -------------------------------------------------------------------------- */
/* cv2.matchTemplate(image, template, method, mask) for template `templ_idx`
 * (MTM/__init__.py:92, via computeScoreMap :56-92): float32 (rows-h+1, cols-w+1) to host memory. */
int mtm_score_map(mtm_ctx* ctx, int templ_idx, float* out, int64_t out_row_stride_bytes);

/* The per-template pipeline of _multi_compute (MTM/__init__.py:222-241) for every template set by
 * mtm_set_templates, batched: score maps, then either local extrema above/below `score_threshold`
 * (skimage peak_local_max / scipy find_peaks semantics, :22-53) or the global extremum
 * (cv2.minMaxLoc, :226).  Hits come back ordered by template index, then descending quality, then
 * row-major position; coordinates are relative to the uploaded image.  The threshold is the
 * python float of the reference call; it is narrowed to float32 for the comparison with the
 * float32 map exactly as numpy does.  On MTM_E_OVERFLOW *n_out is the capacity needed. */
int mtm_find_matches(mtm_ctx* ctx, int mode, double score_threshold,
                     mtm_hit* out, int64_t capacity, int64_t* n_out);

/* One call for "this image, these templates": mtm_set_image + mtm_find_matches without the round trip to the
 * host in between - what one MTM.matchTemplates / findMatches call does with the image it is given
 * (MTM/__init__.py:95-177; the templates come from mtm_set_templates).  The image becomes the context's
 * current image.  Where the layout allows (one unmasked single-channel uint8 size class on the matrix-core
 * kernel) the image crosses PCIe in row bands, and the score kernel of the rows already there runs under the
 * transfer of the next band: the upload costs little more than its first band.  Results are those of the two
 * separate calls. */
int mtm_find_matches_image(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, int mode, double score_threshold,
                           mtm_hit* out, int64_t capacity, int64_t* n_out);

/* mtm_find_matches_image (local extrema) followed by MTM's non-maxima suppression - what MTM.matchTemplates does with
 * the hits of all templates (MTM/__init__.py:290-296 -> MTM/NMS.py:53-84 -> cv2.dnn.NMSBoxes): hits whose score passes
 * `score_threshold` (1 - score for TM_SQDIFF_NORMED, as NMS.py:73-75 transforms it), best first, each kept unless it
 * overlaps an already kept one by more than `max_overlap` (intersection over union, OpenCV's float expression); at most
 * `n_object` of them (n_object < 0: all - a sentinel, NOT Python's indexes[:n_object]: MTM.matchTemplates sends a finite
 * negative N_object the two-step way, mtm_find_matches_image + mtm_nms + the slice).  Returns the kept hits in that
 * order - the list mtm_nms would select from the list mtm_find_matches_image returns.  Of thousands of peaks (dense images) the ones a neighbourhood's best peak suppresses
 * are dropped on the device and never cross PCIe; mtm_timing.n_hits is the number of peaks before the suppression. */
int mtm_find_matches_image_nms(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                               int64_t row_stride_bytes, double score_threshold, double max_overlap, int64_t n_object,
                               mtm_hit* out, int64_t capacity, int64_t* n_out);

/* One step of the process-per-GPU form in one native call (round 5): search this rank's shard of the caller's template
 * list (the context's current templates; global_idx[i] = list position of local template i), exchange the ranks' hit
 * lists through the context's communicator (mtm_comm_init; without one, or with one rank: no exchange), merge them in
 * template order and run MTM's non-maxima suppression - every rank returns the same kept hits, best first.  The
 * reference's fan-in of per-template results (MTM/__init__.py:173-177) + MTM/NMS.py:53-84 across processes.  A rank
 * without units passes n_local_templ = 0 (px may be NULL) and still takes part in the collective. */
int mtm_find_matches_image_sharded_nms(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                                       int64_t row_stride_bytes, double score_threshold, double max_overlap,
                                       int64_t n_object, int method, const int32_t* global_idx, int n_local_templ,
                                       mtm_hit* out, int64_t capacity, int64_t* n_out);

/* A batch of images of ONE shape against the templates of the last mtm_set_templates ("thousands of images", reference
 * tutorials/Tutorial3-SpeedingUp.ipynb: well plates, time-lapse stacks): what n_images calls of mtm_find_matches_image
 * return, in one chain of launches instead of one per image.  images[b] points at image b's first row; every image has
 * rows x cols x chans pixels of `dtype` and the row stride `row_stride_bytes` (a cropped view of a larger image needs no
 * host copy).  uint8 and uint16 only: MTM_F32 returns MTM_E_INVALID (the float32 screen and re-scoring routes work on
 * neighbourhoods of one image); so does a template taller or wider than the images.
 * The images are uploaded as ONE image of n_images * rows rows, and the statistics and score launches run over the whole
 * stack.  Map rows whose windows straddle two images are computed and ignored: the peak pass treats the rows outside
 * image b's own map rows as outside the map (the border rule of MTM_OPT_PEAK_BORDER), the global extremum is taken per
 * (image, template) in the image's own row-major order, and 1-D / 1x1 per-image maps take the host's find_peaks_1d path.
 * The maps are always materialised (no kernel candidate list, no fused extremum).  Batches taller than
 * MTM_OPT_BATCH_MAX_ROWS, or than a device-memory budget for the maps, run in chunks of whole images; results do not depend
 * on the chunking.
 * Output: the hits of image 0, then image 1, ... - each image's records exactly those (and in the order) mtm_find_matches_image
 * returns for it alone, coordinates in the image's own frame; counts[b] = records of image b.  counts is filled on
 * MTM_E_OVERFLOW too: *n_out is then the capacity needed and mtm_last_hits returns the records.  Afterwards the context has
 * no current image (mtm_find_matches, mtm_last_score_map: MTM_E_STATE until the next mtm_set_image). */
int mtm_find_matches_batch(mtm_ctx* ctx, const void* const* images, int n_images, int rows, int cols, int chans,
                           int dtype, int64_t row_stride_bytes, int mode, double score_threshold,
                           mtm_hit* out, int64_t capacity, int64_t* counts, int64_t* n_out);

/* Coarse-to-fine search (reference tutorials/Tutorial3-SpeedingUp.ipynb: the searchBox and downscaling recipes combined;
 * DESIGN 5.2).  The image (uint8, `rows` x `cols` before any downscale) crosses PCIe once; the coarse image - its
 * integer-factor area downscale, as mtm_set_image_downscaled makes it - is derived on the device from the same upload.
 * Templates: those of the last mtm_set_templates (unmasked uint8, method 1..5), downscaled by `factor` on the host with the
 * same arithmetic for the coarse level.
 *   coarse level: the local extrema of every template's coarse map that pass `coarse_threshold` (mtm_find_matches'
 *                 rule, border option and "no non-maximum pixel, no peaks" rule); the best `max_candidates` per template.
 *   windows:      a candidate at coarse output (cy, cx) stands for the full-resolution positions rows
 *                 [cy f - radius, cy f + radius] x columns [cx f - radius, cx f + radius], clipped to the score map.
 *   fine level:   mode MTM_PEAKS_LOCAL - the positions of the windows' union that are local extrema of the full-resolution
 *                 map under mtm_find_matches' rule (neighbours outside the windows count; the map's own border rule) and
 *                 pass `score_threshold`; a template whose windows hold no position that differs from its neighbourhood's
 *                 extremum has none.  MTM_PEAKS_GLOBAL - per template with candidates, the extremum over the union (ties:
 *                 first in row-major order).  Scores are bit for bit those of mtm_score_map.
 * Hits in mtm_find_matches' order, coordinates relative to the image.  Every coarse and full-resolution score map must be
 * at least 2 x 2 and every coarse template at least 2 x 2 (MTM_E_INVALID otherwise).  On MTM_E_OVERFLOW *n_out holds the
 * capacity needed and mtm_last_hits returns the records.  The image becomes the context's current image; the templates
 * stay as they were set. */
int mtm_find_matches_pyramid(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                             int64_t row_stride_bytes, int factor, int mode, double coarse_threshold,
                             double score_threshold, int radius, int max_candidates, mtm_hit* out, int64_t capacity,
                             int64_t* n_out);

/* Many searchBoxes of one image in one call: what n_units calls of mtm_find_matches on the crops return -
 * unit u's template (units[u].templ_idx, of the last mtm_set_templates) searched in the region of unit u as if the crop
 * were the whole image: its own score map of (rows - h + 1) x (cols - w + 1) outputs, whose edges are the map border of
 * MTM_OPT_PEAK_BORDER's rule, mtm_find_matches' "no non-maximum pixel, no peaks" rule and 1-D / 1x1 rules per unit,
 * mode MTM_PEAKS_GLOBAL the unit's extremum (ties: first in row-major order).  Scores are bit for bit those of
 * mtm_score_map on the crop.  The image (uint8 with 1 or 3 channels, or single-channel uint16, the templates' pixel type;
 * unmasked templates, method 0..5) crosses PCIe once.  Hits come grouped by unit in unit order, each group in
 * mtm_find_matches' order; counts[u] = the number of records of unit u; coordinates are in the full image.  A template
 * larger than its unit's region, or a region outside the image, returns MTM_E_INVALID.  Units whose maps together exceed
 * MTM_OPT_BOXES_MAX_FLOATS run in chunks of whole units.  On MTM_E_OVERFLOW *n_out holds the capacity needed, counts are
 * written and mtm_last_hits returns the records.  The image becomes the context's current image. */
int mtm_find_matches_boxes(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, const mtm_box_unit* units, int n_units, int mode,
                           double score_threshold, mtm_hit* out, int64_t capacity, int64_t* counts, int64_t* n_out);

/* Templates tracked through a stack of frames in one call: what a loop of mtm_find_matches_boxes calls in
 * mode MTM_PEAKS_GLOBAL returns, one per frame, each frame's boxes computed from the previous frame's hits.  Track k
 * follows template start[k].templ_idx (of the last mtm_set_templates) from the region of start[k] in frame 0 (clipped to
 * the frame, as mtm_find_matches_boxes takes it).  For frame f, track k's record is the extremum of its template's score
 * map over its current region (ties: first in row-major order; scores bit for bit those of mtm_score_map on the crop),
 * in frame coordinates.  The region of frame f + 1 is that hit widened by `margin` pixels on every side and clipped to
 * the frame - x0 = max(0, x - margin), y0 = max(0, y - margin), x1 = min(cols, x + w + margin),
 * y1 = min(rows, y + h + margin) - unless use_min is set and the score does not pass min_score (methods 0 and 1: score <
 * min_score, the others: score > min_score, compared in double; a NaN score never passes), in which case the region is
 * kept.  Frames: n_frames arrays of one shape, pixel type and row stride (uint8 with 1 or 3 channels, or single-channel
 * uint16, the templates' pixel type; unmasked templates, method 0..5).  They go up in chunks of frames bounded by
 * MTM_OPT_BATCH_MAX_ROWS and a device-memory budget for their planes; the regions stay on the device between frames and
 * chunks, and the host waits once, for the records.  out: n_frames * n_tracks records, frame-major (out[f * n_tracks +
 * k]); templ_idx = the track's template.  A template larger than its frame-0 region, or a region outside the frame,
 * returns MTM_E_INVALID.  Afterwards the context has no current image (as after mtm_find_matches_batch). */
int mtm_track_boxes(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                    int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                    double min_score, mtm_hit* out);

/* mtm_track_boxes with the 3 x 3 score neighbourhood of every record: the same arguments, checks, errors,
 * records and afterwards-state, and nbhd[9 (f * n_tracks + k) + 3 (1 + dy) + (1 + dx)] = the score of track k's template
 * at window (x + dx, y + dy) of frame f's own score map, (x, y) being the record out[f * n_tracks + k], NaN for a window
 * outside that map - what mtm_hit_neighbourhoods returns for that record on frame f, bit for bit.  The neighbourhoods are
 * scored while the frame is on the device: no frame crosses PCIe twice and the host still waits once.  They do not steer
 * the tracks: the regions follow the records.  nbhd: 9 * n_frames * n_tracks floats, required when both counts are
 * positive. */
int mtm_track_boxes_nbhd(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                         int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                         double min_score, mtm_hit* out, float* nbhd);

/* mtm_track_boxes / mtm_track_boxes_nbhd with adaptive templates: the same arguments, checks, errors, records
 * and afterwards-state, but every track owns a copy of its template - made on the device at the start of the call, in
 * buffers of the call: the template set of the context is left as it is - and after each frame whose hit passes (use_min
 * not set, or the score passes min_score: the rule that moves the region) every pixel of that copy becomes
 *   (T * (256 - blend_a) + W * blend_a + 128) >> 8
 * in integers, W being the frame's pixel under the hit; blend_a in 1 .. 256 (256: the window replaces the template).  The
 * copy's constants are recomputed on the device from exact integer sums, in mtm_set_templates' operation order, so frame
 * f + 1 is searched exactly as a mtm_find_matches_boxes call after mtm_set_templates of the blended template would search
 * it.  Two tracks of one template diverge.  The adoption also follows the last frame.  One more launch per frame; the host
 * still waits once.  nbhd: optional (NULL: records only); frame f's neighbourhoods are those of the template frame f was
 * searched with.  templ_out: optional; every track's template after the last frame, track after track, each as
 * mtm_set_templates takes it (interleaved channels, tightly packed, the frames' pixel type).  stats_out: optional; 7
 * doubles per track, the constants of that template as mtm_debug_templ_stats lists them.  out[..].templ_idx = the track's
 * template in the set, as mtm_track_boxes returns it. */
int mtm_track_boxes_adapt(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                          int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin, int use_min,
                          double min_score, mtm_hit* out, float* nbhd, int blend_a, void* templ_out, double* stats_out);

/* mtm_track_boxes with lost tracks re-acquired by a whole-frame search: mtm_track_boxes_adapt's arguments,
 * with blend_a = 0 meaning no adaptation (templ_out and stats_out are then ignored; otherwise blend_a in 1 .. 256) and
 * nbhd == NULL meaning no neighbourhoods; the same checks, errors and afterwards-state.  use_min must be set
 * (MTM_E_INVALID otherwise).  In every frame, a track whose hit in its region does not pass min_score (the rule that
 * keeps the region) is searched again in the same frame over the whole frame - region (0, 0, cols, rows), which always
 * holds the template - with the template the region was searched with: its record of that frame becomes the extremum of
 * the template's whole-frame score map (ties: first in row-major order of that map; the same score bits as the region's
 * map, which it contains).  If that record passes, the next frame's region is around it (and, with blend_a, the track
 * adopts its window); if not, the region is kept and the next frame tries again.  The neighbourhoods are those of the
 * final records.  The second search runs on the device for exactly the tracks that failed, after the frame's first
 * search: the host does not learn which they are and still waits once, for the records.  Two more launches per frame,
 * one of which leaves at once in a frame that lost no track.  A track whose whole-frame map has 2^32 outputs or more
 * returns MTM_E_INVALID (the extremum's key carries a 32-bit index). */
int mtm_track_boxes_reacquire(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans,
                              int dtype, int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, int margin,
                              int use_min, double min_score, mtm_hit* out, float* nbhd, int blend_a, void* templ_out,
                              double* stats_out);

/* mtm_track_boxes for tracks that carry a set of templates: track k follows the templates
 * set_idx[set_off[k] .. set_off[k + 1] - 1] of the current set, all of one (rows, cols); set_off has n_tracks + 1
 * ascending entries, set_off[0] = 0.  start[k] is the frame-0 region, and start[k].templ_idx must equal
 * set_idx[set_off[k]].  In every frame every template of the set is searched in the track's region; the frame's record
 * is that of the template with the best extremum - the first in set order on ties, compared as float32 scores (a NaN
 * never replaces an earlier one) - and out[f * n_tracks + k].templ_idx names it.  The next frame's region is derived from
 * that record by mtm_track_boxes' rule.  reacquire != 0 (needs use_min): a record that does not pass min_score is followed
 * by a whole-frame search of every template of the set, reduced the same way, as mtm_track_boxes_reacquire does for one
 * template.  nbhd: optional (NULL: records only), the 3 x 3 neighbourhoods of the final records in the map of the
 * winning template, as mtm_track_boxes_nbhd returns them.  Checks as mtm_track_boxes', per template; an empty set, a set
 * of templates that differ in shape and reacquire without use_min return MTM_E_INVALID.  One host wait per call. */
int mtm_track_boxes_sets(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                         int64_t row_stride_bytes, const mtm_box_unit* start, int n_tracks, const int32_t* set_off,
                         const int32_t* set_idx, int margin, int use_min, double min_score, int reacquire, mtm_hit* out,
                         float* nbhd);

/* One block of mtm_match_blocks: columns x .. x + w - 1 and rows y .. y + h - 1 of the reference image. */
typedef struct mtm_block {
    int32_t x, y, w, h;
} mtm_block;

/* Block matching between two images of one shape in one call: block k of `reference` is the template, and
 * its search box in `image` is the block's own box widened by `margin` pixels on every side and clipped to the image.
 * out[k] = the extremum of that template's score map over the box - what mtm_find_matches_boxes returns in
 * MTM_PEAKS_GLOBAL mode for the block's pixels set as a template and the box as its region: image coordinates, the same
 * float32 score bits, the first output in row-major order of the box's map on ties - with templ_idx = k.  The templates
 * never exist on the host: a kernel cuts them out of the uploaded reference and computes their constants on the device.
 * uint8 images with 1 or 3 channels or single-channel uint16 ones, each with a row stride of its own; method: MTM_TM_*.
 * nbhd: optional (NULL: records only), 9 n floats - nbhd[9 k + 3 (1 + dy) + (1 + dx)] = the score of block k at window
 * (x + dx, y + dy) of the WHOLE image's map around out[k], NaN outside that map: what mtm_hit_neighbourhoods returns for
 * it, bit for bit.  A block outside the reference or with w < 1 or h < 1, a uint16 block of more than 2^21 pixels and a
 * block of 2^31 pixels or more return MTM_E_INVALID and name the block.  The templates set on the context, their caches
 * and the method they were set with are neither read nor changed; the context has no current image afterwards.  Blocks run
 * in chunks whose template bytes fit 4 * MTM_OPT_BOXES_MAX_FLOATS; one host wait per call. */
int mtm_match_blocks(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                     int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                     int n_blocks, int margin, int method, mtm_hit* out, float* nbhd);

/* Test support: the host plan of a mtm_match_blocks call (no context, no GPU) - its checks, tile table and chunk split
 * for a template budget of `budget_bytes`.  tiles: 3 int32 per tile (block, first output row, first output column of a
 * 16 x 16 tile of the block's map), at most tile_cap tiles are written and *n_tiles is their full number; chunk_of[k] =
 * the chunk block k runs in; toff[k] = the byte offset of its template planes in that chunk's buffer; maps: 4 int32 per
 * block (x0, y0 of its search box, ow, oh of its map).  Any output may be NULL. */
int mtm_debug_plan_blocks(int rows, int cols, int chans, int dtype, const mtm_block* blocks, int n_blocks, int margin,
                          int64_t budget_bytes, int32_t* tiles, int64_t tile_cap, int64_t* n_tiles, int32_t* chunk_of,
                          int64_t* toff, int32_t* maps);

/* mtm_match_blocks_stack: the reference of pair p. */
#define MTM_BLOCKS_REF_PREVIOUS 0 /* frames[p] */
#define MTM_BLOCKS_REF_FIRST 1    /* frames[0] */

/* Block matching over a stack of n_frames frames of one shape in one call: pair p (0 .. n_frames - 2)
 * searches frames[p + 1] for the blocks of its reference - frames[p] (MTM_BLOCKS_REF_PREVIOUS) or frames[0]
 * (MTM_BLOCKS_REF_FIRST) - exactly as mtm_match_blocks(reference, frames[p + 1], ...) does.  Frames as mtm_track_boxes
 * takes them: n_frames pointers, one row stride.
 * Per-pair results (planes == NULL): out_hits[p n_blocks + k] = mtm_match_blocks' out[k] of pair p, bit for bit; nbhd:
 * optional, 9 floats per record in the same order, mtm_match_blocks' nbhd of the pair.
 * Ensemble planes (planes != NULL; out_hits and nbhd are ignored): S = 2 margin + 1, planes[(k S + margin + dy) S +
 * margin + dx] = the mean over the pairs of block k's score at displacement (dx, dy): the float32 rounding of
 * (((s_0 + s_1) + ...) + s_{P-1}) / P in float64, s_p the pair's float32 score; NaN where the clipped search box has no
 * output at that displacement.  n_blocks S^2 above MTM_OPT_BOXES_MAX_FLOATS returns MTM_E_INVALID and names both numbers.
 * Frames go up in stacks of at most MTM_OPT_BATCH_MAX_ROWS rows (never fewer than two frames: frames of at most 32767
 * rows), each frame once plus the frame that carries the reference into a stack; no kernel reads across frames.  Checks,
 * block chunks and the context's state afterwards as mtm_match_blocks'; n_frames < 2 with n_blocks > 0 returns
 * MTM_E_INVALID.  One host wait per call. */
int mtm_match_blocks_stack(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, const mtm_block* blocks, int n_blocks, int margin, int method, int mode,
                           mtm_hit* out_hits, float* nbhd, float* planes);

/* Test support: the host plan of a mtm_match_blocks_stack call (no context, no GPU).  chunks: 4 int32 per frame chunk -
 * (f0, nf, carried, p0): the chunk uploads the stack [frame carried, frames f0 .. f0 + nf - 1] and runs the pairs p0 ..
 * p0 + nf - 1 -, at most chunk_cap chunks are written and *n_chunks is their full number.  With blocks and clip != NULL:
 * clip[2 k], clip[2 k + 1] = (ox, oy) of block k, how far its search box was clipped at the left and at the top (output
 * (y, x) of its map is cell (y + oy, x + ox) of its plane); rows .. dtype describe the frames as for
 * mtm_debug_plan_blocks. */
int mtm_debug_plan_blocks_stack(int n_frames, int frames_per_chunk, int mode, int32_t* chunks, int64_t chunk_cap,
                                int64_t* n_chunks, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                                int n_blocks, int margin, int32_t* clip);

/* mtm_match_blocks_stack with a predicted displacement per block, shared by every pair: block k is searched
 * in the box mtm_match_blocks_at gives it for offsets[2 k], offsets[2 k + 1].  Frames, mode, checks and the context's state
 * afterwards as mtm_match_blocks_stack's; the boxes and the fixed tile table as mtm_match_blocks_at's.
 * Per-pair results (planes == NULL): out_hits[p n_blocks + k] = mtm_match_blocks_at's out[k] of pair p, bit for bit; nbhd
 * likewise.
 * Ensemble planes (planes != NULL; nbhd is ignored): with (cx, cy) the block's moved and clamped position, planes[(k S +
 * margin + dy) S + margin + dx] = the mean over the pairs of block k's score at position (cx + dx, cy + dy), in
 * mtm_match_blocks_stack's arithmetic, NaN where the clipped box has no such output.  The means and the NaN fill are
 * computed on the device (blocks_plane_peak_kernel) and the planes come back as float32; out_hits, if not NULL, gets one
 * record per block: the plane's peak - the largest mean that is not NaN, the smallest for TM_SQDIFF(_NORMED), -0 equal to
 * +0, the first cell in row-major order on ties - at (cx + dx, cy + dy) with the plane's own float32. */
int mtm_match_blocks_stack_at(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                              int64_t row_stride_bytes, const mtm_block* blocks, const int32_t* offsets, int n_blocks,
                              int margin, int method, int mode, mtm_hit* out_hits, float* nbhd, float* planes);

/* mtm_match_blocks with a predicted displacement per block: offsets[2 k], offsets[2 k + 1] = (dx, dy) of
 * block k.  The block's position is moved by its offset and clamped so that the block still lies inside the image - cx =
 * min(max(x + dx, 0), cols - w), cy likewise -, and the search box is the box of the moved block widened by `margin` and
 * clipped to the image (MTM.blocks.search_box_at); the template is still the block at (x, y) of the reference.  out, nbhd,
 * checks, chunks and the context's state afterwards as mtm_match_blocks'; zero offsets give its records bit for bit.  Any
 * int32 offset is valid.  The boxes are computed on the device from the uploaded offsets, and every block's map is scored
 * over a fixed grid of ceil((2 margin + 1) / 16)^2 tiles (per axis at most the tiles of the block's map over the whole
 * image); the tiles of all blocks must stay below 2^31. */
int mtm_match_blocks_at(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                        int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                        const int32_t* offsets, int n_blocks, int margin, int method, mtm_hit* out, float* nbhd);

/* One pass of mtm_match_blocks_passes: every bw x bh block at stride (sx, sy) that lies wholly inside the image, in
 * row-major order (MTM.blocks.grid), searched with `margin`. */
typedef struct mtm_block_pass {
    int32_t bw, bh, sx, sy, margin;
} mtm_block_pass;

/* Coarse-to-fine block matching in one call.  Pass 0 is mtm_match_blocks over its grid.  Every later pass
 * p is mtm_match_blocks_at over its own grid with, for each block, the displacement (record position - block position) of
 * the block of pass p - 1 whose centre is nearest: per axis, on doubled centres, index min(n - 1, max(0, 2 x + wf - wc +
 * s) / (2 s)) of a coarse axis of n blocks of size wc at stride s for a fine block of size wf at x (an exact tie goes to
 * the higher index).  Records are pass-major: out holds those of pass 0's blocks, then pass 1's, ...; nbhd (optional) 9
 * floats per record in the same order.  Both images are uploaded once and the host waits once: the boxes of the later
 * passes are computed on the device from the previous pass's records and never reach the host.  A pass with bw, bh, sx or
 * sy < 1 or margin < 0, or whose grid is empty, returns MTM_E_INVALID and names the pass; other checks, the template-byte
 * chunks within a pass and the context's state afterwards as mtm_match_blocks'. */
int mtm_match_blocks_passes(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                            const mtm_block_pass* passes, int n_passes, int method, mtm_hit* out, float* nbhd);

/* Test support: the host plan of a mtm_match_blocks_passes call (no context, no GPU).  counts[p] = the blocks of pass p;
 * tiles: 4 int32 per tile of the fixed tile table - (pass, block within the pass, first output row, first output column) -
 * pass after pass, at most tile_cap tiles are written and *n_tiles is their full number; chunk_of: one int32 per block,
 * pass-major, the chunk of its pass the block runs in (budget_bytes as mtm_debug_plan_blocks').  With coarse != NULL and 1
 * <= at_pass < n_passes: coarse holds one record per block of pass at_pass - 1, and for every block k of pass at_pass
 * pred[2 k], pred[2 k + 1] = the predicted (dx, dy) and maps[4 k ..] = (x0, y0, ow, oh) of the unit the device would
 * search - the very functions the kernel runs.  Any output may be NULL. */
int mtm_debug_plan_blocks_passes(int rows, int cols, int chans, int dtype, const mtm_block_pass* passes, int n_passes,
                                 int64_t budget_bytes, int64_t* counts, int32_t* tiles, int64_t tile_cap, int64_t* n_tiles,
                                 int32_t* chunk_of, const mtm_hit* coarse, int at_pass, int32_t* pred, int32_t* maps);

/* mtm_match_blocks_passes with outlier validation between the passes: after every pass its records go
 * through the normalised median test (Westerweel & Scarano), and the next pass is steered by the validated records instead
 * of the raw ones.  The grid of a pass is nx x ny blocks in row-major order, d = (dx, dy) = record position - block
 * position.  The neighbours of a block are the blocks of its 3 x 3 grid neighbourhood that exist, without the block itself;
 * a block with fewer than 3 neighbours is valid.  Per component u (dx, then dy) over the n >= 3 neighbour values, with
 * dmed(s) = s[(n - 1) / 2] + s[n / 2] of the sorted values (the doubled median, int64): m2 = dmed(u_i), r_i = |2 u_i - m2|,
 * rm4 = dmed(r_i), and the block is an outlier in the component iff (double)(2 |2 u_0 - m2|) > threshold * ((double)rm4 +
 * 4.0 * epsilon) - one rounded float64 addition, one rounded float64 multiplication, no fused operation.  A block is invalid if
 * either component is an outlier; the displacement that steers the next pass is then ((m2x + 1) >> 1, (m2y + 1) >> 1), the
 * neighbours' median rounded half towards +infinity.  Only raw records are read - neighbours that are outliers themselves
 * count as they are, nothing is iterated -, so the result depends on no order of evaluation.  out and nbhd are the RAW
 * records and their neighbourhoods, exactly mtm_match_blocks_passes' layout; valid (required): one byte per record in
 * the same pass-major order, 1 = valid, 0 = outlier; the last pass is validated too.  threshold and epsilon must be
 * finite and >= 0 (MTM_E_INVALID names the argument).  One small launch per pass more than mtm_match_blocks_passes; the
 * flags come back behind the call's single wait.  Everything else as mtm_match_blocks_passes. */
int mtm_match_blocks_passes_validated(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                                      int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                      const mtm_block_pass* passes, int n_passes, int method, double threshold,
                                      double epsilon, mtm_hit* out, float* nbhd, uint8_t* valid);

/* Test support: the median test of mtm_match_blocks_passes_validated over one grid of records.  recs: nx * ny records in
 * row-major order, block (iy, ix) at (ix sx, iy sy).  valid[k] = 1 / 0 as above; steer[k] = recs[k], or for an outlier
 * recs[k] with x, y = block position + replacement displacement.  ctx == NULL runs the rule on the host (no GPU); with a
 * context the records are uploaded, the validation kernel is launched once and its output comes back.  nx, ny, sx, sy >=
 * 1, nx * ny < 2^31; threshold and epsilon as above. */
int mtm_debug_validate_blocks(mtm_ctx* ctx, const mtm_hit* recs, int nx, int ny, int sx, int sy, double threshold,
                              double epsilon, uint8_t* valid, mtm_hit* steer);

/* mtm_match_blocks_at with every block's SECOND correlation peak: the best output of the block's map outside
 * an exclusion window around the first peak - what a PIV package divides the first peak by for a vector's signal-to-noise.
 * The map is the oh x ow one the record in `out` is the extremum of; its cells are ordered as the 64-bit quality key orders
 * them, quality q = score, or -score for methods 0 and 1: larger q first, -0 equal to +0, ties to the smaller row-major
 * index.  With (py, px) the first peak's cell, the second peak is the first cell in that order among those with
 * max(|y - py|, |x - px|) > exclusion.  second[k]: templ_idx, w, h as out[k], x, y the cell in image coordinates and score
 * its float32 score, (mode_min ? -q : q) + 0.0f; a map with no cell outside the exclusion (a 1 x 1 map; any map that reaches
 * at most `exclusion` cells beyond the peak) gives x = y = -1 and a NaN score - the maps of these calls hold no NaN, so NaN
 * means "none" and nothing else.  offsets may be NULL (no displacement: mtm_match_blocks' boxes); out and nbhd are
 * mtm_match_blocks_at's, bit for bit.  The scores stay on the device: the score launch also stores them, one launch
 * sub-range of whole blocks within MTM_OPT_BOXES_MAX_FLOATS floats at a time (never fewer than one block), and a small
 * kernel per sub-range reduces them; still one wait.  exclusion < 0 or second == NULL: MTM_E_INVALID, "bad arguments". */
int mtm_match_blocks_second(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                            const int32_t* offsets, int n_blocks, int margin, int method, mtm_hit* out, float* nbhd,
                            int exclusion, mtm_hit* second);

/* mtm_match_blocks_at / mtm_match_blocks_second with a static MASK over the reference.  mask: rows x cols
 * bytes at mask_stride_bytes per row, non-zero = the pixel takes part, for every channel.  Block k's template is its pixels
 * of the reference with the mask's pixels under it - what mtm_find_matches_boxes returns in MTM_PEAKS_GLOBAL mode for the
 * block set as a masked template.  With M the block's binary mask and the integers summed over all channels - tms = sum (T
 * M)^2, per output c1 = sum I T M and c2 = sum (I M)^2 -, TM_CCORR_NORMED scores (float)(c1 / sqrt(tms c2)) in float64 with
 * IEEE square root and division, TM_SQDIFF (float)(-2 c1 + c2 + tms): the exhaustive masked map's bits.  An output whose
 * score is NaN (c2 == 0 or tms == 0 under TM_CCORR_NORMED) is never a peak; a block whose mask keeps no pixel is not
 * searched; such a block, and a block all of whose outputs are NaN, gets x = y = -1 and a NaN score in out (nine NaNs in
 * nbhd, x = y = -1 and NaN in second).  offsets may be NULL (mtm_match_blocks' boxes); exclusion < 0: no second peak
 * (second is not read), else second is required and NaN cells are never chosen.  The mask goes up once, into a buffer of its
 * own; a block takes 2 w h chans template bytes of the chunk budget.  MTM_E_INVALID names the argument for a NULL mask, a
 * dtype other than MTM_U8 and a method other than TM_SQDIFF / TM_CCORR_NORMED; everything else as mtm_match_blocks_at. */
int mtm_match_blocks_masked(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, const void* mask, int64_t mask_stride_bytes, int rows, int cols,
                            int chans, int dtype, const mtm_block* blocks, int n_blocks, const int32_t* offsets, int margin,
                            int method, int exclusion, mtm_hit* out, float* nbhd, mtm_hit* second);

/* mtm_match_blocks_passes_validated with the second peak of every record, pass-major as out (second: required).  valid may
 * be NULL: no validation, mtm_match_blocks_passes' chain (threshold and epsilon are then not read).  The second peaks steer
 * nothing: out, nbhd and valid are those of the call without them, bit for bit. */
int mtm_match_blocks_passes_second(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                                   int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                   const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                   mtm_hit* out, float* nbhd, uint8_t* valid, int exclusion, mtm_hit* second);

/* Test support: the second peaks of n constructed maps.  planes: the maps back to back, map k of oh[k] x ow[k] float32
 * cells, row-major; a NaN cell takes no part.  firsts: the row-major index of each map's first peak, or NULL - the map's
 * best cell by the rule above.  out[k]: templ_idx = k, x, y the second peak's cell in the map's own coordinates (origin 0,
 * 0), w = h = 0, score as above; (-1, -1) and NaN where there is none (a map of NaNs included).  ctx == NULL runs the
 * rule on the host (no GPU); with a context the maps are uploaded and the second-peak kernel is launched once over all of
 * them.  n >= 1, oh, ow >= 1, oh * ow < 2^32, mode_min 0 or 1, exclusion >= 0. */
int mtm_debug_second_peaks(mtm_ctx* ctx, const float* planes, int n, const int32_t* oh, const int32_t* ow,
                           const int32_t* firsts, int mode_min, int exclusion, mtm_hit* out);

/* mtm_match_blocks_passes over the pairs of a frame stack in one call.  passes as mtm_match_blocks_passes
 * takes them, frames and mode as mtm_match_blocks_stack; n_frames >= 2.  With n = the blocks of all passes:
 * Per-pair results (planes == NULL): out_hits[p n + j] = mtm_match_blocks_passes' out[j] for pair p, bit for bit, nbhd
 * likewise - every pair runs its own chain of passes on the device, all passes of the pairs of a frame chunk ahead of the
 * next upload, every frame uploaded once (plus a chunk's carried frame).
 * Ensemble (planes != NULL; nbhd is ignored): pass 0 sums mtm_match_blocks_stack's planes over its grid; their peaks (as
 * mtm_match_blocks_stack_at records them) steer pass 1 as a pass's records steer the next in mtm_match_blocks_passes, and
 * so on.  planes: every pass's N_p (2 margin_p + 1)^2 floats, pass after pass; out_hits (may be NULL): the n peak records.
 * All planes together above MTM_OPT_BOXES_MAX_FLOATS return MTM_E_INVALID.  A pass needs every pair: a stack that fits one
 * frame chunk goes up once, any other once per pass.  One host wait per call. */
int mtm_match_blocks_stack_passes(mtm_ctx* ctx, const void* const* frames, int n_frames, int rows, int cols, int chans,
                                  int dtype, int64_t row_stride_bytes, const mtm_block_pass* passes, int n_passes, int method,
                                  int mode, mtm_hit* out_hits, float* nbhd, float* planes);

/* Test support: blocks_plane_peak_kernel on constructed sums (ctx == NULL: the same rule on the host).  acc: n planes of
 * side x side float64 sums (side odd); block k's clipped box covers cells oy <= cy < oy + oh[k], ox <= cx < ox + ow[k],
 * (ox, oy) = clip[2 k], clip[2 k + 1].  planes_out: n side^2 floats, (float)(acc / pairs) inside the box and NaN outside;
 * recs_out[k]: the peak as mtm_match_blocks_stack_at records it for a block centred on (0, 0) - x = dx, y = dy, w = h = 0 -,
 * (-1, -1) and NaN for a plane without a number. */
int mtm_debug_plane_peaks(mtm_ctx* ctx, const double* acc, int n, int side, const int32_t* clip, const int32_t* oh,
                          const int32_t* ow, int pairs, int method, float* planes_out, mtm_hit* recs_out);


/* Window deformation.  THE RULE, in integers.  A coarse grid of nx x ny blocks of size (wc, hc) at stride (sx,
 * sy), row-major, carries displacements d[j nx + i] = (dx, dy).  Coordinates are doubled: pixel x is X2 = 2 x, the centre of a
 * block at x of width w is X2 = 2 x + w - 1, the centre of coarse column i is Cx_i = 2 i sx + wc - 1.  Per axis, nx == 1: i =
 * 0, ax = 0; else i = clamp(floor((X2 - (wc - 1)) / (2 sx)), 0, nx - 2), a = clamp(X2 - Cx_i, 0, 2 sx), ax = (256 a + sx) / (2
 * sx) in 0 .. 256 (constant extrapolation outside the centres' hull); j, ay likewise; i1 = min(i + 1, nx - 1), j1 likewise.
 * The field in Q8 (1/256 pixel), per component, in int64, the shift arithmetic (a floor):
 *   F = (d[j,i] (256 - ax)(256 - ay) + d[j,i1] ax (256 - ay) + d[j1,i] (256 - ax) ay + d[j1,i1] ax ay + 128) >> 8.
 * The warp: output pixel (x, y) samples X = clamp(256 x + Fx(2 x, 2 y), 0, 256 (W - 1)), Y likewise with H; x0 = X >> 8, fx =
 * X & 255, x1 = min(x0 + 1, W - 1), y0, fy, y1 likewise; per channel
 *   out = (I[y0,x0] (256 - fx)(256 - fy) + I[y0,x1] fx (256 - fy) + I[y1,x0] (256 - fx) fy + I[y1,x1] fx fy + 32768) >> 16.
 * A zero field returns the image, an integer constant field the shifted image with replicated edges, both exactly.
 *
 * mtm_deform_image warps one image by the field of `displacements` (2 int32 per block of the grid of bw x bh blocks at stride
 * (sx, sy) over the image, row-major: dx, dy; each within +-2^22) into `out` (the image's shape and pixel type, rows
 * out_stride_bytes apart).  uint8 with 1 or 3 channels or single-channel uint16, at most 65535 rows; an empty grid is
 * MTM_E_INVALID.  ctx == NULL runs the rule on the host (no GPU); with a context the image and the displacements are
 * uploaded, the warp kernel is launched once and the warped image comes back: one wait (mtm_get_timing: total_ms is the
 * warp kernel's time alone).  The image becomes the context's current image. */
int mtm_deform_image(mtm_ctx* ctx, const void* px, int64_t row_stride_bytes, int rows, int cols, int chans, int dtype, int bw,
                     int bh, int sx, int sy, const int32_t* displacements, void* out, int64_t out_stride_bytes);

/* mtm_match_blocks_passes with window deformation between the passes.  Pass 0 is unchanged.  For a pass p >=
 * 1, with d the displacements (record position - block position) of the records that steer it - pass p - 1's, or with valid
 * != NULL the validated ones of mtm_match_blocks_passes_validated -: the whole ORIGINAL image is warped by the field of d (the
 * rule above; never a warp of a warp) into a buffer of its own, every block of pass p is searched in the warped image in its
 * own box widened by the pass's margin (no offset), nbhd's neighbourhoods come from the warped image, and with c = F at the
 * block's doubled centre (2 x + w - 1, 2 y + h - 1) the record's position is the one found plus ((c + 128) >> 8) per
 * component - not clamped: it may lie outside the image, it carries a displacement.  That record is what `out` holds, what
 * validation tests and what steers pass p + 1.  predicted (required): 2 int32 per record, pass-major as out, c in Q8, zero
 * for pass 0; a refined position is the fitted one in the warped image plus c / 256.  valid may be NULL (no validation;
 * threshold and epsilon are then not read).  n_passes * max(rows, cols) must not pass 2^22.  Still one wait; a deformed
 * pass launches the warp and two small kernels, and no unit kernel.  Everything else as mtm_match_blocks_passes. */
int mtm_match_blocks_passes_deformed(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                                     int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                     const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                     mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted);

/* Sub-pixel steering of the deformed passes.  THE RULE.  The fit: per axis the three float32 scores of the
 * record's 3 x 3 neighbourhood (neighbour at -1, centre, neighbour at +1) widened to double as a, b, c, negated for methods 0
 * and 1; d = (a - 2.0 b) + c; the offset o = 0.5 (a - c) / d when a, b, c are finite, b >= a, b >= c and d < 0, else 0.0
 * (IEEE float64, nothing contracted).  The Q8 position: P = (double)pos_w + o per component, pos_w the integer position found
 * in the searched (warped) image; Q = floor(256.0 P + 0.5).  The steering displacement of record k of a pass, b its block's
 * (x, y) and c the pass's predicted field at the block's centre (Q8; zero for pass 0): D8 = Q - 256 b + c; with validation an
 * outlier - flagged as before, on the integer record - takes D8 = 256 rep, rep its neighbours' integer median.  The filter over
 * the pass's ny x nx grid, per component in int64, reading only the unfiltered set:
 *   S8[j,i] = (sum over u, v in {-1, 0, 1} of k[u] k[v] D8[clamp(j + u, 0, ny - 1), clamp(i + v, 0, nx - 1)] + 8) >> 4,
 * k = (1, 2, 1), the shift arithmetic.  The field of Q8 nodes S (|S| <= 2^30), (i, ax), (j, ay) as above:
 *   F = (S[j,i] (256 - ax)(256 - ay) + S[j,i1] ax (256 - ay) + S[j1,i] (256 - ax) ay + S[j1,i1] ax ay + 32768) >> 16,
 * which for S = 256 d is the F of d above, bit for bit.  The warp and the record's shift (c + 128) >> 8 are unchanged.
 *
 * mtm_match_blocks_passes_steered is mtm_match_blocks_passes_deformed with the argument `steer`: 0 is that function in every
 * respect (the same launches); 1 steers every pass p >= 1 by the field of the S8 of pass p - 1 instead of the field of its
 * integer records - the neighbourhoods of every pass that steers another are then computed whether or not nbhd is asked
 * for, and two small kernels (one lane per record: D8; one lane per node: S8) follow such a pass.  out, nbhd, valid and
 * predicted keep their meaning and layout; the last pass steers nothing.  Any other steer is MTM_E_INVALID naming it. */
int mtm_match_blocks_passes_steered(mtm_ctx* ctx, const void* reference, int64_t reference_stride_bytes, const void* image,
                                    int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                    const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                    mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted, int steer);

/* mtm_deform_image with displacements in Q8 (1/256 pixel), each within +-2^30: the warp by the field of Q8 nodes above - how a
 * frame is registered when its drift field is known to sub-pixel precision.  256 d gives mtm_deform_image's pixels of d.
 * ctx == NULL runs the rule on the host.  Everything else as mtm_deform_image. */
int mtm_deform_image_q8(mtm_ctx* ctx, const void* px, int64_t row_stride_bytes, int rows, int cols, int chans, int dtype, int bw,
                        int bh, int sx, int sy, const int32_t* displacements_q8, void* out, int64_t out_stride_bytes);

/* Test support: the steering displacements of one pass over a grid of nx x ny blocks at stride (sx, sy), row-major.  recs:
 * the pass's records (positions: the one found plus the rounded field); nbhd: 9 floats per record; predicted: 2 int32 per
 * record, the pass's field in Q8; valid and steer_recs: both NULL, or the flags and validated records of the median test;
 * mode_min: 1 for methods 0 and 1.  out_q8: 2 int32 per record - D8, or with smooth != 0 the filtered S8.  ctx == NULL runs the
 * inline functions on the host (no GPU); with a context everything is uploaded, the steer kernel and - smooth != 0 - the
 * filter kernel are launched once each and out_q8 comes back. */
int mtm_debug_steer_q8(mtm_ctx* ctx, const mtm_hit* recs, const float* nbhd, const int32_t* predicted, const uint8_t* valid,
                       const mtm_hit* steer_recs, int nx, int ny, int sx, int sy, int mode_min, int smooth, int32_t* out_q8);

/* The 3 x 3 score neighbourhoods of n points in one call: out[9 k + 3 (1 + dy) + (1 + dx)] = the score of
 * template pts[k].templ_idx at window (x + dx, y + dy) of the image's score map, NaN for a window outside the map.  Image:
 * uint8 or float32 with 1 or 3 channels, or single-channel uint16, the templates' pixel type; masked templates (uint8 or
 * float32, methods 0..3) as mtm_set_templates took them.  uint8 and uint16 scores are mtm_score_map's bit for bit in the
 * default MTM_OPT_EXACT_DIV mode; float32 scores agree with it to rounding (window sums in float64 of the window itself).
 * The image crosses PCIe once.  A template index out of range, a window outside the map, or a template whose pixel type or
 * channel count differs from the image's returns MTM_E_INVALID and names the point.  The image becomes the context's
 * current image. */
int mtm_hit_neighbourhoods(mtm_ctx* ctx, const void* px, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, const mtm_point* pts, int n, float* out);

/* Stream form of mtm_find_matches ("thousands of images", reference
 * tutorials/Tutorial3-SpeedingUp.ipynb:564: same templates, one image after the other): returns the
 * hits of the CURRENT image exactly like mtm_find_matches and makes `next_px` the current image for
 * the following call.  The next image is uploaded and converted on a second HIP stream while the
 * kernels of the current image run, so its PCIe transfer costs no wall-clock.
 * The caller's buffer is only read during the call.  On MTM_E_OVERFLOW the swap has happened too
 * (fetch the hits with mtm_last_hits). */
int mtm_find_matches_next(mtm_ctx* ctx, int mode, double score_threshold, mtm_hit* out, int64_t capacity,
                          int64_t* n_out, const void* next_px, int rows, int cols, int chans, int dtype,
                          int64_t row_stride_bytes);

/* Split form of mtm_find_matches for hosts that want to work while the GPU does: _async queues everything
 * the call needs on the context's stream (statistics, score kernels, the fetch of the candidate list) and
 * returns without waiting for the GPU; _wait synchronises, extracts the peaks and delivers the hits exactly
 * like mtm_find_matches (MTM_E_OVERFLOW: fetch them with mtm_last_hits).  mtm_find_matches is the two
 * back to back.  Between the two the context must not be used for anything else; one call in flight per
 * context.  (The reference gets its overlap from a thread pool per call, MTM/__init__.py:172-175; a Python
 * host holds the GIL while it builds the hit list of the previous image, so the overlap has to come from
 * the native side.) */
int mtm_find_matches_async(mtm_ctx* ctx, int mode, double score_threshold);
int mtm_find_matches_wait(mtm_ctx* ctx, mtm_hit* out, int64_t capacity, int64_t* n_out);

/* The hit list of the last mtm_find_matches call again, without recomputing anything: the way to
 * collect the result after MTM_E_OVERFLOW told the caller the capacity it needs. */
int mtm_last_hits(mtm_ctx* ctx, mtm_hit* out, int64_t capacity, int64_t* n_out);

/* The score map of template `templ_idx` exactly as the last mtm_find_matches call computed it inside its
 * batched launch (cv2.matchTemplate, MTM/__init__.py:92) - nothing is recomputed.  Only valid when that call
 * materialised the maps (MTM_OPT_HITS_ONLY = 0, or any class that is not on the MFMA kernel); MTM_E_STATE
 * otherwise.  Parity tests use it to check the production launch at full size against the oracle. */
int mtm_last_score_map(mtm_ctx* ctx, int templ_idx, float* out, int64_t out_row_stride_bytes);

int mtm_get_timing(mtm_ctx* ctx, mtm_timing* out);

/* cv2.dnn.NMSBoxes as MTM.NMS uses it (MTM/NMS.py:73-82): keep hits with score > threshold
 * (float32, strict), stable sort by descending score, greedy IoU suppression with
 * overlap <= max_overlap, optional truncation to n_object (-1 = no limit).  `ascending` applies
 * the 1-score transform of MTM/NMS.py:73-75.  Host code (C++), no GPU needed.
 * keep[] receives indices into hits[]; capacity of keep must be >= n. */
int mtm_nms(const mtm_hit* hits, int64_t n, double score_threshold, int ascending,
            int64_t n_object, double max_overlap, int32_t* keep, int64_t* n_keep);

/* mtm_nms on each of n_seg consecutive segments of hits[] (segment s: seg_counts[s] records, in mtm_find_matches' order) as
 * MTM.matchTemplates applies it to one search's hit list: a segment of at most one hit is kept as it is (MTM/NMS.py
 * returns such a list unchanged), every other one goes through the suppression without a limit on the count.  keep[]
 * receives the kept records' indices into hits[], segment after segment; keep_counts[s] = how many of them are segment s's.
 * Capacity of keep: the total number of hits.  Host code (C++), no GPU needed. */
int mtm_nms_segments(const mtm_hit* hits, const int64_t* seg_counts, int64_t n_seg, double score_threshold, int ascending,
                     double max_overlap, int32_t* keep, int64_t* keep_counts);

/* ---- multi-GPU, one process: a group of per-device contexts -------------------------------- */
/* The units (templates / rotations / scales) of a search are independent given the image - the reference runs
 * one thread-pool task per template (MTM/__init__.py:172-175).  A group holds one context and one worker thread
 * per listed device (a device may be listed more than once: several contexts on one GPU).  A search shards the
 * units over the devices by longest-processing-time-first on their multiply-accumulate cost
 * out_px * w * h * C (* 2 with a mask), every device uploads the image and searches its shard concurrently
 * (mtm_set_templates + mtm_find_matches_image; unchanged templates stay resident per device), and the hit lists
 * are merged on the host in template order: the result equals the single-device call.  No collective: in one
 * process every list is in host memory when its worker returns (the one-process-per-GPU form with the RCCL
 * all-gather follows below). */
typedef struct mtm_group mtm_group;
int      mtm_group_create(mtm_group** out, const int* device_ids, int n_devices);
void     mtm_group_destroy(mtm_group* g);
int      mtm_group_size(const mtm_group* g);
mtm_ctx* mtm_group_ctx(mtm_group* g, int i);                       /* per-device context (options, timing) */
int      mtm_group_set_option(mtm_group* g, int option, int64_t value);   /* on every context */
/* the partition a search would use: device_of_unit[i] = index (0 .. size-1) of the device unit i goes to */
int      mtm_group_shards(const mtm_group* g, const mtm_templ* templs, int n_templ, int method, int rows, int cols,
                          int32_t* device_of_unit);
/* mtm_set_templates + mtm_find_matches_image over all devices; hits ordered as mtm_find_matches orders them */
int      mtm_group_find_matches(mtm_group* g, const mtm_templ* templs, int n_templ, int method,
                                const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                                int mode, double score_threshold, mtm_hit* out, int64_t capacity, int64_t* n_out);
/* The same + MTM's non-maxima suppression on the merged list inside the call (round 5; what mtm_find_matches_image_nms is
 * to a single context): local extrema, the kept hits in cv2.dnn.NMSBoxes' order, at most n_object of them (-1: all).
 * Replaces MTM.matchTemplates -> findMatches + NMS (MTM/__init__.py:289-296) for a device group in ONE native call. */
int      mtm_group_find_matches_nms(mtm_group* g, const mtm_templ* templs, int n_templ, int method,
                                    const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                                    double score_threshold, double max_overlap, int64_t n_object,
                                    mtm_hit* out, int64_t capacity, int64_t* n_out);
int      mtm_group_last_hits(mtm_group* g, mtm_hit* out, int64_t capacity, int64_t* n_out);
/* The hit exchange of a group as north_star / SURVEY 8e name it: a single process, ncclCommInitAll over the group's
 * devices, one stream per device, ONE all-gather of fixed-size slots of 24-byte hit records per device inside
 * ncclGroupStart / ncclGroupEnd; rank 0's gathered list is merged and returned (the reference's fan-in,
 * MTM/__init__.py:173-177, followed by the one global NMS of MTM/NMS.py:78).  mtm_group_comm_init() creates the
 * communicators and selects that exchange; it fails with MTM_E_COMM - and the group keeps the host merge - when RCCL is
 * missing or a device is listed twice (RCCL takes one rank per device).  mtm_group_comm_ranks(): ncclCommCount of rank 0
 * (0 without communicators).  mtm_group_set_exchange() switches between the two; both deliver the same list. */
#define MTM_GROUP_EXCHANGE_HOST 0
#define MTM_GROUP_EXCHANGE_RCCL 1
int      mtm_group_comm_init(mtm_group* g);
int      mtm_group_comm_ranks(mtm_group* g);
int      mtm_group_set_exchange(mtm_group* g, int kind);
int      mtm_group_exchange_used(const mtm_group* g);            /* what the last mtm_group_find_matches used */

/* ---- multi-GPU: one process per GPU, templates sharded across ranks (north_star) ------------ */
/* RCCL all-gather of per-rank hit lists over xGMI.  The 128-byte unique id is created on rank 0
 * and distributed by the caller's bootstrap (torch.distributed store, MPI, a file...). */
#define MTM_COMM_ID_BYTES 128
int mtm_comm_unique_id(void* id_out /* MTM_COMM_ID_BYTES */);
int mtm_comm_init(mtm_ctx* ctx, const void* id, int n_ranks, int rank);
/* all-gather: every rank contributes n_local hits; out receives the concatenation in rank order.
 * counts_out[n_ranks] receives the per-rank counts.  Collective call with a deadline: if the other ranks do not
 * arrive within MTM_COMM_TIMEOUT_S seconds (environment; default 300, 0 = wait for ever) the communicator is
 * aborted (ncclCommAbort), the call returns MTM_E_COMM and the context goes back to single-rank operation. */
int mtm_comm_allgather_hits(mtm_ctx* ctx, const mtm_hit* local, int64_t n_local,
                            mtm_hit* out, int64_t capacity, int64_t* counts_out, int64_t* n_out);
/* The result of the last mtm_comm_allgather_hits again (no communication): the way to collect it after
 * MTM_E_OVERFLOW told the caller the capacity it needs.  The collective itself is never repeated - a rank whose
 * buffer was large enough has already left it. */
int mtm_comm_last_gather(mtm_ctx* ctx, mtm_hit* out, int64_t capacity, int64_t* counts_out, int64_t* n_out);
int mtm_comm_destroy(mtm_ctx* ctx);
/* The same exchange for n contexts of ONE process (what mtm_group_comm_init / mtm_group_find_matches use): communicators
 * by ncclCommInitAll over the contexts' devices (context i becomes rank i; MTM_E_COMM if two contexts share a device),
 * and one call that queues every rank's all-gather inside ncclGroupStart / ncclGroupEnd, each on its context's stream, and
 * returns rank 0's gathered list.  mtm_comm_count(): ncclCommCount of the context's communicator, 0 without one. */
int mtm_comm_init_all(mtm_ctx* const* ctxs, int n);
int mtm_comm_count(mtm_ctx* ctx);
int mtm_comm_allgather_hits_all(mtm_ctx* const* ctxs, int n, const mtm_hit* const* local, const int64_t* n_local,
                                mtm_hit* out, int64_t capacity, int64_t* counts_out, int64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* MTM_HIP_H */
