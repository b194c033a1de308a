// The route of one mtm_find_matches call, as a host-only header (no HIP): the GPU side sees it through mtm_ctx.h, the
// host-only unit (mtm_host.cpp: the overflow ladder's decision) and its CPU driver (tests/native/sanitize_host.cpp)
// through mtm_internal.h.  Not part of the ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mtm_hip.h"

// The route of one mtm_find_matches call: what plan_call decides from the context, the mode and the threshold, what the
// launches record for the call, and where fm_end's overflow transitions take it.  It lives as long as the call
// (mtm_find_matches_async / mtm_find_matches_wait keep it in mtm_ctx::fm in between); what lasts across calls - the
// back-off counters, hit_cap, cands_zeroed - stays on the context.
namespace mtmi {
// mtm_find_matches_image_nms: MTM.matchTemplates' non-maxima suppression as part of the call (the host's nms_boxes on
// the fetched list).  Thousands of peaks on the device (the flagged-segment route of dense images) are pruned there
// first (mtm_k_nms.hip.h; MTM_NMS_DEVICE=0: never): what a neighbourhood's best hit suppresses never crosses PCIe.
struct NmsRequest {
    bool on = false;
    double score_threshold = 0.0, max_overlap = 0.0;
    long long n_object = -1;
};
struct CallRoute {
    int mode = MTM_PEAKS_LOCAL;
    int n = 0;
    float thr = 0.0f;
    bool mode_min = false;
    // candidate emission of the launches being queued: threshold (quality: -score for minima) and direction
    bool cand_on = false, cand_min = false;
    float cand_thr = 0.0f;
    bool fused = false;         // local extrema from the kernels' candidate list (verify_peaks / the host's 3x3 test)
    bool hits_only = false;     // ... and no maps in memory (candidates + hash verify)
    bool ext = false;           // global extrema come out of the MFMA epilogue (no maps, no extremum_kernel)
    bool sparse = false;        // segment flags: maps in memory, peaks_sparse_kernel over the flagged row segments
    int flag_tstride = 0, flag_rstride = 0;     // ... the flags' layout (seg_flags[t * flag_tstride + row * flag_rstride + segment])
    bool seg_skip_used = false; // some map holds placeholders for outputs that cannot pass (the maps are not published)
    // float32 refinement (mtm_refine.hip.h)
    bool refine = false;        // bf16 classes are refined
    bool refine_scan = false;   // ... by map scan + ring re-scoring (maps in memory) instead of kernel candidates
    bool pp_mode = false;       // the candidate buffer holds the map scan's potential peaks, whose neighbourhoods in the maps
                                // are exact - decisions by verify_peaks_kernel, never from the list alone
    bool f32_exact = false;     // bf16 classes run the float64 kernel
    bool raw_rig = false;       // a raw-sum method with a threshold, listed by the bound of the sum (kernel candidates only)
    float rig_thr = 0.0f;       // the exact quality threshold (the lists' own cand_thr carries a margin in map mode)
    float scan_thr = 0.0f;      // map mode: the threshold of refine_scan_kernel (rig_thr lowered by rig_cap)
    float rig_cap = 0.0f;       // map mode: the bound up to which the scan's tolerances hold (else: float64 kernel)
    int bf16_np = 3;            // piece products of the hits-only screens (1: the one-product screen)
    // masked float32 classes screened on the bf16 matrix cores (launch_masked_bf16)
    bool mbf_thr_on = false;    // local extrema against mbf_thr, or (mbf_global) the global extremum
    bool mbf_global = false;
    float mbf_thr = 0.0f;
    bool mbf_used = false;      // some class's maps hold "below the threshold" placeholders
    // the candidate list's landing buffer: the score kernel writes its head there itself (cand_pin: the first pass only)
    bool cand_pin = false, pin_direct = false, prefetched = false;
    size_t cand_pin_n = 0;
    bool banded_u8 = false;     // the image came in row bands (uint8): such calls clear the candidate header themselves
    bool zero_pending = false;  // ... and this one has not done so yet
    bool single_band = false;   // the banded upload is ONE band (banded_ok: a call too small for two score launches)
    int64_t cand_cap = 0;
    unsigned hash_mask = 0;
    // the tail screen's split of the call (tail_split_for): the rule's value, computed once for the call's threshold and
    // class shape - every statistics and score launch of every band then carries the same one
    int tail_h = 0, tail_w = 0, tail_s = 0;
    float tail_thr = 0.0f;
    NmsRequest nms;
    long long nms_raw_count = -1;   // >= 0: the device pruned the peak list; the count before that
    long long nms_sure = 0;         // ... and its first nms_sure hits are kept for certain (the neighbourhoods' best)
};
}  // namespace mtmi
