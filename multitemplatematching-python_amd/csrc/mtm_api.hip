// libmtm_hip.so - the search entry points: mtm_find_matches and its variants (the route of a call, its score pass, the
// fallback ladder around the peak pass of mtm_peaks.hip, host verification of the kernels' candidates, hit lists), score
// maps, timing.  Launches no kernel itself.
#include "mtm_ctx.h"

using namespace mtm;
using namespace mtmi;

namespace {

struct NextImage {
    const void* px;
    int rows, cols, chans, dtype;
    int64_t stride;
    bool staged;
};

// Enqueue the upload + plane conversion of the next image of a stream on the copy stream, into the
// image slot the kernels are not reading.  Called by find_matches_impl after the kernels of the
// current image are enqueued and before it waits for them: the PCIe transfer (and the host-side
// staging the runtime does for pageable memory) runs under the kernels.
int stage_next_image(mtm_ctx* c, NextImage* nx) {
    if (!nx || nx->staged) return MTM_OK;
    MTMC(ensure_copy_stream(c));
    if (!c->next_ready) HIPC(hipEventCreateWithFlags(&c->next_ready, hipEventDisableTiming));
    // The runtime batches stream commands and only submits them when somebody asks about the stream:
    // push the kernels of the current image out first, then (below) the copy, so that they overlap.
    (void)hipStreamQuery(c->stream);
    // straight from the caller's (pageable) rows: the runtime stages them through its own pinned
    // buffers, which measured 5x faster than a host copy into hipHostMalloc memory on this platform
    MTMC(upload_image(c, c->slot[1 - c->cur], nx->px, nx->stride, nx->rows, nx->cols, nx->chans, nx->dtype,
                      c->copy_stream));
    HIPC(hipEventRecord(c->next_ready, c->copy_stream));
    (void)hipStreamQuery(c->copy_stream);
    nx->staged = true;
    return MTM_OK;
}

int find_matches_impl(mtm_ctx* c, int mode, double score_threshold, mtm_hit* out, int64_t capacity,
                      int64_t* n_out, NextImage* next, const ImageArgs* up = nullptr, const NmsRequest* nms = nullptr);

// The route of a call on the placed templates and the current image (`banded`: it arrives in row bands), decided from the
// context's switches and back-off counters.  No HIP call, no change to the context: fm_begin acts on what it returns.
CallRoute plan_call(const mtm_ctx* c, int mode, float thr, bool banded) {
    CallRoute R;
    const int n = (int)c->templs.size();
    const bool mode_min = method_mode_min(c->method);
    R.mode = mode;
    R.n = n;
    R.thr = thr;
    R.mode_min = mode_min;
    R.cand_cap = std::min<int64_t>(c->hit_cap, kCandListMax);
    R.banded_u8 = banded && c->dtype == MTM_U8;
    // masked float32 classes: the bf16 screen needs the threshold - local extrema, or (mbf_global) the templates' best
    // lower bounds and everything that reaches them; mtm_score_map (a route of its own, no threshold) keeps the float64
    // kernel.  What the peak pass compares with: the float32 threshold, on float32 scores.
    R.mbf_thr_on = n > 0 && f32_refined(c);
    R.mbf_global = mode == MTM_PEAKS_GLOBAL;
    R.mbf_thr = thr;

    // fused peak candidates: only when every class runs the MFMA kernel - and not while the maps of this context are
    // known to be dense (the last attempts overflowed the candidate list: smooth images at a low threshold), where the
    // full peak pass over the maps is the cheaper route
    bool fused = mode == MTM_PEAKS_LOCAL && n > 0 && c->fuse_backoff == 0;
    // Segment flags (the default route while the back-off lasts): the maps go to memory as in map mode, and the score kernel
    // sets a flag per row segment (a wave's 256 outputs of one template row) in which something passes the threshold;
    // peaks_sparse_kernel visits those instead of scanning 1 GB of maps (4K x 32 templates).  A first version wrote only
    // the flagged segments, from the hits-only screens: no faster - on such images the screens pass nearly everywhere.
    // uint8 classes on the lean 1- / 3-channel MFMA epilogue, every map 2-D.
    if (mode == MTM_PEAKS_LOCAL && n > 0 && !fused && c->sparse_maps && c->hits_only &&
        c->dtype == MTM_U8 && (c->chans == 1 || c->chans == 3) && (int)c->list2d.size() == n) {
        bool ok = true;
        int max_oh = 0, max_nseg = 0;
        for (const SizeClass& sc : c->classes) {
            ok = ok && sc.kernel == MTM_KERNEL_MFMA && sc.slabs.empty();
            max_oh = std::max(max_oh, c->rows - sc.h + 1);
            max_nseg = std::max(max_nseg, (c->cols - sc.w + 1 + kMfSeg - 1) / kMfSeg);
        }
        // (bounded: the flags are cleared on every call and compact_hits_kernel sums the per-(template, strip) counters in
        // every block - with thousands of templates the flagged route would cost more than the full scan it replaces)
        if (ok && (long long)n * max_oh * max_nseg <= (64ll << 20) && (long long)n * max_nseg <= 4096) {
            R.flag_rstride = max_nseg;
            R.flag_tstride = max_oh * max_nseg;
            R.sparse = true;
            R.cand_min = mode_min;          // the threshold the score kernel flags against (launch_ncc)
            R.cand_thr = mode_min ? -thr : thr;
        }
    }
    for (const SizeClass& sc : c->classes) {
        fused = fused && (sc.kernel == MTM_KERNEL_MFMA || sc.kernel == MTM_KERNEL_MFMA16 || sc.kernel == MTM_KERNEL_MFMA_F32);
    }
    // float32 images on the bf16 matrix cores: the kernel's scores are a screen, the decisions are taken on exact
    // float64 scores (mtm_refine.hip.h).  Calls that mix bf16 classes with float64-kernel ones (float masks) run
    // everything on the float64 kernel.  (refine and f32_exact exclude each other on every route.)
    {
        bool any_bf16 = false, all_bf16 = n > 0;
        for (const SizeClass& sc : c->classes) {
            const bool b = sc.kernel == MTM_KERNEL_MFMA_F32;
            any_bf16 = any_bf16 || b;
            all_bf16 = all_bf16 && b;
        }
        // raw sums (TM_SQDIFF / TM_CCORR / TM_CCOEFF): only the refined global extremum runs on the matrix cores - maps and
        // thresholds on unnormalised sums have no error the bf16 pieces could promise (an exact copy is TM_SQDIFF 0)
        const bool raw_m = c->method == MTM_TM_SQDIFF || c->method == MTM_TM_CCORR || c->method == MTM_TM_CCOEFF;
        // ... except, round 5, local extrema against a threshold while the kernel's candidate list is available: every output
        // whose upper bound (score + E, E in the sum's own units) passes the threshold is listed and re-scored exactly -
        // route 1 only; maps, the map scan and every overflow keep the float64 kernel
        R.raw_rig = any_bf16 && all_bf16 && raw_m && mode == MTM_PEAKS_LOCAL && f32_refined(c) && fused;
        if (any_bf16 && raw_m && (mode != MTM_PEAKS_GLOBAL || !f32_refined(c)) && !R.raw_rig) {
            R.f32_exact = true;
        } else if (any_bf16 && f32_refined(c)) {
            if (all_bf16) R.refine = true;
            else R.f32_exact = true;
        }
    }
    if (R.f32_exact) fused = false;                 // the float64 kernel writes maps and lists no candidates
    // fused global extremum (cv2.minMaxLoc inside the score kernel): every class on the 1- or 3-channel MFMA kernel
    // (plain, two-row, row-multiplexed or in slabs - there in slab_combine_kernel; binary masks with the reciprocal
    // normalisation), the uint16 byte-plane kernel
    // or the float32 kernel; same switch as the hits-only mode (MTM_OPT_HITS_ONLY)
    if (mode == MTM_PEAKS_GLOBAL && c->hits_only && n > 0 && (c->chans == 1 || c->chans == 3) && !R.f32_exact) {
        bool ok = true;
        for (const SizeClass& sc : c->classes)
            ok = ok && ((sc.kernel == MTM_KERNEL_MFMA &&
                         (!sc.masked || (c->exact_div < 2 && c->chans == 1 && c->method <= MTM_TM_CCORR_NORMED))) ||
                        sc.kernel == MTM_KERNEL_MFMA16 || sc.kernel == MTM_KERNEL_MFMA_F32);
        if (ok) {
            R.ext = R.cand_on = R.hits_only = true;
            R.cand_min = mode_min;
            R.cand_thr = 0.0f;
        }
    }
    if (mode == MTM_PEAKS_GLOBAL && R.refine && !R.ext) {
        // no fused extremum in this configuration (maps requested, MTM_FUSE_PEAKS=0): the float64 kernel + extremum_kernel
        R.refine = false;
        R.f32_exact = true;
    }
    // the refined routes' own thresholds: rig_thr the exact one, rig_cap the widest error bound the map scan's tolerances
    // cover (4 x the largest class constant: windows whose mean lies within ~4 standard deviations of their tile's)
    if (R.refine) {
        const float tq = mode_min ? -thr : thr;
        R.rig_thr = tq;
        float eps = 0.0f;
        for (const SizeClass& sc : c->classes)
            if (sc.kernel == MTM_KERNEL_MFMA_F32) eps = std::max(eps, bf16_rig_eps(c->chans, sc.h, bf16_nkb(sc.w)));
        R.rig_cap = std::max(kRefineThrMargin, 4.0f * eps);
        R.scan_thr = tq - R.rig_cap * std::max(1.0f, std::fabs(tq));
    }
    // float32 refinement without kernel candidates: the potential peaks of a map scan, listed in the candidate buffer
    if (mode == MTM_PEAKS_LOCAL && R.refine && !fused && n > 0) {
        R.pp_mode = R.refine_scan = true;
        R.cand_min = mode_min;
        R.cand_thr = R.scan_thr;
    }
    if (fused) {
        R.fused = R.cand_on = true;
        // the counter is normally cleared right after the previous call fetched it (off the critical path); round 5: a banded
        // uint8 call lets its first statistics launch do it (zero_pending; run_score_banded) - no fill command at all
        R.zero_pending = R.banded_u8;
        R.cand_min = mode_min;
        R.cand_thr = mode_min ? -thr : thr;
        // (float32 refinement: everything within the margin of the threshold is listed and re-scored)
        if (R.refine) R.cand_thr -= kRefineThrMargin * std::max(1.0f, std::fabs(R.cand_thr));
        // hits-only: single-channel MFMA classes, every map 2-D, no recent candidate overflow
        R.hits_only = c->hits_only && (c->chans == 1 || c->chans == 3) && (int)c->list2d.size() == n;
    }
    // hash table of the candidate positions (hits-only verification on the device: only when the
    // candidates are too many to be checked on the host, see fm_end)
    if (R.hits_only && !R.ext) {
        R.hash_mask = (unsigned)(cand_hash_slots(R.cand_cap) - 1);
    }
    // The landing buffer of the candidate list (pinned).  Round 5: when every class of the call runs ncc_mfma_kernel's own
    // epilogue, the waves that fill the first slots of the list write them there as well (MfmaParams::cand_pin) and the
    // host finds them when the last score launch has ended - no fetch kernel (or copy command) with its kernel boundary
    // behind the score pass.
    R.prefetched = mode == MTM_PEAKS_LOCAL && fused && !c->list2d.empty();
    if (R.prefetched) {
        bool pin = c->cand_pinned != 0 && !R.refine;
        for (const SizeClass& sc : c->classes) {
            pin = pin && ((sc.kernel == MTM_KERNEL_MFMA && sc.slabs.empty()) || sc.kernel == MTM_KERNEL_MFMA16);
        }
        R.cand_pin = pin;
        R.cand_pin_n = std::min<size_t>(kHitPrefetch, (size_t)R.cand_cap);
    }
    // float32: the hits-only refined routes (kernel candidates re-scored; the fused extremum by bounds) and the masked
    // classes' screen start with ONE piece product unless a recent call overflowed its list that way
    R.bf16_np = c->dtype == MTM_F32 && c->f32_mfma == 1 && c->np1_backoff == 0 ? 1 : 3;
    return R;
}

int fm_begin(mtm_ctx* c, int mode, double score_threshold, NextImage* next, CallRoute& R, const ImageArgs* up = nullptr) {
    HIPC(hipSetDevice(c->device));
    bool banded = false, single_band = false;
    if (up) {
        // the geometry first (placement depends on it); the pixels follow in stream order
        adopt_image(c, up->rows, up->cols, up->chans, up->dtype);
        c->have_image = false;                       // until the upload is queued: an error below leaves no stale image
        if (!c->have_templ) {
            set_error("set the templates first");
            return MTM_E_STATE;
        }
        c->have_image = true;
    }
    host_trace(c, 1);
    MTMC(place_templates(c));
    host_trace(c, 2);
    if (up) {
        banded = banded_ok(c, *up, &single_band);
        if (!banded) {
            const int rc = upload_image(c, c->slot[c->cur], up->px, up->stride, up->rows, up->cols, up->chans, up->dtype,
                                        c->stream);
            if (rc != MTM_OK) {
                c->have_image = false;
                return rc;
            }
        }
    }
    c->timing = mtm_timing{};
    c->maps_valid = false;
    // numpy compares the float32 map with the python-float threshold in float32
    R = plan_call(c, mode, (float)score_threshold, banded);
    R.single_band = single_band;
    host_trace(c, 18);
    // the back-off countdowns: a call the back-off kept from its route counts it down
    if (mode == MTM_PEAKS_LOCAL && R.n > 0 && c->fuse_backoff > 0) --c->fuse_backoff;
    if (c->dtype == MTM_F32 && c->f32_mfma == 1 && c->np1_backoff > 0) --c->np1_backoff;

    // the route's buffers
    if (R.sparse) {
        MTMC(c->seg_flags.ensure((size_t)R.n * R.flag_tstride));
        HIPC(hipMemsetAsync(c->seg_flags.p, 0, (size_t)R.n * R.flag_tstride, c->stream));
    }
    if (R.ext) {
        MTMC(c->counters.ensure(sizeof(unsigned long long) * 2 * (size_t)R.n));
        HIPC(hipMemsetAsync(c->counters.p, 0, sizeof(unsigned long long) * 2 * (size_t)R.n, c->stream));
    }
    // the candidate buffer: kernel candidates, and the refined routes' records - the outputs within the margin of the running
    // best (global extremum), the potential peaks of the map scan (local extrema without kernel candidates)
    if (R.fused || R.pp_mode || (R.refine && R.ext)) {
        const size_t cands_cap = c->cands.cap;
        MTMC(c->cands.ensure(16 + sizeof(mtm_hit) * (size_t)c->hit_cap));
        if (c->cands.cap != cands_cap) c->cands_zeroed = nullptr;      // reallocated (possibly at the same address)
        if (!R.zero_pending && c->cands.p != c->cands_zeroed) HIPC(hipMemsetAsync(c->cands.p, 0, 16, c->stream));
        c->cands_zeroed = nullptr;
    }
    if (R.hash_mask) MTMC(c->chash.ensure(cand_hash_bytes(R.hash_mask)));
    if (R.prefetched) {
        const size_t fetch_bytes = 16 + sizeof(mtm_hit) * R.cand_pin_n;
        if (c->pinned_cap < fetch_bytes) {
            if (c->pinned) (void)hipHostFree(c->pinned);
            c->pinned = nullptr;
            c->pinned_cap = 0;
            HIPC(hipHostMalloc(&c->pinned, fetch_bytes, hipHostMallocDefault));
            c->pinned_cap = fetch_bytes;
        }
        if (R.cand_pin) {               // the window starts out as "no record" (template index -1) in every slot
            uint8_t* land = static_cast<uint8_t*>(c->pinned);
            std::memset(land, 0, 16);
            mtm_hit* w = reinterpret_cast<mtm_hit*>(land + 16);
            for (size_t i = 0; i < R.cand_pin_n; ++i) w[i].templ_idx = -1;
        }
    }
    host_trace(c, 3);
    // start of the GPU time of the call (timing.total_ms).  Banded: recorded by run_score_banded once the first band's
    // copy is on its way - nothing is queued ahead of that copy that does not have to be (every API call is 5-10 us)
    if (!banded) HIPC(hipEventRecord(c->ev[0], c->stream));
    if (banded) {
        const int rc = run_score_banded(c, R, *up);
        if (rc != MTM_OK) {
            c->have_image = false;                   // possibly half an image on the device
            (void)hipStreamSynchronize(c->copy_stream);
            return rc;
        }
    } else {
        MTMC(run_score_all(c, R));
    }
    HIPC(hipEventRecord(c->ev[1], c->stream));
    host_trace(c, 9);
    // (the first pass only: a re-run of the score pass lists no candidates unless its transition asks for them)
    R.cand_on = false;
    R.pin_direct = R.cand_pin;
    R.cand_pin = false;
    // stream mode: the kernels of this image are on their way - start the upload of the next one now.
    // (Not later: the device-to-host copy of the hit records below lands in pageable memory, which
    // the runtime executes synchronously, i.e. after the kernels.)
    MTMC(stage_next_image(c, next));
    if (R.prefetched) {
        // Few candidates (the usual case): they are in the pinned landing buffer when the stream is done and the 3x3 test
        // runs on the host (fm_end) - written there by the score kernel itself (pin_direct), else by a one-group kernel
        if (!R.pin_direct) MTMC(queue_cand_fetch(c->stream, c->cands.p, c->pinned, R.cand_pin_n));
        HIPC(hipEventRecord(c->ev[2], c->stream));
    }
    return MTM_OK;
}

// ---- The fallback ladder.  An overflowing list moves the call one step down (ladder_next, mtm_host.cpp): each transition
// below lowers the route (ladder_apply: a slower route, or a longer list), keeps the context's back-off in step and re-runs
// what the lowered route needs.
inline void back_off(int& counter, int& len) {      // the next `len` calls skip the route; the period doubles while they overflow
    counter = len;
    len = std::min(2 * len, 1024);
}

// re-runs the score pass on the lowered route
int rescore(mtm_ctx* c, CallRoute& R) {
    c->timing.ncc_launches = 0;
    c->timing.sq_launches = 0;
    MTMC(run_score_all(c, R));
    HIPC(hipEventRecord(c->ev[1], c->stream));
    return MTM_OK;
}

// float32 refinement, the ONE-PRODUCT screen listed more than the list holds: the same route with three piece products -
// bounds 2^8 times tighter - before anything slower is tried (and the next calls start there)
int to_three_products(mtm_ctx* c, CallRoute& R) {
    ladder_apply(R, LadderStep::ThreeProducts);
    back_off(c->np1_backoff, c->np1_backoff_len);
    HIPC(hipMemsetAsync(c->cands.p, 0, 16, c->stream));
    if (R.ext) HIPC(hipMemsetAsync(c->counters.p, 0, sizeof(unsigned long long) * 2 * std::max(1, R.n), c->stream));
    else if (R.hits_only) HIPC(hipMemsetAsync(c->chash.p, 0, cand_hash_key_bytes(R.hash_mask), c->stream));
    R.cand_on = true;
    MTMC(rescore(c, R));
    R.cand_on = false;
    return MTM_OK;
}

// float32 refinement, the kernel candidates (everything above the threshold) overflowed: the potential peaks of a map scan
// instead - far fewer
int to_map_scan(mtm_ctx* c, CallRoute& R) {
    ladder_apply(R, LadderStep::MapScan);
    back_off(c->fuse_backoff, c->backoff_len);
    HIPC(hipMemsetAsync(c->cands.p, 0, 16, c->stream));
    return rescore(c, R);
}

// float32: the float64 kernel decides, on maps in memory (the refined lists overflowed, or a bound is too wide for the map
// scan's tolerances)
int to_float64(mtm_ctx* c, CallRoute& R) {
    const bool raw_rig = R.raw_rig;
    ladder_apply(R, LadderStep::Float64);
    if (raw_rig) back_off(c->fuse_backoff, c->backoff_len);     // raw sums have no map-scan route: the next calls start here
    return rescore(c, R);
}

// dense maps, the candidate list overflowed: the next calls on this context go straight to map mode (dense route, or the
// full peak pass), this one takes the full peak pass.  (An overflow of the dense route's own list - row maxima only - is no
// retry: the back-off it runs under keeps counting down.)
int to_maps(mtm_ctx* c, CallRoute& R) {
    const bool maps_in_memory = !R.hits_only;
    ladder_apply(R, LadderStep::Maps);
    back_off(c->fuse_backoff, c->backoff_len);
    if (maps_in_memory) return MTM_OK;
    return rescore(c, R);               // no maps in memory: compute them (this call pays twice - the overflowed launch left early)
}

// the per-segment lists of the flagged route are bounded in total: if growing them did not help, the full scan with its single
// list takes over - the maps are complete unless the score pass left the unflagged segments out (then once more, in full:
// the maps may be published)
int leave_segments(mtm_ctx* c, CallRoute& R) {
    const bool maps_complete = !R.seg_skip_used;
    ladder_apply(R, LadderStep::GrowListLeaveSegments);
    return maps_complete ? MTM_OK : rescore(c, R);
}

// the step ladder_next named: its transition above, or - the pass found `count` peaks, more than the hit list holds - a list
// with room for them
int take_step(mtm_ctx* c, CallRoute& R, LadderStep step, unsigned long long count) {
    switch (step) {
        case LadderStep::Done: return MTM_OK;
        case LadderStep::ThreeProducts: return to_three_products(c, R);
        case LadderStep::MapScan: return to_map_scan(c, R);
        case LadderStep::Float64: return to_float64(c, R);
        case LadderStep::Maps: return to_maps(c, R);
        case LadderStep::GrowList:
        case LadderStep::GrowListLeaveSegments: break;
    }
    c->hit_cap = (int64_t)count + 1024;     // grow and rerun the compaction pass
    if (step == LadderStep::GrowListLeaveSegments) return leave_segments(c, R);
    ladder_apply(R, step);
    return MTM_OK;
}

// ---- fm_end, the synchronising half of a call, in stages.

// MTM_PEAKS_GLOBAL: the per-template extremum keys (from the score kernels' epilogue, or extremum_kernel over the maps) ->
// one record per template.  Passes: the first, then one per step down - three products, the float64 kernel (which lists
// nothing).
int collect_global_extremum(mtm_ctx* c, CallRoute& R, std::vector<mtm_hit>& hits) {
    const int n = R.n;
    const size_t key_bytes = sizeof(unsigned long long) * 2 * (size_t)std::max(1, n);
    std::vector<unsigned long long> best(2 * (size_t)std::max(1, n));
    bool done = false;
    for (int pass = 0; pass < 3 && !done; ++pass) {
        MTMC(queue_extremum_pass(c, R));
        HIPC(hipEventRecord(c->ev[2], c->stream));
        HIPC(hipMemcpyAsync(best.data(), c->counters.p, key_bytes, hipMemcpyDeviceToHost, c->stream));
        // refined: the outputs within the margin of their template's best are listed - more than the list holds?
        // ... or an output that cannot be screened at all (Bf16Params::nf_flag, the header's spare word)?
        unsigned long long hdr[2] = {0ull, 0ull};
        const bool refined = R.refine && R.ext;
        if (refined) HIPC(hipMemcpyAsync(hdr, c->cands.p, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        const unsigned long long nlisted = hdr[0];
        const bool not_finite = refined && (unsigned)hdr[1] != 0u;
        const LadderStep step = ladder_next(R, PassOutcome{not_finite, refined && (int64_t)nlisted > R.cand_cap, false}, pass);
        if (step == LadderStep::Done) {
            if (refined && R.bf16_np == 1) c->np1_backoff_len = 16;
            done = true;
        } else {
            MTMC(take_step(c, R, step, 0));
        }
    }
    if (!done) return ladder_exhausted();
    for (int t = 0; t < n; ++t) {
        const TemplDev& d = c->td_host[t];
        hits.push_back(decode_extremum_key(best[2 * t + (R.mode_min ? 1 : 0)], R.mode_min, t, d.ow, d.cols, d.rows));
    }
    return MTM_OK;
}

// Few candidates (the usual case): they are in the pinned landing buffer when the stream is done (fm_begin: R.prefetched)
// and the 3x3 test runs on the host (verify_candidates_3x3) - saves two kernels, three fills and a copy.  *verified: the
// whole list was in the window; `hits` / `tflags` hold the result.
int verify_on_host(mtm_ctx* c, CallRoute& R, std::vector<mtm_hit>& hits, int* tflags, bool* verified) {
    const size_t nfetch = R.cand_pin_n;
    HIPC(hipStreamSynchronize(c->stream));
    host_trace(c, 10);
    uint8_t* land = static_cast<uint8_t*>(c->pinned);
    unsigned long long ncand = 0;
    if (R.pin_direct) {
        // the window's slots fill from 0 upwards (every reserved slot below the capacity is written before the
        // launch ends): the count is the first slot that still says "no record"
        const mtm_hit* w = reinterpret_cast<const mtm_hit*>(land + 16);
        while (ncand < nfetch && w[ncand].templ_idx >= 0) ++ncand;
        if (ncand == nfetch) {      // window full: the list's real length is on the device (dense maps; rare)
            HIPC(hipMemcpyAsync(&ncand, c->cands.p, sizeof(ncand), hipMemcpyDeviceToHost, c->stream));
            HIPC(hipStreamSynchronize(c->stream));
        }
        std::memcpy(land, &ncand, sizeof(ncand));
    }
    std::memcpy(&ncand, land, sizeof(ncand));
    std::memcpy(&c->timing.sclk_mhz, land + 8, sizeof(float));
    if (ncand > nfetch) return MTM_OK;
    // everything needed is on the host: clear the counter for the next call while this one finishes
    // (unless this context's calls clear it in their own first kernel: banded uint8 calls)
    if (!R.banded_u8 && hipMemsetAsync(c->cands.p, 0, 16, c->stream) == hipSuccess) c->cands_zeroed = c->cands.p;
    const TemplDev* td = c->td_host.data();
    verify_candidates_3x3(reinterpret_cast<const mtm_hit*>(land + 16), (size_t)ncand, MapDims{&td->oh, &td->ow, sizeof(TemplDev)},
                          R.mode_min, R.mode_min ? -R.thr : R.thr, c->opt_border == MTM_BORDER_CONSTANT ? 0.0f : -INFINITY,
                          c->vh_keys, c->vh_vals, hits, tflags);
    *verified = true;
    if (R.refine && R.bf16_np == 1) c->np1_backoff_len = 16;
    return MTM_OK;
}

// skimage: a map in which every pixel equals its local maximum has no peaks at all (the scans' flag words, the candidate
// routes' peak counts: mtm_internal.h).  1-D / 1x1 maps: append_line_map_peaks.  tflags[t] becomes "t's records go".
void drop_trivial_maps(const mtm_ctx* c, const CallRoute& R, std::vector<int>& tflags, std::vector<mtm_hit>& hits) {
    if (hits.empty()) return;
    for (int t = 0; t < R.n; ++t) {
        const TemplDev& d = c->td_host[t];
        const int f = tflags[(size_t)t];
        tflags[(size_t)t] = d.oh <= 1 || d.ow <= 1 || (R.fused ? fused_count_trivial(f, d.oh, d.ow) : scan_flags_trivial((unsigned)f));
    }
    hits.erase(std::remove_if(hits.begin(), hits.end(), [&](const mtm_hit& h) { return tflags[(size_t)h.templ_idx] != 0; }),
               hits.end());
}

// 1x1 and 1-D maps (MTM/__init__.py:25-41) on the host.  The maps in memory are those of a stack of nb images of `rows`
// rows each (one image: nb = 1, rows = its rows); image b's records go to per_img[b].
int append_line_map_peaks(mtm_ctx* c, float thr, bool mode_min, int nb, int rows, std::vector<mtm_hit>* per_img) {
    for (int t = 0; t < (int)c->templs.size(); ++t) {
        const TemplDev& d = c->td_host[t];
        const int oh_b = rows - d.rows + 1;
        if (oh_b > 1 && d.ow > 1) continue;
        std::vector<float> mp((size_t)d.oh * d.ow);
        HIPC(hipMemcpy2DAsync(mp.data(), sizeof(float) * d.ow, c->maps.as<float>() + d.map_off, sizeof(float) * d.map_pitch,
                              sizeof(float) * d.ow, d.oh, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        for (int b = 0; b < nb; ++b)        // (a row, or a column of a one-column map)
            line_map_peaks(mp.data() + (size_t)b * rows * d.ow, oh_b, d.ow, thr, mode_min, t, d.cols, d.rows, per_img[b]);
    }
    return MTM_OK;
}

// deterministic order: template, then descending quality, then row-major position - or, with a suppression request, MTM.NMS'
// selection in its order; timing.n_hits = the peaks before that
void order_and_suppress(mtm_ctx* c, const CallRoute& R, std::vector<mtm_hit>& hits) {
    host_trace(c, 11);
    const bool mode_min = R.mode_min;
    // (the device may have pruned the list already - queue_device_nms / fetch_device_nms -: the count of peaks is the one before that)
    const int64_t n_raw = R.nms_raw_count >= 0 ? (int64_t)R.nms_raw_count : (int64_t)hits.size();
    if (R.nms.on && n_raw > 1) {                    // MTM.NMS (a list of one hit is returned as it is: MTM/NMS.py:53-55)
        const float thr_s = (float)(mode_min ? (1.0 - R.nms.score_threshold) : R.nms.score_threshold);
        std::vector<int32_t> keep;
        nms_select(hits.data(), (int64_t)hits.size(), mode_min ? 1 : 0, thr_s, (float)R.nms.max_overlap, keep,
                   R.nms_raw_count >= 0 ? R.nms_sure : 0);
        std::vector<mtm_hit> kept(keep.size());
        for (size_t i = 0; i < keep.size(); ++i) kept[i] = hits[(size_t)keep[i]];
        hits.swap(kept);
    } else {
        sort_hits(hits, mode_min);
    }
    if (R.nms.on && R.nms.n_object >= 0 && (long long)hits.size() > R.nms.n_object)
        hits.resize((size_t)R.nms.n_object);                // MTM/NMS.py:81-82
    c->timing.n_hits = n_raw;
    host_trace(c, 12);
}

// the call's GPU times from its three events (ev[2] is complete: every path synchronised the stream behind it)
int finish_call_timing(mtm_ctx* c) {
    HIPC(hipEventSynchronize(c->ev[2]));
    HIPC(hipEventElapsedTime(&c->timing.score_ms, c->ev[0], c->ev[1]));
    HIPC(hipEventElapsedTime(&c->timing.peaks_ms, c->ev[1], c->ev[2]));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[2]));
    return collect_ncc_time(c);
}

// Synchronising half: waits for the stream, verifies / extracts the peaks, delivers the hits.
int fm_end(mtm_ctx* c, CallRoute& R, mtm_hit* out, int64_t capacity, int64_t* n_out) {
    HIPC(hipSetDevice(c->device));
    std::vector<mtm_hit> hits;
    if (R.mode == MTM_PEAKS_GLOBAL) {
        MTMC(collect_global_extremum(c, R, hits));
    } else {
        // ---- 2-D maps.  Fused path: the score kernels appended every pixel above the threshold to the candidate list; the
        // 3x3 local maxima among them are hits.  If the list overflowed (dense maps), or on any class without candidates,
        // the peak pass scans the maps instead.
        const bool any2d = !c->list2d.empty();
        std::vector<int> tflags((size_t)std::max(1, R.n), 0);
        bool done = false;
        if (R.fused && any2d && !R.pp_mode) MTMC(verify_on_host(c, R, hits, tflags.data(), &done));
        if (!done && R.hits_only)
            HIPC(hipMemsetAsync(c->chash.p, 0, cand_hash_key_bytes(R.hash_mask), c->stream));
        if (R.pp_mode) R.fused = true;          // the potential peaks are in the candidate buffer, their neighbourhoods in the maps
        done = done || !any2d;
        HitBuffer hb(R.n);
        std::vector<uint8_t> host_buf;
        DeviceNms dnms;                 // (the device's share of a suppression request, queued behind the flagged-segment peak pass)
        // Passes: the first, then one per step down the ladder (ladder_next; tests/native/sanitize_host.cpp walks every
        // sequence the device can report: no step but a grown list twice, at most 5 passes).  A ladder that runs out is an
        // internal error, never an empty list.
        for (int attempt = 0; attempt < 5 && !done; ++attempt) {
            unsigned long long count = 0;
            PassOutcome outcome{};
            MTMC(queue_peak_pass(c, R, hb, &dnms));
            MTMC(fetch_pass_outcome(c, R, hb, host_buf, tflags.data(), &count, &outcome));
            const LadderStep step = ladder_next(R, outcome, attempt);
            const bool grow = step == LadderStep::GrowList || step == LadderStep::GrowListLeaveSegments;
            if ((step == LadderStep::Done || grow) && R.fused && !R.pp_mode) {      // the candidates fitted
                c->backoff_len = 16;
                if (R.refine && R.bf16_np == 1) c->np1_backoff_len = 16;
            }
            if (step == LadderStep::Done) {
                MTMC(fetch_peak_list(c, R, hb, host_buf, count, tflags.data(), dnms, hits));
                done = true;
            } else {
                MTMC(take_step(c, R, step, count));
            }
        }
        if (!done) return ladder_exhausted();
        if (!any2d) {
            HIPC(hipEventRecord(c->ev[2], c->stream));
            HIPC(hipStreamSynchronize(c->stream));
        }
        drop_trivial_maps(c, R, tflags, hits);
        MTMC(append_line_map_peaks(c, R.thr, R.mode_min, 1, c->rows, &hits));
        order_and_suppress(c, R, hits);
    }
    MTMC(finish_call_timing(c));
    if (R.mode != MTM_PEAKS_LOCAL || !R.nms.on) c->timing.n_hits = (int64_t)hits.size();
    // what the call's route came to
    c->timing.hits_only = R.sparse ? 2 : R.hits_only ? 1 : 0;
    c->timing.f32_route = R.mbf_used ? 4 : R.f32_exact ? 3 : !R.refine ? 0 : (R.refine_scan ? 2 : 1);
    c->maps_valid = !R.hits_only && !R.ext && !R.seg_skip_used && !R.mbf_used;
    return publish_hits(hits, c->last_hits, out, capacity, n_out,
                        "mtm_find_matches: output capacity too small (fetch the result with mtm_last_hits)");
}

int find_matches_impl(mtm_ctx* c, int mode, double score_threshold, mtm_hit* out, int64_t capacity,
                      int64_t* n_out, NextImage* next, const ImageArgs* up, const NmsRequest* nms) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !out) ||
        (mode != MTM_PEAKS_LOCAL && mode != MTM_PEAKS_GLOBAL)) {
        set_error("mtm_find_matches: bad arguments");
        return MTM_E_INVALID;
    }
    if (c->fm_in_flight) {
        set_error("mtm_find_matches: a mtm_find_matches_async call is in flight (collect it with mtm_find_matches_wait)");
        return MTM_E_INVALID;
    }
    CallRoute R;
    MTMC(fm_begin(c, mode, score_threshold, next, R, up));
    if (nms) R.nms = *nms;
    return fm_end(c, R, out, capacity, n_out);
}

// ---- mtm_find_matches_batch: n images of one shape as ONE tall image of n * rows rows (include/mtm_hip.h).  Map row y
// belongs to image b = y / rows; it is a window of that image when y % rows < rows - h + 1 and straddles a seam otherwise.

// Images per chunk: the row bound (MTM_OPT_BATCH_MAX_ROWS) and the device memory of the chunk - a float per template and
// pixel for the maps, the raw copy and the uint8 / int8 / float32 planes per channel, the window statistics.
int batch_chunk_images(const mtm_ctx* c, int rows, int cols, int chans) {
    const double pitch = (double)round_up((size_t)cols + kPadCols, 64);
    const double per_image = (double)rows * pitch * (4.0 * (double)c->templs.size() + 10.0 * chans + 48.0);
    const int by_rows = std::max(1, c->batch_max_rows / rows);
    const int by_mem = (int)std::max(1.0, std::min(1e9, kBatchChunkBytes / per_image));
    return std::min(by_rows, by_mem);
}

// Images px[0 .. nb) of the batch as one stack: upload, statistics and score launches over the whole stack (maps in memory),
// then the seam-aware peak pass (peaks_batch_kernel) or the per-image extremum (extremum_batch_kernel); 1-D / 1x1 per-image
// maps on the host.  Appends each image's records, ordered as fm_end orders them, to per_img[b].
int batch_chunk(mtm_ctx* c, const void* const* px, int nb, int rows, int cols, int chans, int dtype, int64_t stride, int mode,
                float thr, std::vector<mtm_hit>* per_img) {
    adopt_image(c, nb * rows, cols, chans, dtype);
    MTMC(place_templates(c));
    MTMC(upload_image_stack(c, c->slot[c->cur], px, nb, stride, rows, cols, chans, dtype, c->stream));
    c->timing = mtm_timing{};
    const int n = (int)c->templs.size();
    const bool mode_min = method_mode_min(c->method);
    // the map route: no candidate list, no fused extremum, no segment flags (each keeps one answer per template over the
    // whole launch, or packs stack rows where the seams need image rows)
    CallRoute R;
    R.mode = mode;
    R.n = n;
    R.thr = thr;
    R.mode_min = mode_min;
    HIPC(hipEventRecord(c->ev[0], c->stream));
    MTMC(run_score_all(c, R));
    HIPC(hipEventRecord(c->ev[1], c->stream));
    // the maps are in memory: the peak pass (mtm_peaks.hip) -> per-image records
    MTMC(batch_peak_pass(c, mode, thr, mode_min, nb, rows, per_img));
    if (mode != MTM_PEAKS_GLOBAL) {
        MTMC(append_line_map_peaks(c, thr, mode_min, nb, rows, per_img));
        for (int b = 0; b < nb; ++b) sort_hits(per_img[b], mode_min);
    }
    return finish_call_timing(c);
}

}  // namespace

namespace mtmi {

int ladder_exhausted() {
    set_error("mtm_find_matches: internal state (the overflow fallbacks ran out of passes)");
    return MTM_E_STATE;
}

}  // namespace mtmi

extern "C" {

int mtm_score_map(mtm_ctx* c, int templ_idx, float* out, int64_t out_row_stride_bytes) {
    if (!c || !out) {
        set_error("mtm_score_map: bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_score_map");
    HIPC(hipSetDevice(c->device));
    MTMC(place_templates(c));
    if (templ_idx < 0 || templ_idx >= (int)c->templs.size()) {
        set_error("mtm_score_map: template index out of range");
        return MTM_E_INVALID;
    }
    const TemplDev& d = c->td_host[templ_idx];
    if (out_row_stride_bytes < (int64_t)(sizeof(float) * d.ow)) {
        set_error("mtm_score_map: output row stride too small");
        return MTM_E_INVALID;
    }
    const SizeClass& sc = c->classes[c->templs[templ_idx].cls];
    // position of the template inside its class list
    int pos = 0;
    while (sc.members[pos] != templ_idx) ++pos;
    c->timing = mtm_timing{};
    StatPlanes st;
    MTMC(ensure_maps(c));
    // a map-mode route: no candidates, no extremum; float32 classes take the maps of the raw-sum methods from the float64
    // kernel (plan_call)
    CallRoute R;
    R.f32_exact = sc.kernel == MTM_KERNEL_MFMA_F32 &&
                  (c->method == MTM_TM_SQDIFF || c->method == MTM_TM_CCORR || c->method == MTM_TM_CCOEFF);
    MTMC(launch_stats(c, R, sc, &st));
    MTMC(launch_ncc(c, R, sc, sc.tlist_off + pos, 1, st, pos));
    HIPC(hipMemcpy2DAsync(out, (size_t)out_row_stride_bytes, c->maps.as<float>() + d.map_off,
                          sizeof(float) * d.map_pitch, sizeof(float) * d.ow, d.oh, hipMemcpyDeviceToHost,
                          c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    MTMC(collect_ncc_time(c));
    return MTM_OK;
}

int mtm_find_matches(mtm_ctx* c, int mode, double score_threshold, mtm_hit* out, int64_t capacity,
                     int64_t* n_out) {
    return find_matches_impl(c, mode, score_threshold, out, capacity, n_out, nullptr);
}

int mtm_find_matches_image(mtm_ctx* c, const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                           int mode, double score_threshold, mtm_hit* out, int64_t capacity, int64_t* n_out) {
    if (!c) {
        set_error("mtm_find_matches_image: null context");
        return MTM_E_INVALID;
    }
    host_trace(c, 0);
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, "mtm_find_matches_image"));
    const ImageArgs up{px, rows, cols, chans, dtype, row_stride_bytes};
    const int rc = find_matches_impl(c, mode, score_threshold, out, capacity, n_out, nullptr, &up);
    host_trace(c, 15);
    return rc;
}

int mtm_find_matches_image_nms(mtm_ctx* c, const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                               double score_threshold, double max_overlap, int64_t n_object, mtm_hit* out, int64_t capacity,
                               int64_t* n_out) {
    if (!c) {
        set_error("mtm_find_matches_image_nms: null context");
        return MTM_E_INVALID;
    }
    host_trace(c, 0);
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, "mtm_find_matches_image_nms"));
    const ImageArgs up{px, rows, cols, chans, dtype, row_stride_bytes};
    const NmsRequest nms{true, score_threshold, max_overlap, n_object};
    const int rc = find_matches_impl(c, MTM_PEAKS_LOCAL, score_threshold, out, capacity, n_out, nullptr, &up, &nms);
    host_trace(c, 15);
    return rc;
}

// One step of the process-per-GPU form in ONE native call (round 5): this rank's shard is searched, its hits get their list
// positions in the caller's whole template list (global_idx), the ranks' lists are exchanged (mtm_comm_allgather_hits: the
// context's communicator; none / one rank: no exchange), merged in template order and suppressed - every rank returns
// the same kept hits.  What MTM.distributed.matchTemplates_sharded did in four steps from Python (search, remap,
// all-gather, mtm_nms) with the reference's fan-in (MTM/__init__.py:173-177) and MTM/NMS.py:53-84 behind it.
int mtm_find_matches_image_sharded_nms(mtm_ctx* c, const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                                       double score_threshold, double max_overlap, int64_t n_object, int method,
                                       const int32_t* global_idx, int n_local_templ, mtm_hit* out, int64_t capacity,
                                       int64_t* n_out) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !out) || n_local_templ < 0 || (n_local_templ > 0 && !global_idx)) {
        set_error("mtm_find_matches_image_sharded_nms: bad arguments");
        return MTM_E_INVALID;
    }
    // This is a COLLECTIVE: whatever goes wrong on this rank before the exchange (arguments that differ per rank, a bad
    // image, a HIP error in the search) must not keep it away from the all-gather - the other ranks would wait in it without
    // a time-out of their own.  A failing rank joins with zero hits and its error code in the slot header; every rank then
    // returns an error (this one its own, the others MTM_E_COMM naming the rank) instead of a list with hits missing.
    std::vector<mtm_hit> local;
    int local_rc = MTM_OK;
    std::string local_msg;
    if (n_local_templ > 0) {                    // (a rank without units still takes part in the exchange)
        if ((int)c->templs.size() != n_local_templ || c->method != method) {
            set_error("mtm_find_matches_image_sharded_nms: global_idx / method do not match the context's template set");
            local_rc = MTM_E_INVALID;
        }
        host_trace(c, 0);
        if (local_rc == MTM_OK)
            local_rc = check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, "mtm_find_matches_image_sharded_nms");
        if (local_rc == MTM_OK) {
            const ImageArgs up{px, rows, cols, chans, dtype, row_stride_bytes};
            int64_t n = 0;
            const int rc = find_matches_impl(c, MTM_PEAKS_LOCAL, score_threshold, nullptr, 0, &n, nullptr, &up);
            if (rc != MTM_OK && rc != MTM_E_OVERFLOW) local_rc = rc;
        }
        if (local_rc == MTM_OK) {
            local = c->last_hits;               // (find_matches_impl keeps the whole list there whatever the capacity)
            for (mtm_hit& h : local) h.templ_idx = global_idx[h.templ_idx];
        } else {
            local_msg = mtm_last_error();
        }
    }
    std::vector<mtm_hit> all;
    if (c->comm && c->n_ranks > 1) {
        std::vector<int64_t> counts((size_t)c->n_ranks, 0);
        std::vector<int32_t> flags;
        int64_t n_all = 0;
        all.resize(std::max<size_t>(4096, local.size() * (size_t)c->n_ranks));
        int rc = comm_allgather_hits_flagged(c, local.data(), (int64_t)local.size(), (int32_t)local_rc, all.data(), (int64_t)all.size(),
                                             counts.data(), &n_all, &flags);
        if (rc == MTM_E_OVERFLOW) {             // (a local matter: the gathered slots are still in the staging area)
            all.resize((size_t)n_all);
            rc = mtm_comm_last_gather(c, all.data(), n_all, counts.data(), &n_all);
        }
        if (local_rc != MTM_OK) {               // this rank's own failure: its message, its code (the exchange has been served)
            set_error(local_msg);
            return local_rc;
        }
        if (rc != MTM_OK) return rc;
        for (size_t r = 0; r < flags.size(); ++r)
            if (flags[r] != 0) {
                set_error("mtm_find_matches_image_sharded_nms: rank " + std::to_string(r) + " failed its local search (code " +
                          std::to_string(flags[r]) + "); no list is returned");
                return MTM_E_COMM;
            }
        all.resize((size_t)n_all);
    } else {
        if (local_rc != MTM_OK) {
            set_error(local_msg);
            return local_rc;
        }
        all.swap(local);
    }
    std::stable_sort(all.begin(), all.end(), [](const mtm_hit& a, const mtm_hit& b) { return a.templ_idx < b.templ_idx; });
    const bool ascending = method_mode_min(method);
    if (all.size() > 1) {                       // (MTM/NMS.py:53-55: a list of one hit is returned as it is)
        const float thr_s = (float)(ascending ? (1.0 - score_threshold) : score_threshold);
        std::vector<int32_t> keep;
        nms_select(all.data(), (int64_t)all.size(), ascending ? 1 : 0, thr_s, (float)max_overlap, keep);
        std::vector<mtm_hit> kept(keep.size());
        for (size_t i = 0; i < keep.size(); ++i) kept[i] = all[(size_t)keep[i]];
        all.swap(kept);
    }
    if (n_object >= 0 && (int64_t)all.size() > n_object) all.resize((size_t)n_object);
    return publish_hits(all, c->last_hits, out, capacity, n_out,
                        "mtm_find_matches_image_sharded_nms: output capacity too small (fetch the result with mtm_last_hits)");
}

int mtm_find_matches_next(mtm_ctx* c, int mode, double score_threshold, mtm_hit* out, int64_t capacity,
                          int64_t* n_out, const void* next_px, int rows, int cols, int chans, int dtype,
                          int64_t row_stride_bytes) {
    if (!c) {
        set_error("mtm_find_matches_next: null context");
        return MTM_E_INVALID;
    }
    MTMC(check_image_args(next_px, rows, cols, chans, dtype, row_stride_bytes, "mtm_find_matches_next"));
    NextImage nx{next_px, rows, cols, chans, dtype, row_stride_bytes, false};
    const int rc = find_matches_impl(c, mode, score_threshold, out, capacity, n_out, &nx);
    if (rc != MTM_OK && rc != MTM_E_OVERFLOW) {
        if (nx.staged) (void)hipStreamSynchronize(c->copy_stream);   // drop the staged image
        return rc;
    }
    // the results of the current image are final: make the staged image current
    if (!nx.staged) MTMC(stage_next_image(c, &nx));
    HIPC(hipEventSynchronize(c->next_ready));
    c->cur = 1 - c->cur;
    adopt_image(c, rows, cols, chans, dtype);
    return rc;
}

int mtm_find_matches_batch(mtm_ctx* c, const void* const* images, int n_images, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, int mode, double score_threshold, mtm_hit* out, int64_t capacity,
                           int64_t* counts, int64_t* n_out) {
    if (!c || !n_out || n_images < 0 || (n_images > 0 && (!images || !counts)) || capacity < 0 || (capacity > 0 && !out) ||
        (mode != MTM_PEAKS_LOCAL && mode != MTM_PEAKS_GLOBAL)) {
        set_error("mtm_find_matches_batch: bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_find_matches_batch");
    if (dtype == MTM_F32) {
        set_error("mtm_find_matches_batch: uint8 and uint16 images only (float32: mtm_find_matches_image per image)");
        return MTM_E_INVALID;
    }
    *n_out = 0;
    if (n_images == 0) return MTM_OK;
    for (int b = 0; b < n_images; ++b)
        MTMC(check_image_args(images[b], rows, cols, chans, dtype, row_stride_bytes, "mtm_find_matches_batch"));
    if (!c->have_templ) {
        set_error("mtm_find_matches_batch: set the templates first");
        return MTM_E_STATE;
    }
    for (const HostTempl& t : c->templs)
        if (t.rows > rows || t.cols > cols) {        // (the stack would hide it: a template taller than one image fits it)
            set_error("mtm_find_matches_batch: a template is larger than the images");
            return MTM_E_INVALID;
        }
    HIPC(hipSetDevice(c->device));
    const int per_chunk = batch_chunk_images(c, rows, cols, chans);
    std::vector<std::vector<mtm_hit>> per_img((size_t)n_images);
    mtm_timing acc{};
    int rc = MTM_OK;
    for (int b0 = 0; b0 < n_images && rc == MTM_OK; b0 += per_chunk) {
        const int nb = std::min(per_chunk, n_images - b0);
        rc = batch_chunk(c, images + b0, nb, rows, cols, chans, dtype, row_stride_bytes, mode, (float)score_threshold,
                         per_img.data() + b0);
        acc.total_ms += c->timing.total_ms;
        acc.score_ms += c->timing.score_ms;
        acc.peaks_ms += c->timing.peaks_ms;
        acc.ncc_kernel_ms += c->timing.ncc_kernel_ms;
        acc.ncc_sum_ms += c->timing.ncc_sum_ms;
        acc.ncc_launches += c->timing.ncc_launches;
        acc.sq_launches += c->timing.sq_launches;
        acc.masked_stat_ms += c->timing.masked_stat_ms;
        acc.kernel_used = c->timing.kernel_used;
        acc.sclk_mhz = c->timing.sclk_mhz;
    }
    // the stack is none of the caller's images: no current image, no published maps
    c->have_image = false;
    c->maps_valid = false;
    if (rc != MTM_OK) return rc;
    std::vector<mtm_hit> all;
    for (int b = 0; b < n_images; ++b) {
        counts[b] = (int64_t)per_img[(size_t)b].size();
        all.insert(all.end(), per_img[(size_t)b].begin(), per_img[(size_t)b].end());
    }
    acc.n_hits = (int64_t)all.size();
    c->timing = acc;
    return publish_hits(all, c->last_hits, out, capacity, n_out,
                        "mtm_find_matches_batch: output capacity too small (fetch the result with mtm_last_hits)");
}

int mtm_last_hits(mtm_ctx* c, mtm_hit* out, int64_t capacity, int64_t* n_out) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !out)) {
        set_error("mtm_last_hits: bad arguments");
        return MTM_E_INVALID;
    }
    return copy_out_hits(c->last_hits, out, capacity, n_out, "mtm_last_hits: output capacity too small");
}

int mtm_last_score_map(mtm_ctx* c, int templ_idx, float* out, int64_t out_row_stride_bytes) {
    if (!c || !out) {
        set_error("mtm_last_score_map: bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_last_score_map");
    if (!c->placed || !c->maps_valid) {
        set_error("mtm_last_score_map: the last mtm_find_matches did not materialise the score maps "
                  "(MTM_OPT_HITS_ONLY = 0 makes it), or the inputs changed since");
        return MTM_E_STATE;
    }
    if (templ_idx < 0 || templ_idx >= (int)c->templs.size()) {
        set_error("mtm_last_score_map: template index out of range");
        return MTM_E_INVALID;
    }
    const TemplDev& d = c->td_host[templ_idx];
    if (out_row_stride_bytes < (int64_t)(sizeof(float) * d.ow)) {
        set_error("mtm_last_score_map: output row stride too small");
        return MTM_E_INVALID;
    }
    HIPC(hipSetDevice(c->device));
    HIPC(hipMemcpy2DAsync(out, (size_t)out_row_stride_bytes, c->maps.as<float>() + d.map_off, sizeof(float) * d.map_pitch,
                          sizeof(float) * d.ow, d.oh, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return MTM_OK;
}

int mtm_find_matches_async(mtm_ctx* c, int mode, double score_threshold) {
    if (!c || (mode != MTM_PEAKS_LOCAL && mode != MTM_PEAKS_GLOBAL)) {
        set_error("mtm_find_matches_async: bad arguments");
        return MTM_E_INVALID;
    }
    if (c->fm_in_flight) {
        set_error("mtm_find_matches_async: a call is already in flight (collect it with mtm_find_matches_wait)");
        return MTM_E_INVALID;
    }
    MTMC(fm_begin(c, mode, score_threshold, nullptr, c->fm));
    c->fm_in_flight = true;
    return MTM_OK;
}

int mtm_find_matches_wait(mtm_ctx* c, mtm_hit* out, int64_t capacity, int64_t* n_out) {
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !out)) {
        set_error("mtm_find_matches_wait: bad arguments");
        return MTM_E_INVALID;
    }
    if (!c->fm_in_flight) {
        set_error("mtm_find_matches_wait: no call in flight");
        return MTM_E_INVALID;
    }
    c->fm_in_flight = false;
    return fm_end(c, c->fm, out, capacity, n_out);
}

int mtm_get_timing(mtm_ctx* c, mtm_timing* out) {
    if (!c || !out) return MTM_E_INVALID;
    *out = c->timing;
    return MTM_OK;
}

// ---------------------------------------------------------------------------------------------
// RCCL hit exchange.  librccl is loaded lazily so that the library itself has no link-time
// dependency on it (single-GPU users never touch it).
// ---------------------------------------------------------------------------------------------
}  // extern "C"
