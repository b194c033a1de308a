// libmtm_hip.so - the host side of the peak pass: one launcher per route of mtm_k_peaks.hip.h, the device's share of the
// non-maxima suppression (mtm_k_nms.hip.h), and their callers - the search calls' peak pass (queue_peak_pass and its
// fetches, the extremum pass, the batch pass, the candidate fetch), the window searches' pass (window_peak_pass) and the
// two test-support entries (mtm_debug_peak_pass, mtm_debug_device_nms).  The only unit that launches these kernels: a
// search and the test entry run the same launch code.
#include "mtm_ctx.h"

using namespace mtm;
using namespace mtmi;
#include "mtm_k_peaks.hip.h"
#include "mtm_k_nms.hip.h"

namespace {

// ---- The launchers.  Each takes a stream and device pointers - the context's buffers or the test entry's arena -, derives
// its grid and capacities from mtm_peak_sizing.h, queues the kernels of its route and returns what it derived.  Allocation,
// memsets, copies and the hipGetLastError behind a group of launches stay with the caller.

// the score maps under a pass: `n` maps td[tlist[0 .. n)], the largest height and width among them
struct PeakMaps {
    const float* maps;
    const TemplDev* td;
    const int* tlist;
    int n, max_oh, max_ow;
};
// what is a peak: maxima of the map or (mode_min) of its negation, above `thr` - the scans compare the score with the call's
// threshold, the verifiers a candidate's quality (score, or -score for minima) with the threshold's quality
struct PeakRule {
    bool mode_min;
    float thr;
    int border;
};
// where the peaks go: `cap` records, their count, one int per map (the scans' flag words, the verifiers' peak counts)
struct PeakList {
    mtm_hit* records;
    unsigned long long cap;
    unsigned long long* count;
    int* ints;
};

// grid of the peak scans: strips of 4 * strip_rows rows x kPkCols columns over the largest map, one layer per map
PeakGrid scan_grid(const PeakMaps& m, int strip_rows) { return peak_grid_dims(m.max_oh, m.max_ow, m.n, strip_rows); }
dim3 dim3_of(const PeakGrid& g) { return dim3(g.x, g.y, g.z); }

PeakGrid queue_scan(hipStream_t s, const PeakMaps& m, const PeakRule& r, const PeakList& l) {
    const PeakGrid g = scan_grid(m, kPkRows);
    hipLaunchKernelGGL(peaks_kernel, dim3_of(g), dim3(256), 0, s, m.maps, m.td, m.tlist, r.mode_min ? 1 : 0, r.thr, r.border,
                       l.records, l.cap, l.count, l.ints);
    return g;
}

// the maps are those of a stack of images of img_rows rows each; l.ints: one per (image, template of the n_templ placed)
PeakGrid queue_scan_batch(hipStream_t s, const PeakMaps& m, const PeakRule& r, const PeakList& l, int img_rows, int n_templ) {
    const PeakGrid g = scan_grid(m, kPkRows);
    hipLaunchKernelGGL(peaks_batch_kernel, dim3_of(g), dim3(256), 0, s, m.maps, m.td, m.tlist, r.mode_min ? 1 : 0, r.thr, r.border,
                       l.records, l.cap, l.count, l.ints, img_rows, n_templ);
    return g;
}

// The flagged-segment scan keeps a list per (map, strip column) (at most 64 MB of them) and their counters, then compacts
// them into one list for the host: [counters, cnt_bytes][n_lists lists of cap_t records, list_bytes].
struct SegLists {
    PeakGrid grid{};
    unsigned long long n_lists = 0, cap_t = 0;
    size_t cnt_bytes = 0, list_bytes = 0;
};
SegLists segment_lists(const PeakMaps& m, unsigned long long hit_cap) {
    SegLists sl;
    sl.grid = scan_grid(m, kPkSparseRows);
    sl.n_lists = (unsigned long long)sl.grid.z * sl.grid.x;
    sl.cap_t = peak_list_cap(hit_cap, sl.n_lists);
    sl.cnt_bytes = round_up(sizeof(unsigned long long) * (size_t)sl.n_lists, 256);
    sl.list_bytes = sizeof(mtm_hit) * (size_t)sl.cap_t * (size_t)sl.n_lists;
    return sl;
}
// the flags as the score kernel wrote them (the strides are its: CallRoute::flag_tstride / flag_rstride); holes: the
// unflagged segments of the maps were never written
struct SegFlags {
    const uint8_t* flags;
    int tstride, rstride;
    bool holes;
};
// sl = segment_lists(m, l.cap); counts_t cleared by the caller
void queue_segments(hipStream_t s, const PeakMaps& m, const PeakRule& r, const PeakList& l, const SegLists& sl,
                    unsigned long long* counts_t, mtm_hit* hits_t, const SegFlags& f) {
    hipLaunchKernelGGL(peaks_sparse_kernel, dim3_of(sl.grid), dim3(256), 0, s, m.maps, m.td, m.tlist, r.mode_min ? 1 : 0, r.thr,
                       r.border, hits_t, sl.cap_t, counts_t, l.ints, f.flags, f.tstride, f.rstride, f.holes ? 1 : 0);
    hipLaunchKernelGGL(compact_hits_kernel, dim3((unsigned)sl.n_lists), dim3(256), 0, s, hits_t, sl.cap_t, counts_t, (int)sl.n_lists,
                       l.records, l.cap, l.count);
}

// The candidate list [count | spare][records] of capacity cand_cap, verified against the maps - or, hash_keys given, against
// the hash table of its own positions (mask + 1 slots, the mask as plan_call set it; keys cleared by the caller, the values
// behind them).  r.thr: the quality a hit exceeds.  -> work-groups of each launch (one thread per candidate: a list grown
// past the candidate capacity only adds idle ones).
unsigned queue_verify(hipStream_t s, const PeakMaps& m, const PeakRule& r, const PeakList& l, const unsigned long long* cand_hdr,
                      unsigned long long cand_cap, unsigned long long* hash_keys, unsigned hash_mask) {
    const unsigned blocks = verify_blocks((long long)std::max(l.cap, cand_cap));
    const mtm_hit* cands = reinterpret_cast<const mtm_hit*>(cand_hdr + 2);
    if (hash_keys) {
        int* vals = reinterpret_cast<int*>(hash_keys + (size_t)hash_mask + 1);
        hipLaunchKernelGGL(cand_hash_insert_kernel, dim3(blocks), dim3(256), 0, s, cands, cand_hdr, cand_cap, hash_keys, vals,
                           hash_mask);
        hipLaunchKernelGGL(verify_hash_kernel, dim3(blocks), dim3(256), 0, s, m.td, r.mode_min ? 1 : 0, r.border, cands, cand_hdr,
                           cand_cap, hash_keys, vals, hash_mask, l.records, l.cap, l.count, l.ints, r.thr);
    } else {
        hipLaunchKernelGGL(verify_peaks_kernel, dim3(blocks), dim3(256), 0, s, m.maps, m.td, r.mode_min ? 1 : 0, r.border, cands,
                           cand_hdr, cand_cap, l.records, l.cap, l.count, l.ints, r.thr);
    }
    return blocks;
}

// the extremum keys (maximum, minimum) of the n maps of td -> keys (cleared by the caller); -> work-groups per map
int queue_extremum(hipStream_t s, const float* maps, const TemplDev* td, int n, unsigned long long* keys) {
    const int nb = extremum_blocks();
    hipLaunchKernelGGL(extremum_kernel, dim3(nb, n), dim3(256), 0, s, maps, td, nb, keys);
    return nb;
}
// ... per image of a stack of n_img images of img_rows rows; max_px: the most outputs one image has in one map
int queue_extremum_batch(hipStream_t s, const float* maps, const TemplDev* td, int n, int img_rows, int n_img, long long max_px,
                         unsigned long long* keys) {
    const int nb = extremum_batch_blocks(max_px);
    hipLaunchKernelGGL(extremum_batch_kernel, dim3(nb, n, n_img), dim3(256), 0, s, maps, td, img_rows, nb, keys);
    return nb;
}

// the 2-D maps of the context's placed templates
PeakMaps ctx_maps(const mtm_ctx* c) {
    PeakMaps m{c->maps.as<float>(), c->td.as<TemplDev>(), c->tlist.as<int>() + c->list2d_off, (int)c->list2d.size(), 0, 0};
    for (int t : c->list2d) {
        m.max_oh = std::max(m.max_oh, c->td_host[t].oh);
        m.max_ow = std::max(m.max_ow, c->td_host[t].ow);
    }
    return m;
}

// Lays out nms_buf and queues the chain - two memsets, the five launches, the copy of the two counters - for the list of
// *dcount records at `dhits` (both on the device); reads nothing else of the call from the context.  n_max sizes the buffers
// and the launches; a count outside [n_min, n_max] makes every kernel return at once.
int queue_nms_chain(mtm_ctx* c, const mtm_hit* dhits, const unsigned long long* dcount, unsigned n_min, size_t n_max, bool ascending,
                    float thr_score, float thr_overlap, const NmsGrid& g, DeviceNms* q) {
    NmsParams p{};
    p.hits = dhits;
    p.n_ptr = dcount;
    p.n_min = n_min;
    p.n_max = (unsigned)n_max;
    p.ascending = ascending ? 1 : 0;
    p.thr_score = thr_score;
    p.thr_overlap = thr_overlap;
    p.cell = g.cell;
    p.gw = g.gw;
    p.gh = g.gh;
    const size_t n_cells = (size_t)p.gw * p.gh;
    const size_t off_rank = round_up(sizeof(unsigned) * (n_cells + 1), 256), off_status = off_rank + round_up(sizeof(unsigned) * n_max, 256);
    const size_t off_sorted = off_status + round_up(sizeof(int) * n_max, 256);
    const size_t off_hdr = off_sorted + round_up(sizeof(mtm_hit) * n_max, 256), off_out = off_hdr + 256;
    MTMC(c->nms_buf.ensure(off_out + sizeof(mtm_hit) * n_max));
    uint8_t* b = c->nms_buf.as<uint8_t>();
    p.cell_cnt = reinterpret_cast<unsigned*>(b);
    p.rank = reinterpret_cast<unsigned*>(b + off_rank);
    p.status = reinterpret_cast<int*>(b + off_status);
    p.sorted = reinterpret_cast<mtm_hit*>(b + off_sorted);
    p.out_count = reinterpret_cast<unsigned long long*>(b + off_hdr);
    p.out = reinterpret_cast<mtm_hit*>(b + off_out);
    HIPC(hipMemsetAsync(p.cell_cnt, 0, sizeof(unsigned) * (n_cells + 1), c->stream));
    HIPC(hipMemsetAsync(b + off_hdr, 0, 16, c->stream));
    const unsigned blocks = (unsigned)((n_max + 255) / 256);
    hipLaunchKernelGGL(nms_count_kernel, dim3(blocks), dim3(256), 0, c->stream, p);
    hipLaunchKernelGGL(nms_offsets_kernel, dim3(1), dim3(1024), 0, c->stream, p);
    hipLaunchKernelGGL(nms_scatter_kernel, dim3(blocks), dim3(256), 0, c->stream, p);
    hipLaunchKernelGGL(nms_champion_kernel, dim3(blocks), dim3(256), 0, c->stream, p);
    hipLaunchKernelGGL(nms_prune_kernel, dim3(blocks), dim3(256), 0, c->stream, p);
    HIPC(hipGetLastError());
    // (into page-locked memory: a device-to-host copy into a pageable stack slot may hold the host until the whole peak pass
    // is done - the round trip this queueing exists to avoid)
    if (!c->pin_small) HIPC(hipHostMalloc(&c->pin_small, 64, hipHostMallocDefault));
    q->cnt_pin = static_cast<unsigned long long*>(c->pin_small);
    HIPC(hipMemcpyAsync(c->pin_small, b + off_hdr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    q->queued = true;
    q->n_max = (unsigned)n_max;
    q->out = p.out;
    return MTM_OK;
}

// the production call: the grid of the context's image and templates (mtm_nms_core.h: nms_grid), lists of nms_device_min ..
// min(hit capacity, 2^18) peaks
int queue_device_nms(mtm_ctx* c, const NmsRequest& req, const mtm_hit* dhits, const unsigned long long* dcount, bool ascending, DeviceNms* q) {
    int max_side = 0;
    for (const TemplDev& d : c->td_host) max_side = std::max(max_side, std::max(d.rows, d.cols));
    const size_t n_max = (size_t)std::min<int64_t>(c->hit_cap, 1ll << 18);
    // MTM/NMS.py:73-78: the scores are float32 (1 - score for the difference methods), the threshold a python float
    // transformed in double and narrowed by the cv2 binding
    const float thr_score = (float)(ascending ? (1.0 - req.score_threshold) : req.score_threshold);
    return queue_nms_chain(c, dhits, dcount, (unsigned)std::min<long long>(c->nms_device_min, 1ll << 30), n_max, ascending, thr_score,
                           (float)req.max_overlap, nms_grid(c->rows, c->cols, max_side), q);
}

// after the stream was synchronised (q.cnt_pin has landed): the pruned list of `count` peaks -> `rest`, *n_sure = champions
int fetch_device_nms(mtm_ctx* c, const DeviceNms& q, unsigned long long count, std::vector<mtm_hit>& rest, long long* n_sure) {
    const unsigned long long n_champ = q.cnt_pin ? q.cnt_pin[0] : 0ull, n_undecided = q.cnt_pin ? q.cnt_pin[1] : 0ull;
    if (n_champ + n_undecided > count) {
        set_error("mtm_find_matches_image_nms: internal state (pruned list longer than the peak list)");
        return MTM_E_STATE;
    }
    if (c->host_trace && c->trace_calls <= 12)
        std::fprintf(stderr, "[mtm host trace] device NMS: %llu peaks -> %llu champions + %llu for the host's pass\n", count,
                     n_champ, n_undecided);
    rest.resize((size_t)(n_champ + n_undecided));
    if (n_champ) HIPC(hipMemcpyAsync(rest.data(), q.out, sizeof(mtm_hit) * (size_t)n_champ, hipMemcpyDeviceToHost, c->stream));
    if (n_undecided)
        HIPC(hipMemcpyAsync(rest.data() + n_champ, q.out + (count - n_undecided), sizeof(mtm_hit) * (size_t)n_undecided,
                            hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    *n_sure = (long long)n_champ;
    return MTM_OK;
}

}  // namespace

namespace mtmi {

int queue_cand_fetch(hipStream_t stream, const void* cands, void* pinned, size_t max_records) {
    hipLaunchKernelGGL(fetch_cands_kernel, dim3(1), dim3(256), 0, stream, static_cast<const uint4*>(cands), static_cast<uint4*>(pinned),
                       (unsigned long long)max_records);
    HIPC(hipGetLastError());
    return MTM_OK;
}

int queue_peak_pass(mtm_ctx* c, const CallRoute& R, HitBuffer& hb, DeviceNms* dnms) {
    *dnms = DeviceNms{};
    MTMC(c->hits.ensure(hb.hdr_bytes + sizeof(mtm_hit) * (size_t)c->hit_cap));
    hb.base = c->hits.as<uint8_t>();
    HIPC(hipMemsetAsync(hb.base, 0, hb.hdr_bytes, c->stream));
    const PeakMaps m = ctx_maps(c);
    const PeakRule scan{R.mode_min, R.thr, c->opt_border};
    const PeakList list{hb.records(), (unsigned long long)c->hit_cap, hb.count(), hb.flags()};
    if (R.fused) {
        // the candidate count (for the overflow check on the host) and the spare word
        HIPC(hipMemcpyAsync(hb.cand_header(), c->cands.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
        // a hit's quality (score, or -score for minima) exceeds the threshold's
        queue_verify(c->stream, m, PeakRule{R.mode_min, R.mode_min ? -R.thr : R.thr, c->opt_border}, list,
                     c->cands.as<unsigned long long>(), (unsigned long long)R.cand_cap,
                     R.hits_only ? c->chash.as<unsigned long long>() : nullptr, R.hash_mask);
    } else if (R.sparse) {
        const SegLists sl = segment_lists(m, list.cap);
        MTMC(c->hits_t.ensure(sl.cnt_bytes + sl.list_bytes));
        unsigned long long* counts_t = c->hits_t.as<unsigned long long>();
        HIPC(hipMemsetAsync(counts_t, 0, sl.cnt_bytes, c->stream));
        queue_segments(c->stream, m, scan, list, sl, counts_t, reinterpret_cast<mtm_hit*>(c->hits_t.as<uint8_t>() + sl.cnt_bytes),
                       SegFlags{c->seg_flags.as<uint8_t>(), R.flag_tstride, R.flag_rstride, R.seg_skip_used});
        // a suppression request: its device share follows at once (it reads the list's length on the device)
        if (R.nms.on && R.nms.max_overlap >= 0.0) MTMC(queue_device_nms(c, R.nms, hb.records(), hb.count(), R.mode_min, dnms));
    } else {
        queue_scan(c->stream, m, scan, list);
    }
    HIPC(hipGetLastError());
    return MTM_OK;
}

int fetch_pass_outcome(mtm_ctx* c, const CallRoute& R, const HitBuffer& hb, std::vector<uint8_t>& host_buf, int* tflags,
                       unsigned long long* count, PassOutcome* o) {
    HIPC(hipEventRecord(c->ev[2], c->stream));
    host_buf.resize(hb.hdr_bytes + sizeof(mtm_hit) * std::min<size_t>(kHitPrefetch, (size_t)c->hit_cap));
    HIPC(hipMemcpyAsync(host_buf.data(), hb.base, host_buf.size(), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    const HitBuffer::Header h = hb.decode(host_buf.data(), R.n, tflags);
    *count = h.count;
    o->rig_wide = R.fused && h.rig_wide != 0;
    o->cands_overflow = R.fused && (int64_t)h.ncand > R.cand_cap;
    o->hits_overflow = (int64_t)h.count > c->hit_cap;
    return MTM_OK;
}

int fetch_peak_list(mtm_ctx* c, CallRoute& R, const HitBuffer& hb, const std::vector<uint8_t>& host_buf, unsigned long long count,
                    const int* tflags, const DeviceNms& dnms, std::vector<mtm_hit>& hits) {
    if (dnms.queued && R.sparse && !R.fused && (long long)count >= c->nms_device_min && count <= dnms.n_max) {
        bool trivial = false;       // (a map every pixel of which equals its local maximum loses its peaks: drop_trivial_maps)
        for (int t : c->list2d) trivial = trivial || scan_flags_trivial((unsigned)tflags[(size_t)t]);
        if (!trivial) {
            MTMC(fetch_device_nms(c, dnms, count, hits, &R.nms_sure));
            R.nms_raw_count = (long long)count;
            return MTM_OK;
        }
    }
    hits.resize((size_t)count);
    const size_t got = std::min<size_t>((size_t)count, (host_buf.size() - hb.hdr_bytes) / sizeof(mtm_hit));
    if (got) std::memcpy(hits.data(), hb.host_records(host_buf.data()), sizeof(mtm_hit) * got);
    if (count > got) {
        HIPC(hipMemcpyAsync(hits.data() + got, hb.records() + got, sizeof(mtm_hit) * ((size_t)count - got),
                            hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
    }
    return MTM_OK;
}

int queue_extremum_pass(mtm_ctx* c, const CallRoute& R) {
    if (R.ext) return MTM_OK;
    const size_t key_bytes = sizeof(unsigned long long) * 2 * (size_t)std::max(1, R.n);
    MTMC(c->counters.ensure(key_bytes));
    HIPC(hipMemsetAsync(c->counters.p, 0, key_bytes, c->stream));
    if (R.n > 0) {
        queue_extremum(c->stream, c->maps.as<float>(), c->td.as<TemplDev>(), R.n, c->counters.as<unsigned long long>());
        HIPC(hipGetLastError());
    }
    return MTM_OK;
}

int batch_peak_pass(mtm_ctx* c, int mode, float thr, bool mode_min, int nb, int rows, std::vector<mtm_hit>* per_img) {
    const int n = (int)c->templs.size();
    if (mode == MTM_PEAKS_GLOBAL) {
        std::vector<unsigned long long> best(2 * (size_t)nb * std::max(1, n), 0ull);
        long long max_px = 1;
        for (const TemplDev& d : c->td_host) max_px = std::max(max_px, (long long)(rows - d.rows + 1) * d.ow);
        MTMC(c->counters.ensure(sizeof(unsigned long long) * best.size()));
        HIPC(hipMemsetAsync(c->counters.p, 0, sizeof(unsigned long long) * best.size(), c->stream));
        if (n > 0) {
            queue_extremum_batch(c->stream, c->maps.as<float>(), c->td.as<TemplDev>(), n, rows, nb, max_px,
                                 c->counters.as<unsigned long long>());
            HIPC(hipGetLastError());
        }
        HIPC(hipEventRecord(c->ev[2], c->stream));
        HIPC(hipMemcpyAsync(best.data(), c->counters.p, sizeof(unsigned long long) * best.size(), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        for (int b = 0; b < nb; ++b)
            for (int t = 0; t < n; ++t) {           // (fm_end's decoding, on the image's own index)
                const TemplDev& d = c->td_host[t];
                per_img[b].push_back(decode_extremum_key(best[2 * ((size_t)b * n + t) + (mode_min ? 1 : 0)], mode_min, t,
                                                         d.ow, d.cols, d.rows));
            }
        return MTM_OK;
    }
    std::vector<int> nontriv((size_t)nb * std::max(1, n), 0);
    std::vector<mtm_hit> hits;
    if (!c->list2d.empty()) {
        // [hit count | nontrivial flag per (image, template)] [records]
        const size_t hdr = round_up(sizeof(unsigned long long) + sizeof(int) * nontriv.size(), 16);
        const PeakMaps m = ctx_maps(c);
        bool done = false;
        for (int pass = 0; pass < 2 && !done; ++pass) {         // (a list that overflowed: once more, large enough)
            MTMC(c->hits.ensure(hdr + sizeof(mtm_hit) * (size_t)c->hit_cap));
            uint8_t* dbase = c->hits.as<uint8_t>();
            unsigned long long* counter = reinterpret_cast<unsigned long long*>(dbase);
            mtm_hit* dhits = reinterpret_cast<mtm_hit*>(dbase + hdr);
            HIPC(hipMemsetAsync(dbase, 0, hdr, c->stream));
            queue_scan_batch(c->stream, m, PeakRule{mode_min, thr, c->opt_border},
                             PeakList{dhits, (unsigned long long)c->hit_cap, counter, reinterpret_cast<int*>(counter + 1)}, rows, n);
            HIPC(hipGetLastError());
            std::vector<uint8_t> hb(hdr);
            HIPC(hipMemcpyAsync(hb.data(), dbase, hdr, hipMemcpyDeviceToHost, c->stream));
            HIPC(hipStreamSynchronize(c->stream));
            unsigned long long count = 0;
            std::memcpy(&count, hb.data(), sizeof(count));
            std::memcpy(nontriv.data(), hb.data() + sizeof(count), sizeof(int) * nontriv.size());
            if ((int64_t)count <= c->hit_cap) {
                hits.resize((size_t)count);
                if (count) {
                    HIPC(hipMemcpyAsync(hits.data(), dhits, sizeof(mtm_hit) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
                    HIPC(hipStreamSynchronize(c->stream));
                }
                done = true;
            } else {
                c->hit_cap = (int64_t)count + 1024;
            }
        }
        if (!done) return ladder_exhausted();
    }
    HIPC(hipEventRecord(c->ev[2], c->stream));
    // stack rows -> (image, row); skimage: a map in which every pixel equals its local maximum has no peaks at all
    for (const mtm_hit& h : hits) {
        const int b = h.y / rows;
        if (!nontriv[(size_t)b * n + h.templ_idx]) continue;
        mtm_hit r = h;
        r.y -= b * rows;
        per_img[b].push_back(r);
    }
    return MTM_OK;
}

int window_peak_pass(mtm_ctx* c, int n, bool global, const WindowPeakLaunch& launch, std::vector<unsigned long long>& best,
                     std::vector<mtm_hit>& recs, const char* who) {
    const size_t flag_bytes = sizeof(unsigned long long) * (1 + (size_t)n) + sizeof(int) * (size_t)n;
    MTMC(c->win_flags.ensure(flag_bytes));
    std::vector<uint8_t> fl(flag_bytes);
    unsigned long long cap = (unsigned long long)std::max<int64_t>(1, c->hit_cap), count = 0;
    for (int pass = 0; pass < 2; ++pass) {          // (a list that overflowed: once more, large enough)
        MTMC(c->win_hits.ensure(sizeof(mtm_hit) * (size_t)cap));
        HIPC(hipMemsetAsync(c->win_flags.p, 0, flag_bytes, c->stream));
        unsigned long long* counter = c->win_flags.as<unsigned long long>();
        MTMC(launch(c->win_hits.as<mtm_hit>(), cap, counter, counter + 1, reinterpret_cast<int*>(counter + 1 + n)));
        HIPC(hipMemcpyAsync(fl.data(), c->win_flags.p, flag_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        std::memcpy(&count, fl.data(), sizeof(count));
        if (count <= cap) break;
        if (pass == 1) {            // (cannot happen: the second pass runs with room for every record of the first)
            set_error(std::string(who) + ": hit list overflowed twice");
            return MTM_E_HIP;
        }
        cap = count + 1024;
    }
    if (global) {
        best.resize((size_t)n);
        if (n > 0) std::memcpy(best.data(), fl.data() + sizeof(unsigned long long), sizeof(unsigned long long) * (size_t)n);
        return MTM_OK;
    }
    std::vector<mtm_hit> raw((size_t)count);
    if (count > 0) HIPC(hipMemcpy(raw.data(), c->win_hits.p, sizeof(mtm_hit) * (size_t)count, hipMemcpyDeviceToHost));
    std::vector<int> nontrivial((size_t)n);
    if (n > 0) std::memcpy(nontrivial.data(), fl.data() + sizeof(unsigned long long) * (1 + (size_t)n), sizeof(int) * (size_t)n);
    for (const mtm_hit& r : raw)
        if (nontrivial[(size_t)r.templ_idx]) recs.push_back(r);     // a slot with no output that differs from its
                                                                    // neighbourhood's max has no peaks
    return MTM_OK;
}

}  // namespace mtmi

extern "C" {

// Test support: the chain of queue_nms_chain on a list the caller hands over (tests/test_gpu_device_nms.py).
int mtm_debug_device_nms(mtm_ctx* c, const mtm_hit* hits, int64_t n, int rows, int cols, int max_side, double score_threshold,
                         int ascending, double max_overlap, int64_t n_min, int64_t n_max, mtm_hit* out, int64_t capacity,
                         int64_t* n_champions, int64_t* n_undecided) {
    if (!c) {
        set_error("mtm_debug_device_nms: null context");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_debug_device_nms");
    const bool gate = n >= n_min && n <= n_max;
    if (n < 0 || (n > 0 && !hits) || rows < 1 || cols < 1 || max_side < 0 || !(max_overlap >= 0.0) || n_min < 0 || n_max < 1 ||
        n_max > (1ll << 18) || capacity < 0 || !n_champions || !n_undecided || (gate && (capacity < n || (n > 0 && !out)))) {
        set_error("mtm_debug_device_nms: bad arguments (negative sizes, max_overlap < 0, n_max outside 1 .. 2^18, or a capacity "
                  "below the length of a list inside [n_min, n_max])");
        return MTM_E_INVALID;
    }
    const NmsGrid g = nms_grid(rows, cols, max_side);
    if ((long long)g.gw * g.gh > (1ll << 24)) {
        set_error("mtm_debug_device_nms: more than 2^24 grid cells");
        return MTM_E_INVALID;
    }
    HIPC(hipSetDevice(c->device));
    // [the count][the records]
    MTMC(c->nms_dbg.ensure(256 + sizeof(mtm_hit) * (size_t)std::max<int64_t>(n, 1)));
    uint8_t* d = c->nms_dbg.as<uint8_t>();
    const unsigned long long count = (unsigned long long)n;
    HIPC(hipMemcpyAsync(d, &count, sizeof(count), hipMemcpyHostToDevice, c->stream));
    if (n) HIPC(hipMemcpyAsync(d + 256, hits, sizeof(mtm_hit) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    DeviceNms q;
    MTMC(queue_nms_chain(c, reinterpret_cast<const mtm_hit*>(d + 256), reinterpret_cast<const unsigned long long*>(d),
                         (unsigned)std::min<int64_t>(n_min, 1ll << 30), (size_t)n_max, ascending != 0,
                         (float)(ascending ? (1.0 - score_threshold) : score_threshold), (float)max_overlap, g, &q));
    HIPC(hipStreamSynchronize(c->stream));
    std::vector<mtm_hit> rest;
    long long n_sure = 0;
    MTMC(fetch_device_nms(c, q, count, rest, &n_sure));
    if (!gate && !rest.empty()) {
        set_error("mtm_debug_device_nms: internal state (a list outside [n_min, n_max] produced records)");
        return MTM_E_STATE;
    }
    if (!rest.empty()) std::memcpy(out, rest.data(), sizeof(mtm_hit) * rest.size());
    *n_champions = (int64_t)n_sure;
    *n_undecided = (int64_t)rest.size() - (int64_t)n_sure;
    return MTM_OK;
}

// Test support: the peak pass on maps the caller hands over (tests/test_gpu_peaks.py).  Everything lives in peak_dbg - the
// TemplDev table, the map arena, flags, lists, counters -, laid out per call; nothing of the context's placement or options is
// read or written.  The launches are the launchers' above, the ones queue_peak_pass / queue_extremum_pass / batch_peak_pass
// go through, and `info` is what they derived.
int mtm_debug_peak_pass(mtm_ctx* c, const mtm_peak_pass* a) {
    if (!c || !a) {
        set_error("mtm_debug_peak_pass: null context or arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_debug_peak_pass");
    const auto bad = [](const char* what) {
        set_error(std::string("mtm_debug_peak_pass: ") + what);
        return MTM_E_INVALID;
    };
    const int n = a->n_maps, route = a->route;
    if (n < 1 || n > 4096 || route < MTM_PEAK_SCAN || route > MTM_PEAK_EXTREMUM_BATCH || !a->dims || !a->maps || !a->info ||
        (a->border != MTM_BORDER_CONSTANT && a->border != MTM_BORDER_NEAREST) || a->hit_cap < 1 || a->hit_cap > (1ll << 24) ||
        a->pattern_byte < 0 || a->pattern_byte > 255 || a->capacity < 0 || a->n_ints < 0 || a->list_cap < 0)
        return bad("bad arguments (1 .. 4096 maps, a route, a border rule, hit_cap in 1 .. 2^24, a pattern byte)");
    const bool batch = route == MTM_PEAK_SCAN_BATCH || route == MTM_PEAK_EXTREMUM_BATCH;
    const bool ext = route == MTM_PEAK_EXTREMUM || route == MTM_PEAK_EXTREMUM_BATCH;
    const bool verify = route == MTM_PEAK_VERIFY_MAPS || route == MTM_PEAK_VERIFY_HASH;
    // the table, as plan_placement fills the fields the peak kernels read
    std::vector<TemplDev> td((size_t)n, TemplDev{});
    std::vector<size_t> src_off((size_t)n);
    size_t arena = 0, src = 0;
    PeakMaps pm{nullptr, nullptr, nullptr, n, 0, 0};        // (the pointers: once the arena is laid out)
    int n_img = 1;
    long long max_px = 1;
    for (int t = 0; t < n; ++t) {
        const int oh = a->dims[4 * t], ow = a->dims[4 * t + 1], h = a->dims[4 * t + 2], w = a->dims[4 * t + 3];
        const int least = ext ? 1 : 2;          // (the scans and verifiers only ever see 2-D maps: mtm_ctx::list2d)
        if (oh < least || ow < least || oh > kBatchMaxRows || ow > 65535 || h < 1 || w < 1) return bad("a map's size");
        TemplDev& d = td[(size_t)t];
        d.rows = h;
        d.cols = w;
        d.oh = oh;
        d.ow = ow;
        d.map_pitch = map_pitch_of(ow);
        d.map_off = (long long)arena;
        d.k1_off = d.k2_off = d.pack_off = -1;
        arena += (size_t)d.map_pitch * oh;
        src_off[(size_t)t] = src;
        src += (size_t)oh * ow;
        pm.max_oh = std::max(pm.max_oh, oh);
        pm.max_ow = std::max(pm.max_ow, ow);
        if (batch) {
            if (a->img_rows < 2 || h > a->img_rows - 1 || (oh + h - 1) % a->img_rows != 0) return bad("img_rows does not fit a map");
            const int nbt = (oh + h - 1) / a->img_rows;
            if (t > 0 && nbt != n_img) return bad("the maps' stacks differ in their number of images");
            n_img = nbt;
            max_px = std::max(max_px, (long long)(a->img_rows - h + 1) * ow);
        }
    }
    if (arena > (64ull << 20)) return bad("more than 2^26 floats of maps");
    const size_t n_ints = (size_t)n * (size_t)n_img;
    const size_t capacity = (size_t)a->capacity;
    if (ext) {
        if (!a->keys || !a->ext_hits || (size_t)a->n_ints < n_ints) return bad("the extremum routes need keys and ext_hits of 2 * n_ints");
    } else if (!a->records || !a->count || !a->raw || !a->trivial || (size_t)a->n_ints < n_ints || a->capacity < a->hit_cap) {
        return bad("records (capacity >= hit_cap), count, raw and trivial (n_ints each) are needed");
    }
    // the segment route's lists, and its flags: a byte per (map, row, strip column), padded to the largest map
    const unsigned long long hit_cap = (unsigned long long)a->hit_cap;
    SegLists seg;
    size_t flag_rstride = 0, flag_tstride = 0;
    if (route == MTM_PEAK_SEGMENTS) {
        seg = segment_lists(pm, hit_cap);
        flag_rstride = seg.grid.x;
        flag_tstride = (size_t)pm.max_oh * seg.grid.x;
        if (!a->flags || !a->list_counts || (unsigned long long)a->list_cap < seg.n_lists) return bad("flags and list_counts (one per list) are needed");
    }
    unsigned hash_mask = 0;
    size_t n_judged = 0;
    if (verify) {
        if (a->cand_cap < 1 || a->cand_cap > kCandListMax || a->cand_count < 0 || a->n_cands < 0 || (a->n_cands > 0 && !a->cands))
            return bad("the candidate list (cand_cap in 1 .. 2^20)");
        n_judged = (size_t)std::min(a->cand_count, a->cand_cap);
        if ((size_t)a->n_cands < n_judged) return bad("fewer candidate records than min(cand_count, cand_cap)");
        for (size_t i = 0; i < n_judged; ++i) {
            const mtm_hit& h = a->cands[i];
            if (h.templ_idx < 0 || h.templ_idx >= n || h.x < 0 || h.y < 0 || h.x >= td[(size_t)h.templ_idx].ow ||
                h.y >= td[(size_t)h.templ_idx].oh)
                return bad("a candidate outside its map");
        }
        if (route == MTM_PEAK_VERIFY_HASH) hash_mask = (unsigned)(cand_hash_slots(a->cand_cap) - 1);        // (as plan_call)
    }
    // peak_dbg: [table][map list][count | per-map ints][records][maps][flags][candidates][hash][list counters][lists][keys]
    size_t total = 0;
    const auto take = [&](size_t bytes) {
        const size_t off = total;
        total += round_up(std::max<size_t>(bytes, 16), 256);
        return off;
    };
    const size_t o_td = take(sizeof(TemplDev) * (size_t)n), o_tl = take(sizeof(int) * (size_t)n);
    const size_t hdr_bytes = 16 + sizeof(int) * n_ints;
    const size_t o_hdr = take(hdr_bytes), o_rec = take(sizeof(mtm_hit) * capacity), o_maps = take(sizeof(float) * arena);
    const size_t flag_bytes = (size_t)n * flag_tstride;
    const size_t o_flags = take(flag_bytes);
    const size_t o_cand = take(16 + sizeof(mtm_hit) * (size_t)std::max<int64_t>(verify ? a->cand_cap : 0, 1));
    const size_t o_hash = take(hash_mask ? cand_hash_bytes(hash_mask) : 0);
    const size_t o_cnt = take(seg.cnt_bytes), o_lists = take(seg.list_bytes);
    const size_t key_bytes = sizeof(unsigned long long) * 2 * n_ints;
    const size_t o_keys = take(key_bytes);
    HIPC(hipSetDevice(c->device));
    MTMC(c->peak_dbg.ensure(total));
    uint8_t* b = c->peak_dbg.as<uint8_t>();
    // the arena as the device will hold it: the pattern, then the maps row by row (holes: flagged segments only)
    std::vector<uint8_t> stage(sizeof(float) * arena, (uint8_t)a->pattern_byte);
    for (int t = 0; t < n; ++t) {
        const TemplDev& d = td[(size_t)t];
        for (int y = 0; y < d.oh; ++y) {
            const float* from = a->maps + src_off[(size_t)t] + (size_t)y * d.ow;
            uint8_t* to = stage.data() + sizeof(float) * ((size_t)d.map_off + (size_t)y * d.map_pitch);
            if (route == MTM_PEAK_SEGMENTS && a->holes) {
                for (int sx = 0; sx * kPkCols < d.ow; ++sx)
                    if (a->flags[(size_t)t * flag_tstride + (size_t)y * flag_rstride + (size_t)sx])
                        std::memcpy(to + sizeof(float) * (size_t)sx * kPkCols, from + (size_t)sx * kPkCols,
                                    sizeof(float) * (size_t)std::min(kPkCols, d.ow - sx * kPkCols));
            } else {
                std::memcpy(to, from, sizeof(float) * (size_t)d.ow);
            }
        }
    }
    std::vector<int> tl((size_t)n);
    for (int t = 0; t < n; ++t) tl[(size_t)t] = t;
    HIPC(hipMemcpyAsync(b + o_td, td.data(), sizeof(TemplDev) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(b + o_tl, tl.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(b + o_hdr, 0, hdr_bytes, c->stream));
    if (!ext && capacity) HIPC(hipMemcpyAsync(b + o_rec, a->records, sizeof(mtm_hit) * capacity, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(b + o_maps, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream));
    pm.maps = reinterpret_cast<const float*>(b + o_maps);
    pm.td = reinterpret_cast<const TemplDev*>(b + o_td);
    pm.tlist = reinterpret_cast<const int*>(b + o_tl);
    const PeakRule scan{a->mode_min != 0, a->thr, a->border};
    const PeakList list{reinterpret_cast<mtm_hit*>(b + o_rec), hit_cap, reinterpret_cast<unsigned long long*>(b + o_hdr),
                        reinterpret_cast<int*>(b + o_hdr + 16)};
    unsigned long long* dkeys = reinterpret_cast<unsigned long long*>(b + o_keys);
    PeakGrid grd = scan_grid(pm, kPkRows);      // (reported on every route, also those without a scan)
    unsigned blocks = 0;
    int nbk = 0;
    if (route == MTM_PEAK_SCAN) {
        grd = queue_scan(c->stream, pm, scan, list);
    } else if (route == MTM_PEAK_SCAN_BATCH) {
        grd = queue_scan_batch(c->stream, pm, scan, list, a->img_rows, n);
    } else if (route == MTM_PEAK_SEGMENTS) {
        unsigned long long* counts_t = reinterpret_cast<unsigned long long*>(b + o_cnt);
        HIPC(hipMemcpyAsync(b + o_flags, a->flags, flag_bytes, hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemsetAsync(counts_t, 0, seg.cnt_bytes, c->stream));
        queue_segments(c->stream, pm, scan, list, seg, counts_t, reinterpret_cast<mtm_hit*>(b + o_lists),
                       SegFlags{b + o_flags, (int)flag_tstride, (int)flag_rstride, a->holes != 0});
        grd = seg.grid;
    } else if (verify) {
        const unsigned long long cc[2] = {(unsigned long long)a->cand_count, 0ull};
        unsigned long long* dcc = reinterpret_cast<unsigned long long*>(b + o_cand);
        unsigned long long* keys = hash_mask ? reinterpret_cast<unsigned long long*>(b + o_hash) : nullptr;
        HIPC(hipMemcpyAsync(dcc, cc, sizeof(cc), hipMemcpyHostToDevice, c->stream));
        if (n_judged) HIPC(hipMemcpyAsync(b + o_cand + 16, a->cands, sizeof(mtm_hit) * n_judged, hipMemcpyHostToDevice, c->stream));
        if (keys) HIPC(hipMemsetAsync(keys, 0, cand_hash_key_bytes(hash_mask), c->stream));
        blocks = queue_verify(c->stream, pm, PeakRule{scan.mode_min, a->thr_q, a->border}, list, dcc, (unsigned long long)a->cand_cap,
                              keys, hash_mask);
    } else {
        HIPC(hipMemsetAsync(dkeys, 0, key_bytes, c->stream));
        nbk = route == MTM_PEAK_EXTREMUM ? queue_extremum(c->stream, pm.maps, pm.td, n, dkeys)
                                         : queue_extremum_batch(c->stream, pm.maps, pm.td, n, a->img_rows, n_img, max_px, dkeys);
    }
    HIPC(hipGetLastError());
    std::vector<uint8_t> hdr(hdr_bytes);
    HIPC(hipMemcpyAsync(hdr.data(), b + o_hdr, hdr_bytes, hipMemcpyDeviceToHost, c->stream));
    if (!ext && capacity) HIPC(hipMemcpyAsync(a->records, b + o_rec, sizeof(mtm_hit) * capacity, hipMemcpyDeviceToHost, c->stream));
    if (seg.n_lists)
        HIPC(hipMemcpyAsync(a->list_counts, b + o_cnt, sizeof(unsigned long long) * (size_t)seg.n_lists, hipMemcpyDeviceToHost, c->stream));
    if (ext) HIPC(hipMemcpyAsync(a->keys, dkeys, key_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    if (ext) {
        for (size_t i = 0; i < n_ints; ++i) {
            const TemplDev& d = td[i % (size_t)n];
            a->ext_hits[2 * i] = decode_extremum_key(a->keys[2 * i], false, (int)(i % (size_t)n), d.ow, d.cols, d.rows);
            a->ext_hits[2 * i + 1] = decode_extremum_key(a->keys[2 * i + 1], true, (int)(i % (size_t)n), d.ow, d.cols, d.rows);
        }
    } else {
        unsigned long long count = 0;
        std::memcpy(&count, hdr.data(), sizeof(count));
        *a->count = count;
        std::memcpy(a->raw, hdr.data() + 16, sizeof(int) * n_ints);
        for (size_t i = 0; i < n_ints; ++i) {
            const TemplDev& d = td[i % (size_t)n];
            const int f = a->raw[i];
            a->trivial[i] = verify ? fused_count_trivial(f, d.oh, d.ow) : batch ? f == 0 : scan_flags_trivial((unsigned)f);
        }
    }
    const int64_t info[8] = {(int64_t)grd.x, (int64_t)grd.y, (int64_t)grd.z, (int64_t)seg.cap_t, (int64_t)seg.n_lists, (int64_t)blocks,
                             hash_mask ? (int64_t)hash_mask + 1 : 0, (int64_t)nbk};
    std::memcpy(a->info, info, sizeof(info));
    return MTM_OK;
}

}  // extern "C"
