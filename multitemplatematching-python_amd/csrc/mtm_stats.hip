// libmtm_hip.so - the host side of the window statistics: one launcher per route of stats_route (mtm_stats_route.h),
// launch_stats - what a size class's score kernel reads (stat_wants), the planes, the route's launch - and the two
// test-support entries (mtm_debug_window_stats, mtm_debug_window_stats_route).  The only unit that launches
// mtm_k_stats.hip.h: a search and the test entries run the same launch code.
#include "mtm_ctx.h"

using namespace mtm;
using namespace mtmi;
#include "mtm_k_stats.hip.h"

namespace mtmi {

// One stats_u8_kernel launch: the row units [a.sb0, a.sb1) of the fused single-channel uint8 statistics, in form `form`
// (kStatForms, from 1; 0 = stats_u8_form's choice; *form_took: the one that ran).  Fills the derived fields of `a`.
// launch_stats and the test-support entry mtm_debug_window_stats both come through here.
static int launch_stats_u8(hipStream_t stream, StatU8Args a, int form, int n_cus, int* form_took = nullptr) {
    if (a.sb1 <= a.sb0) return MTM_OK;
    a.owg = stats_u8_owg(a.w);
    const int strips = (a.ow + a.owg - 1) / a.owg;
    if (form == 0) form = stats_u8_form(strips, a.sb1 - a.sb0, n_cus);
    if (form < 1 || form > kStatFormCount) {
        set_error("launch_stats_u8: no such form");
        return MTM_E_INVALID;
    }
    if (form_took) *form_took = form;
    a.rows_wg = kStatFormRows[form - 1];
    a.inv_area = 1.0 / ((double)a.h * (double)a.w);
    const bool tail = a.blkq != nullptr;
    if (tail) {
        a.inv_nq[0] = 1.0 / (double)((a.h - a.tail_s) * a.w);
        a.inv_nq[1] = 1.0 / (double)((a.h - a.tail_s + 1) * a.w);
    }
    const dim3 grid(strips, stats_u8_grid_y(a.sb0, a.sb1, a.oh, a.rows_wg)), block(kStatStrip / 4);
    if (grid.y == 0) return MTM_OK;
    // (the tail boxes and the reciprocal plane in instantiations of their own: a launch without them pays nothing for them)
    auto* kernel = tail ? (a.rsq ? stats_u8_kernel<true, true> : stats_u8_kernel<true, false>)
                        : (a.rsq ? stats_u8_kernel<false, true> : stats_u8_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// ---- one launcher per route of stats_route (mtm_stats_route.h) but the first, which launch_stats_u8 above is: a stream,
// explicit device pointers and geometry (StatGeom, StatScratch, StatOut: mtm_ctx.h), nothing of a context.  launch_stats,
// mbf_prepare (mtm_launch.hip) and the test-support entry mtm_debug_window_stats_route all come through them.

// (every launcher: the planes' rows hold the output row - the fused kernels store whole quads)
static int stat_out_check(const StatGeom& g, const StatOut& o) {
    if (o.st_pitch >= g.ow && o.st_pitch % 4 == 0) return MTM_OK;
    set_error("statistics launch: a plane pitch below the output width, or no multiple of 4");
    return MTM_E_INVALID;
}

// U8MC: stats_u8_mc_kernel<3> over the three uint8 planes
static int launch_stats_u8mc(hipStream_t stream, const uint8_t* u8, int pitch, long long plane, const StatGeom& g, const StatOut& o) {
    MTMC(stat_out_check(g, o));
    const int owg = stats_u8_owg(g.w);
    const dim3 gs((g.ow + owg - 1) / owg, (g.oh + kStatBand4 - 1) / kStatBand4);
    hipLaunchKernelGGL(stats_u8_mc_kernel<3>, gs, dim3(256), 0, stream, u8, pitch, plane, g.h, g.w, g.oh, g.ow, owg, g.inv_area,
                       o.num_type, o.want_sq, o.want_t, o.want_sum2, o.t[0], o.t_plane, o.sum2, o.sq, o.st_pitch);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// U16: stats_u16_kernel over the two biased byte planes, row units [sb0, sb1) of kStatBand4 output rows; blk: the records
// per 16-column block (null: none)
static int launch_stats_u16(hipStream_t stream, const uint8_t* hib, const uint8_t* lob, int pitch, const StatGeom& g,
                            const StatOut& o, double* blk, int blk_pitch, int sb0, int sb1) {
    MTMC(stat_out_check(g, o));
    if (sb1 <= sb0) return MTM_OK;
    const int owg = stats_u8_owg(g.w);
    const dim3 gs((g.ow + owg - 1) / owg, sb1 - sb0);
    hipLaunchKernelGGL(stats_u16_kernel, gs, dim3(256), 0, stream, hib, lob, pitch, g.h, g.w, g.oh, g.ow, owg, g.inv_area,
                       o.num_type, o.want_sq, o.want_t, o.want_sum2, o.t[0], o.sum2, o.sq, o.st_pitch, blk, blk_pitch, sb0);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// the second pass of the two-pass chains: output rows [o0, o1), o0 a multiple of kVsumBand (a band restarts its column sums)
template <typename AccT, typename SumT>
static int launch_vsum(hipStream_t stream, const StatGeom& g, const StatScratch& s, const StatOut& o, int o0, int o1) {
    MTMC(stat_out_check(g, o));
    if (o1 <= o0) return MTM_OK;
    if (o0 % kVsumBand != 0) {
        set_error("launch_vsum: a launch starts on a whole band of output rows");
        return MTM_E_INVALID;
    }
    const dim3 g2((g.ow + 255) / 256, (o1 - o0 + kVsumBand - 1) / kVsumBand);
    hipLaunchKernelGGL((vsum_stats_kernel<AccT, SumT>), g2, dim3(256), 0, stream, static_cast<const AccT*>(s.hs1),
                       static_cast<const AccT*>(s.hs2), s.pitch, s.plane, g.chans, g.h, g.oh, g.ow, g.inv_area, o.num_type,
                       o.want_sq, o.want_t, o.t[0], o.t[1], o.t[2], o.t[3], o.sum2, o.sq, o.st_pitch, o0 / kVsumBand);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// U8_2P: hsum_u8_kernel (a row's two prefix sums in LDS: cols <= kStatsHsumU8MaxCols) + vsum over uint32 row sums
static int launch_stats_u8_2p(hipStream_t stream, const uint8_t* u8, int pitch, long long plane, const StatGeom& g,
                              const StatScratch& s, const StatOut& o) {
    hipLaunchKernelGGL(hsum_u8_kernel, dim3(g.rows, g.chans), dim3(256), sizeof(uint32_t) * 2 * (g.cols + 1), stream, u8, pitch,
                       plane, g.cols, g.w, g.ow, static_cast<uint32_t*>(s.hs1), static_cast<uint32_t*>(s.hs2), s.pitch, s.plane);
    HIPC(hipGetLastError());
    return launch_vsum<uint32_t, unsigned long long>(stream, g, s, o, 0, g.oh);
}

// U8_2P_WIDE: the generic hsum_kernel on the float32 plane of a uint8 image (uint32 row sums: exact) + the same vsum
static int launch_stats_u8_2p_wide(hipStream_t stream, const float* f32, int pitch, long long plane, const StatGeom& g,
                                   const StatScratch& s, const StatOut& o) {
    const dim3 g1((g.ow + 256 * kHsumSeg - 1) / (256 * kHsumSeg), g.rows, g.chans);
    hipLaunchKernelGGL(hsum_kernel<uint32_t>, g1, dim3(256), 0, stream, f32, pitch, plane, g.rows, g.w, g.ow,
                       static_cast<uint32_t*>(s.hs1), static_cast<uint32_t*>(s.hs2), s.pitch, s.plane);
    HIPC(hipGetLastError());
    return launch_vsum<uint32_t, unsigned long long>(stream, g, s, o, 0, g.oh);
}

// F64_LDS (declared in mtm_ctx.h: the masked float32 screen takes its window sums from it too)
int launch_stats_f64_lds(hipStream_t stream, const float* f32, int pitch, long long plane, const StatGeom& g,
                         const StatScratch& s, const StatOut& o, int r0, int r1, int o0, int o1) {
    if (r1 > r0) {
        const dim3 g1((g.ow + 256 * kHsumSeg - 1) / (256 * kHsumSeg), r1 - r0, g.chans);
        hipLaunchKernelGGL(hsum_lds_kernel, g1, dim3(256), hsum_lds_bytes(g.w), stream, f32, pitch, plane, g.rows, g.w, g.ow,
                           static_cast<double*>(s.hs1), static_cast<double*>(s.hs2), s.pitch, s.plane, r0);
        HIPC(hipGetLastError());
    }
    return launch_vsum<double, double>(stream, g, s, o, o0, o1);
}

// F64: the generic hsum_kernel<double> (any window width) + the same vsum, whole image
static int launch_stats_f64(hipStream_t stream, const float* f32, int pitch, long long plane, const StatGeom& g,
                            const StatScratch& s, const StatOut& o) {
    const dim3 g1((g.ow + 256 * kHsumSeg - 1) / (256 * kHsumSeg), g.rows, g.chans);
    hipLaunchKernelGGL(hsum_kernel<double>, g1, dim3(256), 0, stream, f32, pitch, plane, g.rows, g.w, g.ow,
                       static_cast<double*>(s.hs1), static_cast<double*>(s.hs2), s.pitch, s.plane);
    HIPC(hipGetLastError());
    return launch_vsum<double, double>(stream, g, s, o, 0, g.oh);
}

// ---- launch_stats, in stages

// c->stats sized for the class and carved into its planes (kMaxChans window-sum planes, sum2, sq), the row-sum planes
// c->hs1 / hs2 sized: what every launcher but the fused single-channel one takes (*o, *hs), and the plane table's planes
static int stat_buffers(mtm_ctx* c, const SizeClass& sc, const StatWants& wants, StatOut* o, StatScratch* hs, StatPlanes* st) {
    const int oh = c->rows - sc.h + 1;
    const size_t plane = (size_t)st->pitch * oh;
    MTMC(c->stats.ensure(sizeof(double) * plane * (kMaxChans + 2)));
    double* base = c->stats.as<double>();
    const long long hs_plane = (long long)st->pitch * c->rows;
    const size_t esz = c->dtype == MTM_U8 ? sizeof(uint32_t) : sizeof(double);
    MTMC(c->hs1.ensure(esz * hs_plane * c->chans));
    MTMC(c->hs2.ensure(esz * hs_plane * c->chans));
    *hs = StatScratch{c->hs1.p, c->hs2.p, st->pitch, hs_plane};
    *o = StatOut{};
    o->num_type = wants.num_type, o->want_sq = wants.normed ? 1 : 0, o->want_t = wants.want_t ? 1 : 0, o->want_sum2 = 1;
    for (int k = 0; k < kMaxChans; ++k) st->t[k] = o->t[k] = base + plane * k;
    st->sum2 = o->sum2 = base + plane * kMaxChans;
    st->sq = o->sq = base + plane * (kMaxChans + 1);
    o->t_plane = (long long)plane, o->st_pitch = st->pitch;
    return MTM_OK;
}

// The fused single-channel uint8 route: the reciprocal plane and the block records the class wants, the tail boxes' records
// and the templates' tail constants where its score launch will screen its K loop, then ONE stats_u8_kernel launch over the
// band's row units - with the layout conversion of the band's rows and the clearing of the candidate header of a banded call.
static int launch_stats_fused_u8(mtm_ctx* c, CallRoute& R, const SizeClass& sc, const StatWants& wants, const StatBand& band,
                                 const ImageDev& img, const StatOut& o, StatPlanes* st) {
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    const int nsb = (oh + kStatBand4 - 1) / kStatBand4;
    const int b1 = band.sb1 < 0 ? nsb : std::min(band.sb1, nsb);
    double* rsq = nullptr;
    if (wants.rsq) {
        MTMC(c->stats_rsq.ensure(sizeof(double) * (size_t)o.t_plane));
        rsq = c->stats_rsq.as<double>();
    }
    double* blk = nullptr;
    double* blkq = nullptr;
    int tail_s = 0;
    if (wants.blk) {
        st->blk_pitch = (st->pitch + 15) / 16;
        // (the tail boxes' records, when the score launch screens its K loop, follow the window's in the same buffer)
        const size_t nrec = 4 * (size_t)st->blk_pitch * oh;
        tail_s = tail_split_for(c, R, sc);
        MTMC(ensure_tail_consts(c, sc, tail_s));
        MTMC(c->stats_blk.ensure(sizeof(double) * nrec * (tail_s ? 2 : 1)));
        st->blk = blk = c->stats_blk.as<double>();
        if (tail_s) st->blkq = blkq = blk + nrec;
    }
    if (b1 <= band.sb0) return MTM_OK;
    // banded upload with the layout conversion of the band's rows on this launch (run_score_banded): the kernel reads
    // the raw upload buffer (every row that has arrived so far is there) and writes the planes of the new rows
    StatLayout lay{};
    const uint8_t* src = img.u8;
    int src_pitch = img.u8_pitch;
    if (band.lay_r1 > band.lay_r0) {
        mtm_ctx::ImageSlot& sl = c->slot[c->cur];
        lay.u8 = sl.u8.as<uint8_t>();
        lay.u8b = sl.u8b.as<uint8_t>();
        lay.pitch = img.u8_pitch;
        lay.r0 = band.lay_r0;
        lay.r1 = band.lay_r1;
        src = sl.raw.as<uint8_t>();
        src_pitch = c->cols;
    }
    if (R.zero_pending && band.stream != nullptr) {         // banded call: the candidate header is cleared here
        lay.zero16 = c->cands.as<unsigned long long>();
        R.zero_pending = false;
    }
    StatU8Args a{};
    a.img = src;
    a.pitch = src_pitch;
    a.h = sc.h, a.w = sc.w, a.oh = oh, a.ow = ow;
    a.num_type = o.num_type, a.want_sq = o.want_sq, a.want_t = o.want_t, a.want_sum2 = wants.want_sum2 ? 1 : 0;
    a.t0 = o.t[0], a.sum2 = o.sum2, a.sq = o.sq, a.rsq = rsq, a.st_pitch = st->pitch;
    a.blk = blk, a.blkq = blkq, a.blk_pitch = st->blk_pitch, a.tail_s = blkq ? tail_s : 0;
    a.sb0 = band.sb0, a.sb1 = b1;
    a.lay = lay;
    return launch_stats_u8(band.stream ? band.stream : c->stream, a, 0, c->n_cus > 0 ? c->n_cus : 256);
}

// Window statistics of one size class, into c->stats.  Returns the plane table.  `band`: the part a band of a banded
// upload asks for, on its stream (StatBand, mtm_ctx.h); the default is the whole image on c->stream.
int launch_stats(mtm_ctx* c, CallRoute& R, const SizeClass& sc, StatPlanes* out, const StatBand& band) {
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    StatPlanes st{};
    st.pitch = (int)round_up((size_t)ow, 4);
    *out = st;
    const StatWants wants = stat_wants(c->method, sc.kernel, sc.masked, sc.mask_rm_off >= 0, sc.r2, sc.rm_R, c->chans, c->dtype);
    if (wants.none) return MTM_OK;
    StatOut o;
    StatScratch hs;
    MTMC(stat_buffers(c, sc, wants, &o, &hs, &st));
    const ImageDev img = image_dev(c);
    const StatGeom g = stat_geom(c->rows, c->cols, c->chans, sc.h, sc.w);
    const hipStream_t band_stream = band.stream ? band.stream : c->stream;
    const StatsRoute route = stats_route(c->dtype, c->chans, sc.h, sc.w, c->cols, c->fuse_stats != 0);
    switch (route) {
    case kStatsRouteU8:             // fused single-kernel statistics for the common case
        MTMC(launch_stats_fused_u8(c, R, sc, wants, band, img, o, &st));
        break;
    case kStatsRouteU8MC:           // RGB: the fused kernel with one scan per channel + one for the squares
        MTMC(launch_stats_u8mc(c->stream, img.u8, img.u8_pitch, img.u8_plane, g, o));
        break;
    case kStatsRouteU8TwoPass:
        MTMC(launch_stats_u8_2p(c->stream, img.u8, img.u8_pitch, img.u8_plane, g, hs, o));
        break;
    case kStatsRouteU8TwoPassWide:
        MTMC(ensure_f32_plane(c));
        MTMC(launch_stats_u8_2p_wide(c->stream, img.f32, img.f32_pitch, img.f32_plane, g, hs, o));
        break;
    case kStatsRouteU16: {          // single-channel uint16: the fused kernel over the two byte planes (the ones the MFMA kernel reads)
        const int nsb = (oh + kStatBand4 - 1) / kStatBand4;
        const uint8_t* hib = c->slot[c->cur].u8b.as<uint8_t>();
        double* blk = nullptr;
        if (wants.blk) {
            st.blk_pitch = (st.pitch + 15) / 16;
            MTMC(c->stats_blk.ensure(sizeof(double) * 4 * (size_t)st.blk_pitch * oh));
            st.blk = blk = c->stats_blk.as<double>();
        }
        MTMC(launch_stats_u16(band_stream, hib, hib + img.u8_plane, img.u8_pitch, g, o, blk, st.blk_pitch,
                              band.sb0, band.sb1 < 0 ? nsb : std::min(band.sb1, nsb)));
        break;
    }
    case kStatsRouteF64Lds: {
        // banded float32 uploads (run_score_banded_f32): the horizontal sums of the image rows that have just arrived, then
        // the output rows whose windows they complete, in units of kStatBand4 rows that make whole vsum bands (a band
        // restarts its column sums: the planes are bit for bit those of one launch)
        const bool part = band.lay_r1 > band.lay_r0;
        if (!part) MTMC(ensure_f32_plane(c));
        const int o0 = part ? band.sb0 * kStatBand4 : 0, o1 = part && band.sb1 >= 0 ? std::min(oh, band.sb1 * kStatBand4) : oh;
        MTMC(launch_stats_f64_lds(band_stream, img.f32, img.f32_pitch, img.f32_plane, g, hs, o, part ? band.lay_r0 : 0,
                                  part ? band.lay_r1 : c->rows, o0, o1));
        break;
    }
    default:                        // kStatsRouteF64
        MTMC(ensure_f32_plane(c));
        MTMC(launch_stats_f64(band_stream, img.f32, img.f32_pitch, img.f32_plane, g, hs, o));
        break;
    }
    HIPC(hipGetLastError());
    if (wants.masked_mfma) MTMC(launch_masked_sumsq(c, sc, route == kStatsRouteU8, st, o.sum2));
    *out = st;
    return MTM_OK;
}

}  // namespace mtmi

namespace {

// ---- what the two test-support entries share

// their arena (mtm_ctx::stats_dbg), laid out per call: offsets rounded to 256 bytes, at least 16 bytes a piece
struct DebugArena {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t off = total;
        total += round_up(std::max<size_t>(bytes, 16), 256);
        return off;
    }
};

// `launch()` between an event pair of its own on `stream`, waited for: *ns its nanoseconds.  The events are destroyed on
// every path; the launch's error comes before the runtime's.
template <class Launch>
int timed_launch(hipStream_t stream, Launch&& launch, int64_t* ns) {
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = MTM_OK;
    float ms = 0.0f;
    hipError_t e = hipEventCreate(&ev[0]);
    if (e == hipSuccess) e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], stream);
    if (e == hipSuccess) rc = launch();
    if (e == hipSuccess && rc == MTM_OK) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess && rc == MTM_OK) e = hipStreamSynchronize(stream);
    if (e == hipSuccess && rc == MTM_OK) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    MTMC(rc);
    HIPC(e);
    *ns = (int64_t)llround((double)ms * 1e6);
    return MTM_OK;
}

// a piece of the arena into the caller's array, where they asked for it
int fetch(void* to, const uint8_t* from, size_t bytes) {
    if (to) HIPC(hipMemcpy(to, from, bytes, hipMemcpyDeviceToHost));
    return MTM_OK;
}

}  // namespace

extern "C" {

// Test support: stats_u8_kernel on an image the caller hands over (tests/test_gpu_window_stats.py), launched by
// launch_stats_u8 like every statistics launch of a search call.  Everything lives in stats_dbg, laid out per call and
// filled with the caller's pattern first; nothing of the context's image, placement or options is read or written.
int mtm_debug_window_stats(mtm_ctx* c, const mtm_window_stats* a) {
    if (!c || !a) {
        set_error("mtm_debug_window_stats: null context or arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_debug_window_stats");
    const auto bad = [](const char* what) {
        set_error(std::string("mtm_debug_window_stats: ") + what);
        return MTM_E_INVALID;
    };
    const int rows = a->rows, cols = a->cols, h = a->h, w = a->w;
    if (!a->image || !a->info || rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || h < 1 || w < 1 || h > rows || w > cols)
        return bad("an image of 1 .. 16384 rows and columns and a window inside it are needed");
    if (stats_route(MTM_U8, 1, h, w, cols, true) != kStatsRouteU8) return bad("the fused kernel takes w <= 768 and w h 255^2 < 2^32");
    if (a->num_type < 0 || a->num_type > 2 || a->form < 0 || a->form > kStatFormCount || a->pattern_byte < 0 || a->pattern_byte > 255)
        return bad("num_type 0 .. 2, a form and a pattern byte");
    const int oh = rows - h + 1, ow = cols - w + 1, nsb = (oh + kStatBand4 - 1) / kStatBand4;
    const int sb0 = a->sb0, sb1 = a->sb1 < 0 ? nsb : std::min(a->sb1, nsb);
    if (sb0 < 0 || sb0 >= sb1) return bad("an empty range of row units");
    const bool conv = a->lay_r1 > a->lay_r0;
    if (conv && (cols % 4 != 0 || a->lay_r0 < 0 || a->lay_r1 > rows)) return bad("the conversion needs cols % 4 == 0 and rows inside the image");
    const bool tail = a->tail_s != 0;
    if (tail && (a->tail_s < 1 || a->tail_s > h - 1 || !a->blk || !a->blkq)) return bad("tail_s in 1 .. h - 1, with blk and blkq");
    if (!tail && a->blkq) return bad("blkq without tail_s");
    if (a->rsq && !a->sq) return bad("rsq without sq");
    const int st_pitch = (int)round_up((size_t)ow, 4), blk_pitch = (st_pitch + 15) / 16;
    const int pitch = (int)round_up((size_t)cols + kPadCols, 64), rows_alloc = rows + kPadRows;
    // stats_dbg: [header][raw image][uint8 plane][int8 view][t0][sum2][sq][rsq][blk][blkq]
    DebugArena ar;
    const size_t plane_bytes = (size_t)pitch * rows_alloc, st_bytes = sizeof(double) * (size_t)st_pitch * oh;
    const size_t rec_bytes = sizeof(double) * 4 * (size_t)blk_pitch * oh;
    const size_t o_hdr = ar.take(16), o_raw = ar.take((size_t)rows * cols), o_u8 = ar.take(plane_bytes), o_u8b = ar.take(plane_bytes);
    const size_t o_t0 = ar.take(st_bytes), o_sum2 = ar.take(st_bytes), o_sq = ar.take(st_bytes), o_rsq = ar.take(st_bytes);
    const size_t o_blk = ar.take(rec_bytes), o_blkq = ar.take(rec_bytes);
    HIPC(hipSetDevice(c->device));
    MTMC(c->stats_dbg.ensure(ar.total));
    uint8_t* b = c->stats_dbg.as<uint8_t>();
    HIPC(hipMemsetAsync(b, a->pattern_byte, ar.total, c->stream));
    HIPC(hipMemcpyAsync(b + o_raw, a->image, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream));
    if (!conv) {        // the plane as an upload leaves it: the image, zero padding
        HIPC(hipMemsetAsync(b + o_u8, 0, plane_bytes, c->stream));
        HIPC(hipMemcpy2DAsync(b + o_u8, (size_t)pitch, a->image, (size_t)cols, (size_t)cols, (size_t)rows, hipMemcpyHostToDevice,
                              c->stream));
    }
    StatU8Args k{};
    k.img = conv ? b + o_raw : b + o_u8;
    k.pitch = conv ? cols : pitch;
    k.h = h, k.w = w, k.oh = oh, k.ow = ow;
    k.num_type = a->num_type, k.want_sq = a->sq ? 1 : 0, k.want_t = a->t0 ? 1 : 0, k.want_sum2 = a->sum2 ? 1 : 0;
    k.t0 = reinterpret_cast<double*>(b + o_t0), k.sum2 = reinterpret_cast<double*>(b + o_sum2);
    k.sq = reinterpret_cast<double*>(b + o_sq), k.rsq = a->rsq ? reinterpret_cast<double*>(b + o_rsq) : nullptr;
    k.st_pitch = st_pitch;
    k.blk = a->blk ? reinterpret_cast<double*>(b + o_blk) : nullptr;
    k.blkq = tail ? reinterpret_cast<double*>(b + o_blkq) : nullptr;
    k.blk_pitch = a->blk ? blk_pitch : 0, k.tail_s = a->tail_s;
    k.sb0 = sb0, k.sb1 = sb1;
    if (conv) {
        k.lay.u8 = b + o_u8, k.lay.u8b = b + o_u8b, k.lay.pitch = pitch;
        k.lay.r0 = a->lay_r0, k.lay.r1 = a->lay_r1;
    }
    if (a->zero_header) k.lay.zero16 = reinterpret_cast<unsigned long long*>(b + o_hdr);
    const int n_cus = c->n_cus > 0 ? c->n_cus : 256;
    int form = 0;           // the form the launch took: the caller's, or the launcher's rule
    int64_t ns = 0;
    MTMC(timed_launch(c->stream, [&] { return launch_stats_u8(c->stream, k, a->form, n_cus, &form); }, &ns));
    MTMC(fetch(a->t0, b + o_t0, st_bytes));
    MTMC(fetch(a->sum2, b + o_sum2, st_bytes));
    MTMC(fetch(a->sq, b + o_sq, st_bytes));
    MTMC(fetch(a->rsq, b + o_rsq, st_bytes));
    MTMC(fetch(a->blk, b + o_blk, rec_bytes));
    MTMC(fetch(a->blkq, b + o_blkq, rec_bytes));
    MTMC(fetch(a->u8, b + o_u8, (size_t)rows * pitch));
    MTMC(fetch(a->u8b, b + o_u8b, (size_t)rows * pitch));
    MTMC(fetch(a->header, b + o_hdr, 16));
    const int strips = (ow + stats_u8_owg(w) - 1) / stats_u8_owg(w);
    const int64_t info[8] = {st_pitch, blk_pitch, pitch, form, strips, stats_u8_grid_y(sb0, sb1, oh, kStatFormRows[form - 1]), n_cus, ns};
    std::memcpy(a->info, info, sizeof(info));
    return MTM_OK;
}

// Test support: the six other routes of stats_route (tests/test_gpu_stats_routes.py), each through the launcher launch_stats
// uses.  Everything lives in stats_dbg, filled with the caller's pattern first.  The image planes are laid out on the HOST
// exactly as an upload of that dtype leaves them (pitch = cols + 512 rounded up to 64, rows + kPadRows rows a plane, zero
// padding - 0x80 in the biased byte planes) and copied in one piece: the conversion kernels are not what is under test.
int mtm_debug_window_stats_route(mtm_ctx* c, const mtm_window_stats_route* a) {
    if (!c || !a) {
        set_error("mtm_debug_window_stats_route: null context or arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_debug_window_stats_route");
    const auto bad = [](const char* what) {
        set_error(std::string("mtm_debug_window_stats_route: ") + what);
        return MTM_E_INVALID;
    };
    const int rows = a->rows, cols = a->cols, chans = a->chans, h = a->h, w = a->w, dtype = a->dtype;
    if (!a->image || !a->info || rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || h < 1 || w < 1 || h > rows || w > cols)
        return bad("an image of 1 .. 16384 rows and columns and a window inside it are needed");
    if (chans < 1 || chans > kMaxChans || (dtype != MTM_U8 && dtype != MTM_U16 && dtype != MTM_F32))
        return bad("1 .. 4 channels of uint8, uint16 or float32");
    if (a->num_type < 0 || a->num_type > 2 || a->pattern_byte < 0 || a->pattern_byte > 255 || a->route < 0 ||
        a->route >= kStatsRouteCount || (a->want & ~31) != 0)
        return bad("num_type 0 .. 2, a route, the planes wanted and a pattern byte");
    const int route = a->route ? a->route : (int)stats_route(dtype, chans, h, w, cols, true);
    if (route == kStatsRouteU8) return bad("the fused single-channel uint8 kernel is mtm_debug_window_stats's");
    if (const char* why = stats_route_refusal(route, dtype, chans, h, w, cols)) return bad(why);
    const StatGeom g = stat_geom(rows, cols, chans, h, w);
    const int oh = g.oh, ow = g.ow, nsb = (oh + kStatBand4 - 1) / kStatBand4;
    const int sb0 = a->sb0, sb1 = a->sb1 < 0 ? nsb : std::min(a->sb1, nsb);
    if (sb0 < 0 || sb0 >= sb1) return bad("an empty range of row units");
    const bool part = a->lay_r1 > a->lay_r0;
    const bool ranged = route == kStatsRouteU16 || (route == kStatsRouteF64Lds && part);
    if (part && route != kStatsRouteF64Lds) return bad("image rows lay_r0 .. lay_r1: the F64_LDS route only");
    if (!ranged && (sb0 != 0 || sb1 != nsb)) return bad("a range of row units: the U16 route or a partial F64_LDS launch only");
    const int o0 = sb0 * kStatBand4, o1 = std::min(oh, sb1 * kStatBand4);
    if (part) {
        if (o0 % kVsumBand != 0) return bad("a partial F64_LDS launch starts on a whole band: sb0 * 8 a multiple of 32");
        if (a->lay_r0 < 0 || a->lay_r1 > rows || a->lay_r0 > o0) return bad("lay_r0 .. lay_r1 inside the image, lay_r0 <= sb0 * 8");
        if (a->lay_r1 < o1 + h - 1) return bad("lay_r1 < min(oh, sb1 * 8) + h - 1: the windows' last rows have no sums");
    }
    const bool want_t = a->want & 1, want_sum2 = a->want & 2, want_sq = a->want & 4, want_blk = a->want & 8, nulls = a->want & 16;
    const bool two_pass = route != kStatsRouteU8MC && route != kStatsRouteU16;
    if (want_blk && route != kStatsRouteU16) return bad("blk: the U16 route only");
    if (two_pass && nulls && !want_sum2) return bad("the two-pass chains write sum2 whatever is asked: it cannot be null");
    const int st_pitch = (int)round_up((size_t)ow, 4), blk_pitch = (st_pitch + 15) / 16;
    const int pitch = (int)round_up((size_t)cols + kPadCols, 64), rows_alloc = rows + kPadRows;
    // stats_dbg: [image planes][hs1][hs2][t0 .. t3][sum2][sq][blk]
    DebugArena ar;
    const bool bytes_in = route == kStatsRouteU8MC || route == kStatsRouteU8TwoPass || route == kStatsRouteU16;
    const size_t plane_elems = (size_t)pitch * rows_alloc;
    const int n_planes = route == kStatsRouteU16 ? 2 : chans;
    const size_t img_bytes = plane_elems * n_planes * (bytes_in ? 1 : sizeof(float));
    const bool u32_sums = route == kStatsRouteU8TwoPass || route == kStatsRouteU8TwoPassWide;
    const long long hs_plane = (long long)st_pitch * rows;
    const size_t hs_bytes = two_pass ? (u32_sums ? sizeof(uint32_t) : sizeof(double)) * (size_t)hs_plane * chans : 0;
    const size_t st_bytes = sizeof(double) * (size_t)st_pitch * oh, rec_bytes = sizeof(double) * 4 * (size_t)blk_pitch * oh;
    const size_t o_img = ar.take(img_bytes), o_hs1 = ar.take(hs_bytes), o_hs2 = ar.take(hs_bytes), o_t = ar.take(st_bytes * kMaxChans);
    const size_t o_sum2 = ar.take(st_bytes), o_sq = ar.take(st_bytes), o_blk = ar.take(rec_bytes);
    if (ar.total > ((size_t)256 << 20)) return bad("more than 256 MB of planes");
    // the planes, on the host
    std::vector<uint8_t> stage(img_bytes, route == kStatsRouteU16 ? 0x80 : 0);
    {
        const auto px = [&](int y, int x, int ch) -> double {
            const size_t i = ((size_t)y * cols + x) * chans + ch;
            return dtype == MTM_U8 ? (double)static_cast<const uint8_t*>(a->image)[i]
                 : dtype == MTM_U16 ? (double)static_cast<const uint16_t*>(a->image)[i]
                                    : (double)static_cast<const float*>(a->image)[i];
        };
        float* f = reinterpret_cast<float*>(stage.data());
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) {
                const size_t o = (size_t)y * pitch + x;
                if (route == kStatsRouteU16) {
                    const unsigned v = static_cast<const uint16_t*>(a->image)[(size_t)y * cols + x];
                    stage[o] = (uint8_t)((v >> 8) ^ 0x80u);
                    stage[plane_elems + o] = (uint8_t)((v & 255u) ^ 0x80u);
                } else {
                    for (int ch = 0; ch < chans; ++ch) {
                        if (bytes_in) stage[ch * plane_elems + o] = static_cast<const uint8_t*>(a->image)[((size_t)y * cols + x) * chans + ch];
                        else f[ch * plane_elems + o] = (float)px(y, x, ch);
                    }
                }
            }
    }
    HIPC(hipSetDevice(c->device));
    MTMC(c->stats_dbg.ensure(ar.total));
    uint8_t* b = c->stats_dbg.as<uint8_t>();
    HIPC(hipMemsetAsync(b, a->pattern_byte, ar.total, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipMemcpy(b + o_img, stage.data(), img_bytes, hipMemcpyHostToDevice));
    const StatScratch hs{b + o_hs1, b + o_hs2, st_pitch, hs_plane};
    StatOut o{};
    o.num_type = a->num_type, o.want_sq = want_sq, o.want_t = want_t, o.want_sum2 = want_sum2;
    for (int k = 0; k < kMaxChans; ++k)
        o.t[k] = (k < chans && (want_t || !nulls)) ? reinterpret_cast<double*>(b + o_t + st_bytes * k) : nullptr;
    o.t_plane = (long long)st_pitch * oh, o.st_pitch = st_pitch;
    o.sum2 = (want_sum2 || !nulls) ? reinterpret_cast<double*>(b + o_sum2) : nullptr;
    o.sq = (want_sq || !nulls) ? reinterpret_cast<double*>(b + o_sq) : nullptr;
    double* blk = want_blk ? reinterpret_cast<double*>(b + o_blk) : nullptr;
    const int owg = stats_u8_owg(w);
    const int hx = (ow + 256 * kHsumSeg - 1) / (256 * kHsumSeg), vx = (ow + 255) / 256, vy = (o1 - o0 + kVsumBand - 1) / kVsumBand;
    int64_t info[12] = {route, st_pitch, blk_pitch, pitch, 0, 0, 0, two_pass ? vx : 0, two_pass ? vy : 0, two_pass ? st_pitch : 0, 0, 0};
    const uint8_t* img8 = b + o_img;
    const float* img32 = reinterpret_cast<const float*>(b + o_img);
    const long long plane = (long long)plane_elems;
    const auto launch = [&]() -> int {
        switch (route) {
        case kStatsRouteU8MC:
            info[4] = (ow + owg - 1) / owg, info[5] = nsb, info[6] = 1;
            return launch_stats_u8mc(c->stream, img8, pitch, plane, g, o);
        case kStatsRouteU16:
            info[4] = (ow + owg - 1) / owg, info[5] = sb1 - sb0, info[6] = 1;
            return launch_stats_u16(c->stream, img8, img8 + plane_elems, pitch, g, o, blk, want_blk ? blk_pitch : 0, sb0, sb1);
        case kStatsRouteU8TwoPass:
            info[4] = rows, info[5] = chans, info[6] = 1, info[10] = (int64_t)(sizeof(uint32_t) * 2 * (cols + 1));
            return launch_stats_u8_2p(c->stream, img8, pitch, plane, g, hs, o);
        case kStatsRouteU8TwoPassWide:
            info[4] = hx, info[5] = rows, info[6] = chans;
            return launch_stats_u8_2p_wide(c->stream, img32, pitch, plane, g, hs, o);
        case kStatsRouteF64Lds:
            info[4] = hx, info[5] = part ? a->lay_r1 - a->lay_r0 : rows, info[6] = chans, info[10] = (int64_t)hsum_lds_bytes(w);
            return launch_stats_f64_lds(c->stream, img32, pitch, plane, g, hs, o, part ? a->lay_r0 : 0, part ? a->lay_r1 : rows, o0, o1);
        default:
            info[4] = hx, info[5] = rows, info[6] = chans;
            return launch_stats_f64(c->stream, img32, pitch, plane, g, hs, o);
        }
    };
    MTMC(timed_launch(c->stream, launch, &info[11]));
    double* const tout[kMaxChans] = {a->t0, a->t1, a->t2, a->t3};
    for (int k = 0; k < kMaxChans; ++k) MTMC(fetch(tout[k], b + o_t + st_bytes * k, st_bytes));
    MTMC(fetch(a->sum2, b + o_sum2, st_bytes));
    MTMC(fetch(a->sq, b + o_sq, st_bytes));
    MTMC(fetch(a->blk, b + o_blk, rec_bytes));
    std::memcpy(a->info, info, sizeof(info));
    return MTM_OK;
}

}  // extern "C"
