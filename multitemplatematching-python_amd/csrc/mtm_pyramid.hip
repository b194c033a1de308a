// libmtm_hip.so - coarse-to-fine search (mtm_find_matches_pyramid): the local extrema of a downscaled search
// propose candidates, full-resolution scores are computed only in small windows around them (pyr_window_kernel), with the
// exact integer sums and the epilogue of every other score kernel, and the peak test of the exhaustive search is applied
// there.  uint8, unmasked templates of one mtm_set_templates call.
#include "mtm_ctx.h"
#include "mtm_device_util.hip.h"
#include "mtm_k_window.hip.h"

using namespace mtm;
using namespace mtmi;

namespace mtm {

// One candidate window of a template: the full-resolution positions it stands for and the region scored for them (the
// window and a one-pixel ring, both clipped to the score map).  A template's windows are consecutive, best candidate first.
struct PyrWin {
    int t;                      // template index
    int first;                  // index of the template's first window in the list
    int y0, y1, x0, x1;         // window (inclusive bounds)
    int ry0, ry1, rx0, rx1;     // scored region (inclusive bounds)
    long long buf_off;          // float offset of the region's scores in the score buffer, row-major, rx1 - rx0 + 1 per row
};

// Grid: one work-group per window.  Phase 1 scores the region tile by tile: per output the exact correlation and the
// window sums S1 (per channel) and S2 come from v_dot4_u32_u8 over a template chunk and an image tile in LDS (the
// template streams through LDS chunk by chunk, so its size is not bounded by LDS), then window_norm and
// finish_unmasked_with make the float32 score exactly as the exhaustive kernels do.  Phase 2 reads the region back:
//   local mode  - the peak test of peaks_kernel (v == max of its 3x3 neighbourhood, border rule `border`, v > thr_q in
//                 quality space) on the window's positions; a position another window of the same template listed earlier
//                 also covers is left to that window, so every position is emitted once.  nontrivial[t] records that some
//                 position of the window differs from its neighbourhood's maximum.
//   global mode - the best (quality, first in row-major order) position over the window into best[t] (atomicMax on
//                 order(quality) << 32 | ~index, as extremum_kernel keys it).
template <int CH>
__global__ __launch_bounds__(256) void pyr_window_kernel(ImageDev img, const uint8_t* __restrict__ tpx,
                                                         const long long* __restrict__ toff, const TemplDev* __restrict__ td,
                                                         const PyrWin* __restrict__ wins, float* __restrict__ buf, int method,
                                                         int mode_min, int global, float thr_q, int border,
                                                         mtm_hit* __restrict__ hits, unsigned long long cap,
                                                         unsigned long long* __restrict__ counter,
                                                         unsigned long long* __restrict__ best,
                                                         int* __restrict__ nontrivial) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl;
    __shared__ __attribute__((aligned(16))) WinImageLds Il;
    const PyrWin W = wins[blockIdx.x];
    const TemplDev T = td[W.t];
    const int h = T.rows, w = T.cols;
    const uint8_t* tp = tpx + toff[W.t];
    const int tid = threadIdx.x, ly = tid / kWinTile, lx = tid % kWinTile;
    const int RH = W.ry1 - W.ry0 + 1, RW = W.rx1 - W.rx0 + 1;
    float* rb = buf + W.buf_off;
    const double inv_area = 1.0 / ((double)h * (double)w);

    for (int ty0 = 0; ty0 < RH; ty0 += kWinTile)
        for (int tx0 = 0; tx0 < RW; tx0 += kWinTile) {
            unsigned long long corr, s2, s1[CH];
            // (the tile's first output = its window's top-left pixel)
            win_tile_sums_u8<CH>(Tl, Il, img.u8, img.u8_plane, img.u8_pitch, img.rows, img.cols, tp, h, w, W.ry0 + ty0,
                                 W.rx0 + tx0, corr, s1, s2);
            if (ty0 + ly < RH && tx0 + lx < RW) {
                const float score = win_score<CH>(method, T, inv_area, corr, s1, s2);
                rb[(size_t)(ty0 + ly) * RW + tx0 + lx] = score;
            }
        }
    __syncthreads();            // the region's scores are visible to the whole work-group

    const float padv = (border == MTM_BORDER_CONSTANT) ? 0.0f : -INFINITY;
    auto q_at = [&](int y, int x) -> float {        // quality at map position (y, x); the pad value outside the map
        if (y < 0 || y >= T.oh || x < 0 || x >= T.ow) return padv;
        const float s = rb[(size_t)(y - W.ry0) * RW + (x - W.rx0)];
        return mode_min ? -s : s;
    };
    const int WH = W.y1 - W.y0 + 1, WW = W.x1 - W.x0 + 1;
    int nontriv = 0;
    unsigned long long bk = 0ull;
    for (int k = tid; k < WH * WW; k += 256) {
        const int y = W.y0 + k / WW, x = W.x0 + k % WW;
        const float v = q_at(y, x);
        bool emit = false;
        if (global) {
            const unsigned long long key = ((unsigned long long)mf_float_order(v) << 32) |
                                           (0xFFFFFFFFull - (unsigned long long)((long long)y * T.ow + x));
            bk = key > bk ? key : bk;
        } else {
            float mx = v;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) mx = fmaxf(mx, q_at(y + dy, x + dx));
            if (!(v == mx)) {
                nontriv = 1;
            } else if (v > thr_q) {
                emit = true;
                for (int j = W.first; j < (int)blockIdx.x; ++j)
                    if (y >= wins[j].y0 && y <= wins[j].y1 && x >= wins[j].x0 && x <= wins[j].x1) {
                        emit = false;
                        break;
                    }
            }
        }
        mtm_hit rec;
        rec.templ_idx = W.t;
        rec.x = x;
        rec.y = y;
        rec.w = w;
        rec.h = h;
        rec.score = mode_min ? -v : v;
        cand_append(emit, counter, cap, hits, rec);
    }
    if (global) {
        if (bk != 0ull) atomicMax(best + W.t, bk);
    } else if (__syncthreads_or(nontriv) && tid == 0) {
        nontrivial[W.t] = 1;
    }
}

}  // namespace mtm

namespace {

// augment.downscale / planarize_u8_down_kernel on the host: factor 2 -> (sum + 2) >> 2, else rint((float)sum / f^2)
std::vector<uint8_t> downscale_u8(const BlobTempl& t, int f) {
    const int r = t.rows / f, cc = t.cols / f, C = t.chans;
    std::vector<uint8_t> o((size_t)r * cc * C);
    const float scale = 1.0f / (float)(f * f);
    for (int y = 0; y < r; ++y)
        for (int x = 0; x < cc; ++x)
            for (int c = 0; c < C; ++c) {
                unsigned sum = 0;
                for (int dy = 0; dy < f; ++dy)
                    for (int dx = 0; dx < f; ++dx) sum += t.px[((size_t)(y * f + dy) * t.cols + (size_t)x * f + dx) * C + c];
                const unsigned v = (f == 2) ? ((sum + 2u) >> 2) : (unsigned)rintf((float)sum * scale);
                o[((size_t)y * cc + x) * C + c] = (uint8_t)(v > 255u ? 255u : v);
            }
    return o;
}

}  // namespace

extern "C" {

int mtm_find_matches_pyramid(mtm_ctx* c, const void* px, int rows, int cols, int chans, int dtype,
                             int64_t row_stride_bytes, int factor, int mode, double coarse_threshold,
                             double score_threshold, int radius, int max_candidates, mtm_hit* out, int64_t capacity,
                             int64_t* n_out) {
    const char* who = "mtm_find_matches_pyramid";
    if (!c || !n_out || capacity < 0 || (capacity > 0 && !out) || (mode != MTM_PEAKS_LOCAL && mode != MTM_PEAKS_GLOBAL) ||
        factor < 2 || factor > 64 || radius < 0 || max_candidates < 1) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, who));
    if (dtype != MTM_U8) {
        set_error(std::string(who) + ": takes uint8 images");
        return MTM_E_INVALID;
    }
    if (!c->have_templ) {
        set_error(std::string(who) + ": no templates set");
        return MTM_E_STATE;
    }
    if (c->method == MTM_TM_SQDIFF) {
        set_error(std::string(who) + ": TM_SQDIFF is not supported");
        return MTM_E_INVALID;
    }
    std::vector<BlobTempl> tl;
    MTMC(parse_templ_blob(c->templ_blob, tl, who, false));
    const int n = (int)tl.size();
    const int crows = rows / factor, ccols = cols / factor;
    for (int i = 0; i < n; ++i) {
        const BlobTempl& t = tl[(size_t)i];
        const int hc = t.rows / factor, wc = t.cols / factor;
        if (t.chans != chans || hc < 2 || wc < 2 || crows - hc + 1 < 2 || ccols - wc + 1 < 2 || rows - t.rows + 1 < 2 ||
            cols - t.cols + 1 < 2) {
            set_error(std::string(who) + ": template " + std::to_string(i) +
                      ": channel count differs from the image, or its coarse template / a score map is smaller than 2x2");
            return MTM_E_INVALID;
        }
    }
    HIPC(hipSetDevice(c->device));
    if (!c->pyr_sub) MTMC(mtm_ctx_create(&c->pyr_sub, c->device));
    mtm_ctx* s = c->pyr_sub;
    s->opt_border = c->opt_border;
    MTMC(prepare_window_templates(c, tl));
    if (c->pyr_factor != factor || c->pyr_gen != c->templ_gen) {
        // the coarse templates (the coarse context's set)
        c->pyr_gen = 0;
        std::vector<std::vector<uint8_t>> coarse((size_t)n);
        std::vector<mtm_templ> recs((size_t)n);
        for (int i = 0; i < n; ++i) {
            const BlobTempl& t = tl[(size_t)i];
            coarse[(size_t)i] = downscale_u8(t, factor);
            mtm_templ& r = recs[(size_t)i];
            r.px = coarse[(size_t)i].data();
            r.mask = nullptr;
            r.rows = t.rows / factor;
            r.cols = t.cols / factor;
            r.chans = t.chans;
            r.dtype = MTM_U8;
            r.row_stride = (int64_t)r.cols * r.chans;
            r.mask_row_stride = 0;
        }
        MTMC(mtm_set_templates(s, recs.data(), n, c->method));
        c->pyr_gen = c->templ_gen;
        c->pyr_factor = factor;
    }

    // ONE upload: the full-resolution planes, and the coarse planes derived on the device from the same raw copy
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    MTMC(upload_image(c, c->slot[c->cur], px, row_stride_bytes, rows, cols, chans, MTM_U8, c->stream, 1));
    adopt_image(c, rows, cols, chans, MTM_U8);
    MTMC(derive_downscaled_u8(s, c->slot[c->cur], rows, cols, chans, factor, c->stream));
    HIPC(hipStreamSynchronize(c->stream));

    // coarse level: the local extrema of the downscaled search that pass coarse_threshold, in mtm_find_matches' order
    std::vector<mtm_hit> ch(4096);
    int64_t nc = 0;
    int rc = mtm_find_matches(s, MTM_PEAKS_LOCAL, coarse_threshold, ch.data(), (int64_t)ch.size(), &nc);
    if (rc == MTM_E_OVERFLOW) {
        ch.resize((size_t)nc);
        rc = mtm_last_hits(s, ch.data(), nc, &nc);
    }
    if (rc != MTM_OK) return rc;
    ch.resize((size_t)nc);

    // windows: the best max_candidates of every template (the list is ordered by quality, ties row-major)
    MTMC(place_templates(c));
    std::vector<PyrWin> wins;
    long long buf_floats = 0;
    int cur_t = -1, taken = 0, first = 0;
    for (const mtm_hit& hc : ch) {
        if (hc.templ_idx != cur_t) {
            cur_t = hc.templ_idx;
            taken = 0;
            first = (int)wins.size();
        }
        if (taken >= max_candidates) continue;
        ++taken;
        const TemplDev& d = c->td_host[(size_t)cur_t];
        const long long cy = (long long)hc.y * factor, cx = (long long)hc.x * factor;
        const int y0 = (int)std::max(0LL, cy - radius), y1 = (int)std::min((long long)d.oh - 1, cy + radius);
        const int x0 = (int)std::max(0LL, cx - radius), x1 = (int)std::min((long long)d.ow - 1, cx + radius);
        if (y0 > y1 || x0 > x1) continue;
        PyrWin W;
        W.t = cur_t;
        W.first = first;
        W.y0 = y0;
        W.y1 = y1;
        W.x0 = x0;
        W.x1 = x1;
        W.ry0 = std::max(0, y0 - 1);
        W.ry1 = std::min(d.oh - 1, y1 + 1);
        W.rx0 = std::max(0, x0 - 1);
        W.rx1 = std::min(d.ow - 1, x1 + 1);
        W.buf_off = buf_floats;
        buf_floats += (long long)(W.ry1 - W.ry0 + 1) * (W.rx1 - W.rx0 + 1);
        wins.push_back(W);
    }
    if (buf_floats > (1LL << 30)) {
        set_error(std::string(who) + ": the candidate windows need more than 2^30 scores (lower radius or max_candidates)");
        return MTM_E_INVALID;
    }

    const bool mode_min = c->method == MTM_TM_SQDIFF_NORMED;
    const bool global = mode == MTM_PEAKS_GLOBAL;
    std::vector<mtm_hit> hits;
    if (!wins.empty()) {
        MTMC(c->pyr_wins.ensure(sizeof(PyrWin) * wins.size()));
        HIPC(hipMemcpyAsync(c->pyr_wins.p, wins.data(), sizeof(PyrWin) * wins.size(), hipMemcpyHostToDevice, c->stream));
        MTMC(c->win_buf.ensure(sizeof(float) * (size_t)buf_floats));
        const float thr = (float)score_threshold;       // numpy compares the float32 map with the threshold in float32
        const ImageDev img = image_dev(c);
#define MTM_PYR_LAUNCH(CH)                                                                                                  \
    hipLaunchKernelGGL(pyr_window_kernel<CH>, dim3((unsigned)wins.size()), dim3(256), 0, c->stream, img,                    \
                       c->win_tpx.as<uint8_t>(), c->win_toff.as<long long>(), c->td.as<TemplDev>(), c->pyr_wins.as<PyrWin>(), \
                       c->win_buf.as<float>(), c->method, mode_min ? 1 : 0, global ? 1 : 0, mode_min ? -thr : thr,           \
                       c->opt_border, dhits, cap, counter, best, nontrivial)
        auto launch = [&](mtm_hit* dhits, unsigned long long cap, unsigned long long* counter, unsigned long long* best,
                          int* nontrivial) -> int {
            switch (chans) {
                case 1: MTM_PYR_LAUNCH(1); break;
                case 2: MTM_PYR_LAUNCH(2); break;
                case 3: MTM_PYR_LAUNCH(3); break;
                default: MTM_PYR_LAUNCH(4); break;
            }
            HIPC(hipGetLastError());
            return MTM_OK;
        };
#undef MTM_PYR_LAUNCH
        std::vector<unsigned long long> best;
        MTMC(window_peak_pass(c, n, global, launch, best, hits, who));
        if (global) {
            for (int t = 0; t < n; ++t) {
                if (best[(size_t)t] == 0ull) continue;
                const TemplDev& d = c->td_host[(size_t)t];
                hits.push_back(decode_quality_key(best[(size_t)t], mode_min, t, d.ow, d.cols, d.rows));
            }
        } else {
            sort_hits(hits, mode_min);
        }
    }
    c->timing.n_hits = (int64_t)hits.size();
    return publish_hits(hits, c->last_hits, out, capacity, n_out, std::string(who) + ": output capacity too small");
}

}  // extern "C"
