// libmtm_hip.so - many searchBoxes of one image in one call (mtm_find_matches_boxes): every (region, template)
// pair - a unit - gets the score map of its crop, computed tile by tile over the whole chip with the exact integer sums and
// the epilogue of every other score kernel (boxes_score_kernel: win_score_tile, mtm_k_window.hip.h), and the peak rules of mtm_find_matches applied to that map
// alone (boxes_peaks_kernel; 1-D and 1x1 maps on the host, as mtm_find_matches treats them).  uint8 (1 or 3 channels) and
// single-channel uint16, unmasked templates of one mtm_set_templates call.
#include "mtm_ctx.h"
#include "mtm_device_util.hip.h"
#include "mtm_k_window.hip.h"

using namespace mtm;
using namespace mtmi;

namespace mtm {

// A unit as the kernels see it: its template, the image pixel of its map's output (0, 0), the map's size and place in the
// chunk's score buffer (row-major, ow floats per row).
struct BoxUnit {
    int t;
    int y0, x0;
    int oh, ow;
    long long buf_off;
};

// One 16 x 16 tile of outputs of unit u (an index into the chunk's unit table), first output (ty0, tx0) of its map.
struct BoxTile {
    int u, ty0, tx0;
};

// Grid: one work-group per tile of the chunk's tile table, so that a large region spreads over the chip and many small
// ones fill it together.  win_score_tile sums the tile's windows straight from the image's planes (a unit's outputs only
// read pixels of its region) and finishes them: the exhaustive map's float32 values, stored into the unit's map.
template <int CH, bool U16>
__global__ __launch_bounds__(256) void boxes_score_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                          const uint8_t* __restrict__ tpx, const long long* __restrict__ toff,
                                                          const TemplDev* __restrict__ td, const BoxUnit* __restrict__ units,
                                                          const BoxTile* __restrict__ tiles, float* __restrict__ buf,
                                                          int method) {
    __shared__ __attribute__((aligned(16))) WinTemplLds Tl[U16 ? 2 : 1];
    __shared__ __attribute__((aligned(16))) WinImageLds Il[U16 ? 2 : 1];
    const BoxTile K = tiles[blockIdx.x];
    const BoxUnit U = units[K.u];
    const TemplDev T = td[U.t];
    win_score_tile<CH, U16>(Tl, Il, img, lo_b, tpx + toff[U.t], T, U.y0 + K.ty0, U.x0 + K.tx0, K.ty0, K.tx0, U.oh, U.ow, method,
                            [&](bool inside, int y, int x, auto&& score) {
                                if (inside) buf[U.buf_off + (long long)y * U.ow + x] = score();
                            });
}

// Grid: the tiles again (local mode: only those of units with 2-D maps).  Per output of the unit's own map:
//   local mode  - the peak test of peaks_kernel (v == max of its 3x3 neighbourhood, the unit map's edges padded by the
//                 border rule `border`, v > thr_q in quality space); nontrivial[u] records that some output of the unit
//                 differs from its neighbourhood's maximum.  Records carry the unit index in templ_idx.
//   global mode - the unit's best (quality, first in row-major order) output into best[u] (atomicMax on
//                 order(quality) << 32 | ~index, as extremum_kernel keys it).
__global__ __launch_bounds__(256) void boxes_peaks_kernel(const BoxUnit* __restrict__ units, const BoxTile* __restrict__ tiles,
                                                          const float* __restrict__ buf, const TemplDev* __restrict__ td,
                                                          int mode_min, int global, float thr_q, int border,
                                                          mtm_hit* __restrict__ hits, unsigned long long cap,
                                                          unsigned long long* __restrict__ counter,
                                                          unsigned long long* __restrict__ best, int* __restrict__ nontrivial) {
    const BoxTile K = tiles[blockIdx.x];
    const BoxUnit U = units[K.u];
    const int tid = threadIdx.x;
    const int y = K.ty0 + tid / kWinTile, x = K.tx0 + tid % kWinTile;
    const bool on = y < U.oh && x < U.ow;
    const float* m = buf + U.buf_off;
    const float padv = (border == MTM_BORDER_CONSTANT) ? 0.0f : -INFINITY;
    auto q_at = [&](int yy, int xx) -> float {      // quality at output (yy, xx) of the unit's map; the pad value outside it
        if (yy < 0 || yy >= U.oh || xx < 0 || xx >= U.ow) return padv;
        const float s = m[(long long)yy * U.ow + xx];
        return mode_min ? -s : s;
    };
    const float v = on ? q_at(y, x) : padv;
    if (global) {
        unsigned long long key = 0ull;
        if (on)
            key = ((unsigned long long)mf_float_order(v) << 32) |
                  (0xFFFFFFFFull - (unsigned long long)((long long)y * U.ow + x));
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off);
            key = o > key ? o : key;
        }
        if ((tid & 63) == 0 && key != 0ull) atomicMax(best + K.u, key);
        return;
    }
    bool emit = false;
    int nontriv = 0;
    if (on) {
        float mx = v;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) mx = fmaxf(mx, q_at(y + dy, x + dx));
        if (!(v == mx)) nontriv = 1;
        else emit = v > thr_q;
    }
    mtm_hit rec;
    rec.templ_idx = K.u;
    rec.x = x;
    rec.y = y;
    rec.w = td[U.t].cols;
    rec.h = td[U.t].rows;
    rec.score = mode_min ? -v : v;
    cand_append(emit, counter, cap, hits, rec);
    if (__syncthreads_or(nontriv) && tid == 0) nontrivial[K.u] = 1;
}

}  // namespace mtm

namespace mtmi {

// The epilogue constants of mtm_set_templates' statistics for every template, uploaded once per template set (also
// mtm_track_boxes').
int prepare_box_td(mtm_ctx* c, const std::vector<BlobTempl>& tl) {
    if (c->box_gen == c->templ_gen) return MTM_OK;
    const int n = (int)tl.size();
    if ((int)c->templs.size() != n) {
        set_error("mtm_find_matches_boxes: template set and its statistics differ in size");
        return MTM_E_STATE;
    }
    c->box_gen = 0;
    std::vector<TemplDev> td((size_t)n, TemplDev{});
    for (int i = 0; i < n; ++i) {
        const HostTempl& ht = c->templs[(size_t)i];
        TemplDev& d = td[(size_t)i];
        for (int k = 0; k < kMaxChans; ++k) d.mean[k] = ht.st.mean[k];
        d.templ_norm = ht.st.templ_norm;
        d.templ_sum2 = ht.st.templ_sum2;
        d.all_ones = ht.st.all_ones;
        d.rows = tl[(size_t)i].rows;
        d.cols = tl[(size_t)i].cols;
    }
    if (n > 0) {
        MTMC(c->box_td.ensure(sizeof(TemplDev) * (size_t)n));
        HIPC(hipMemcpy(c->box_td.p, td.data(), sizeof(TemplDev) * (size_t)n, hipMemcpyHostToDevice));
    }
    c->box_gen = c->templ_gen;
    return MTM_OK;
}

}  // namespace mtmi

namespace {

// Units u0 .. u1 - 1 (whole units, their maps within the memory budget): maps, peaks, records.  Appends the records of
// each unit, in mtm_find_matches' order and image coordinates, to `hits`, and their number to counts[u].
int boxes_chunk(mtm_ctx* c, const mtm_box_unit* units, const std::vector<BlobTempl>& tl, int u0, int u1, int chans,
                int dtype, int mode, float thr, std::vector<mtm_hit>& hits, int64_t* counts) {
    const int nu = u1 - u0;
    const bool mode_min = method_mode_min(c->method);
    const bool global = mode == MTM_PEAKS_GLOBAL;
    // unit table: the maps of 2-D units first, those of 1-D / 1x1 units after them in one block (local mode reads that
    // block back for the host's rules in one copy); tile table: the tiles of 2-D units first (the peak kernel's grid in
    // local mode)
    std::vector<BoxUnit> bu((size_t)nu);
    std::vector<BoxTile> tiles;
    long long off = 0, off1d = 0;
    size_t n_tiles_2d = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            off1d = off;
            n_tiles_2d = tiles.size();
        }
        for (int k = 0; k < nu; ++k) {
            const mtm_box_unit& s = units[u0 + k];
            const BlobTempl& t = tl[(size_t)s.templ_idx];
            BoxUnit& b = bu[(size_t)k];
            b.t = s.templ_idx;
            b.y0 = s.y0;
            b.x0 = s.x0;
            b.oh = s.rows - t.rows + 1;
            b.ow = s.cols - t.cols + 1;
            const bool line = b.oh <= 1 || b.ow <= 1;
            if (line != (pass == 1)) continue;
            b.buf_off = off;
            off += (long long)b.oh * b.ow;
            for (int ty = 0; ty < b.oh; ty += kWinTile)
                for (int tx = 0; tx < b.ow; tx += kWinTile) tiles.push_back(BoxTile{k, ty, tx});
        }
    }
    const long long n1d_floats = off - off1d;
    MTMC(c->box_units.ensure(sizeof(BoxUnit) * bu.size()));
    MTMC(c->box_tiles.ensure(sizeof(BoxTile) * tiles.size()));
    MTMC(c->win_buf.ensure(sizeof(float) * (size_t)off));
    HIPC(hipMemcpyAsync(c->box_units.p, bu.data(), sizeof(BoxUnit) * bu.size(), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->box_tiles.p, tiles.data(), sizeof(BoxTile) * tiles.size(), hipMemcpyHostToDevice, c->stream));

    const ImageDev img = image_dev(c);
    const uint8_t* lo_b = c->slot[c->cur].u8b.as<uint8_t>() + img.u8_plane;     // uint16: [high ^ 0x80][low ^ 0x80]
    // (both kernels run over the tile table in launch slices, for_launch_slices)
    MTMC(for_launch_slices(0, tiles.size(), [&](size_t t0, unsigned nt) -> int {
        const auto launch_score = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(nt), dim3(256), 0, c->stream, img, lo_b, c->win_tpx.as<uint8_t>(),
                               c->win_toff.as<long long>(), c->box_td.as<TemplDev>(), c->box_units.as<BoxUnit>(),
                               c->box_tiles.as<BoxTile>() + t0, c->win_buf.as<float>(), c->method);
        };
        if (dtype == MTM_U16) launch_score(boxes_score_kernel<1, true>);
        else if (chans == 1) launch_score(boxes_score_kernel<1, false>);
        else launch_score(boxes_score_kernel<3, false>);
        HIPC(hipGetLastError());
        return MTM_OK;
    }));

    std::vector<float> maps1d(global ? 0 : (size_t)n1d_floats);
    const size_t peak_tiles = global ? tiles.size() : n_tiles_2d;
    bool first = true;
    std::vector<mtm_hit> ch;            // this chunk's records, templ_idx = the unit's index in the chunk, unit coordinates
    auto launch = [&](mtm_hit* dhits, unsigned long long cap, unsigned long long* counter, unsigned long long* best,
                      int* nontrivial) -> int {
        MTMC(for_launch_slices(0, peak_tiles, [&](size_t t0, unsigned nt) -> int {
            hipLaunchKernelGGL(boxes_peaks_kernel, dim3(nt), dim3(256), 0, c->stream, c->box_units.as<BoxUnit>(),
                               c->box_tiles.as<BoxTile>() + t0, c->win_buf.as<float>(), c->box_td.as<TemplDev>(),
                               mode_min ? 1 : 0, global ? 1 : 0, mode_min ? -thr : thr, c->opt_border, dhits, cap, counter,
                               best, nontrivial);
            HIPC(hipGetLastError());
            return MTM_OK;
        }));
        if (first && !maps1d.empty())
            HIPC(hipMemcpyAsync(maps1d.data(), c->win_buf.as<float>() + off1d, sizeof(float) * maps1d.size(),
                                hipMemcpyDeviceToHost, c->stream));
        first = false;
        return MTM_OK;
    };
    std::vector<unsigned long long> best;
    MTMC(window_peak_pass(c, nu, global, launch, best, ch, "mtm_find_matches_boxes"));
    if (global) {
        for (int k = 0; k < nu; ++k) {
            const BoxUnit& b = bu[(size_t)k];
            ch.push_back(decode_quality_key(best[(size_t)k], mode_min, k, b.ow, tl[(size_t)b.t].cols, tl[(size_t)b.t].rows));
        }
    } else {
        // 1-D and 1x1 unit maps (MTM/__init__.py:25-41), as mtm_find_matches treats a whole map of that shape
        for (int k = 0; k < nu; ++k) {
            const BoxUnit& b = bu[(size_t)k];
            if (b.oh > 1 && b.ow > 1) continue;
            line_map_peaks(maps1d.data() + (b.buf_off - off1d), b.oh, b.ow, thr, mode_min, k, tl[(size_t)b.t].cols,
                           tl[(size_t)b.t].rows, ch);
        }
        sort_hits(ch, mode_min);
    }
    for (mtm_hit h : ch) {
        const BoxUnit& b = bu[(size_t)h.templ_idx];
        ++counts[u0 + h.templ_idx];
        h.templ_idx = b.t;
        h.x += b.x0;
        h.y += b.y0;
        hits.push_back(h);
    }
    return MTM_OK;
}

}  // namespace

extern "C" {

int mtm_find_matches_boxes(mtm_ctx* c, const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                           const mtm_box_unit* units, int n_units, int mode, double score_threshold, mtm_hit* out,
                           int64_t capacity, int64_t* counts, int64_t* n_out) {
    const char* who = "mtm_find_matches_boxes";
    if (!c || !n_out || n_units < 0 || (n_units > 0 && (!units || !counts)) || capacity < 0 || (capacity > 0 && !out) ||
        (mode != MTM_PEAKS_LOCAL && mode != MTM_PEAKS_GLOBAL)) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, who));
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        set_error(std::string(who) + ": takes uint8 images with 1 or 3 channels and single-channel uint16 images");
        return MTM_E_INVALID;
    }
    if (!c->have_templ) {
        set_error(std::string(who) + ": no templates set");
        return MTM_E_STATE;
    }
    std::vector<BlobTempl> tl;
    MTMC(parse_templ_blob(c->templ_blob, tl, who, true));
    for (int u = 0; u < n_units; ++u) {
        const mtm_box_unit& s = units[u];
        const std::string where = std::string(who) + ": unit " + std::to_string(u);
        if (s.templ_idx < 0 || s.templ_idx >= (int)tl.size()) {
            set_error(where + ": template index out of range");
            return MTM_E_INVALID;
        }
        if (s.y0 < 0 || s.x0 < 0 || s.rows < 1 || s.cols < 1 || s.rows > rows - s.y0 || s.cols > cols - s.x0) {
            set_error(where + ": region outside the image");
            return MTM_E_INVALID;
        }
        const BlobTempl& t = tl[(size_t)s.templ_idx];
        if (t.dtype != dtype || t.chans != chans) {
            set_error(where + ": template and image differ in pixel type or channel count");
            return MTM_E_INVALID;
        }
        if (t.rows > s.rows || t.cols > s.cols) {
            set_error(where + ": template larger than the region");
            return MTM_E_INVALID;
        }
        // (uint16: correlations of up to 2^21 pixels stay below 2^53, exact in float64 as the exhaustive kernels need)
        if (dtype == MTM_U16 && (long long)t.rows * t.cols > (1ll << 21)) {
            set_error(where + ": uint16 template of more than 2^21 pixels");
            return MTM_E_INVALID;
        }
    }
    *n_out = 0;
    for (int u = 0; u < n_units; ++u) counts[u] = 0;
    HIPC(hipSetDevice(c->device));
    MTMC(prepare_window_templates(c, tl));
    MTMC(prepare_box_td(c, tl));

    // ONE upload of the image; every unit reads its region from the same planes
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    MTMC(upload_image(c, c->slot[c->cur], px, row_stride_bytes, rows, cols, chans, dtype, c->stream, 1));
    adopt_image(c, rows, cols, chans, dtype);

    const float thr = (float)score_threshold;       // numpy compares the float32 map with the threshold in float32
    std::vector<mtm_hit> hits;
    for (int u0 = 0; u0 < n_units;) {
        // whole units while their maps fit the budget (at least one)
        long long floats = 0;
        int u1 = u0;
        while (u1 < n_units) {
            const BlobTempl& t = tl[(size_t)units[u1].templ_idx];
            const long long f = (long long)(units[u1].rows - t.rows + 1) * (units[u1].cols - t.cols + 1);
            if (u1 > u0 && floats + f > c->boxes_max_floats) break;
            floats += f;
            ++u1;
        }
        MTMC(boxes_chunk(c, units, tl, u0, u1, chans, dtype, mode, thr, hits, counts));
        u0 = u1;
    }
    c->timing.n_hits = (int64_t)hits.size();
    return publish_hits(hits, c->last_hits, out, capacity, n_out, std::string(who) + ": output capacity too small");
}

}  // extern "C"
