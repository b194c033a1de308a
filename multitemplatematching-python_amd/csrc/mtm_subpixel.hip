// libmtm_hip.so - the 3 x 3 score neighbourhoods of a list of hits (mtm_hit_neighbourhoods): for every point
// (template t, window x, y) the scores of t at windows (x + dx, y + dy), dx, dy in {-1, 0, 1}, of the current image's map,
// NaN outside it.  One launch scores the nine windows of every point: a tile kernel would compute 256 outputs to keep 9,
// so the work is split over the template's pixels instead (split-K) and reduced once per point.
//   uint8 (1 or 3 channels, masked or not) and single-channel uint16: exact integer sums (v_dot4_u32_u8), finished by
//     win_score (unmasked, as boxes_score_kernel feeds it) or finish_masked with IEEE division - mtm_score_map's values bit
//     for bit in the default MTM_OPT_EXACT_DIV mode.
//   float32 (1 or 3 channels, masked or not): float64 FMAs against the float64 weights the exhaustive float64 kernel reads
//     (K1 = T, or T M^2 and K2 = M^2 with a mask), window sums taken directly in float64.  The exhaustive route's window
//     statistics are sliding sums whose segments and bands depend on the map's origin, so these scores agree with
//     mtm_score_map to rounding (1e-6 relative), not bit for bit; flat windows (normalisation guard) may differ outright.
#include "mtm_ctx.h"
#include "mtm_device_util.hip.h"
#include "mtm_k_nbhd.hip.h"

using namespace mtm;
using namespace mtmi;

namespace mtm {

// A template as the neighbourhood kernel reads it: its epilogue constants and where its operands are.
//   px_off: bytes in the byte arena - uint8: planar [C][h][w] of T (masked: T * M, M binary), uint16: the high-byte plane
//           then the low-byte plane; mk_off: the mask's bytes 0xFF / 0x00 [C][h][w] (masked uint8), else -1.
//   k1_off / k2_off: doubles in the weight arena, planar [C][h][w] (float32 images): K1 = T or T M^2, K2 = M^2 or -1.
struct SubTempl {
    TemplDev T;
    long long px_off, mk_off, k1_off, k2_off;
};

// One point: a template and the window (x, y) at the centre of its neighbourhood.
struct SubPoint {
    int t, x, y;
};

constexpr int kSubFW = kSubC + 2;                   // floats per LDS image row (float32)
constexpr size_t kSubLaunchPoints = (size_t)1 << 22; // most work-groups (points) of one launch

typedef float SubImageLdsF[kSubLdsR][kSubFW];

__device__ __forceinline__ void sub_load_image_f(SubImageLdsF& Il, const float* __restrict__ ip, int pitch, int rows, int cols,
                                                 int y0, int x0, int tid) {
    for (int k = tid; k < kSubLdsR * kSubFW; k += 256) {
        const int i = k / kSubFW, j = k % kSubFW;
        const int y = y0 + i, x = x0 + j;
        Il[i][j] = (y >= 0 && y < rows && x >= 0 && x < cols) ? ip[(size_t)y * pitch + x] : 0.0f;
    }
}

// Grid: one 256-thread work-group per point (launch slice).  uint8 / uint16: sub_nbhd_int (mtm_k_nbhd.hip.h).  float32:
// each chunk of kSubR x kSubC template pixels gives every thread four pixels of it; the thread adds their products with the
// nine windows' image pixels, staged in LDS as the chunk's (kSubR + 2) x (kSubC + 2) patch, to its own nine correlations
// and window sums in float64; the work-group's sums are reduced in a fixed order and threads 0 .. 8 finish window
// (dy, dx) = (k / 3 - 1, k % 3 - 1).
template <int CH, int KIND>
__global__ __launch_bounds__(256) void sub_nbhd_kernel(ImageDev img, const uint8_t* __restrict__ lo_b,
                                                       const uint8_t* __restrict__ bytes, const double* __restrict__ wts,
                                                       const SubTempl* __restrict__ st, const SubPoint* __restrict__ pts,
                                                       float* __restrict__ out, int method) {
    constexpr bool kInt = KIND == kSubU8 || KIND == kSubU8Mask || KIND == kSubU16;
    const SubPoint P = pts[blockIdx.x];
    const SubTempl S = st[P.t];
    const int tid = threadIdx.x;
    if constexpr (kInt) {
        __shared__ __attribute__((aligned(16))) WinTemplLds Tl[KIND == kSubU8 ? 1 : 2];
        __shared__ __attribute__((aligned(16))) SubImageLds Il[KIND == kSubU16 ? 2 : 1];
        __shared__ unsigned long long red[4];
        const float score = sub_nbhd_int<CH, KIND>(Tl, Il, red, img.u8, img.u8_plane, lo_b, img.u8_pitch, img.rows, img.cols,
                                                   bytes + S.px_off, bytes + S.mk_off, S.T, P.x, P.y, method);
        if (tid < 9) out[(size_t)blockIdx.x * 9 + tid] = score;
    } else {
        constexpr bool kMasked = KIND == kSubF32Mask;
        constexpr int kS1 = kMasked ? 0 : CH;       // window sums per channel (unmasked only)
        __shared__ __attribute__((aligned(16))) SubImageLdsF If[1];
        __shared__ double red[4];
        const int h = S.T.rows, w = S.T.cols;
        // the nine windows' correlations (masked: sum I T M^2), second sums (sum I^2, masked: sum I^2 M^2) and per-channel
        // sums
        double corr[9], s2[9], s1[9][kS1 > 0 ? kS1 : 1];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            corr[k] = 0;
            s2[k] = 0;
#pragma unroll
            for (int c = 0; c < (kS1 > 0 ? kS1 : 1); ++c) s1[k][c] = 0;
        }
        const int oy = P.y - 1, ox = P.x - 1;       // image pixel of LDS patch (0, 0) for template pixel (r0, c0)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            for (int r0 = 0; r0 < h; r0 += kSubR)
                for (int c0 = 0; c0 < w; c0 += kSubC) {
                    const int ni = min(kSubR, h - r0), nj = min(kSubC, w - c0);
                    __syncthreads();                // the previous chunk's LDS reads are done
                    sub_load_image_f(If[0], img.f32 + c * img.f32_plane, img.f32_pitch, img.rows, img.cols, oy + r0, ox + c0,
                                     tid);
                    __syncthreads();
                    const double* k1 = wts + S.k1_off + (size_t)c * h * w;
                    const double* k2 = kMasked ? wts + S.k2_off + (size_t)c * h * w : nullptr;
                    for (int p = tid; p < kSubR * kSubC; p += 256) {
                        const int i = p / kSubC, j = p % kSubC;
                        if (i >= ni || j >= nj) continue;
                        const size_t ti = (size_t)(r0 + i) * w + c0 + j;
                        const double a = k1[ti];
                        const double b = kMasked ? k2[ti] : 0.0;
#pragma unroll
                        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                            for (int dx = 0; dx < 3; ++dx) {
                                const int k = dy * 3 + dx;
                                const double v = (double)If[0][i + dy][j + dx];
                                corr[k] = fma(v, a, corr[k]);
                                if constexpr (kMasked) {
                                    s2[k] = fma(v * v, b, s2[k]);
                                } else {
                                    s1[k][c < kS1 ? c : 0] += v;
                                    s2[k] = fma(v, v, s2[k]);
                                }
                            }
                    }
                }
        }
        // reduce; thread k < 9 keeps window k's sums
        double rc = 0, r2 = 0, r1[kS1 > 0 ? kS1 : 1];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double a = sub_reduce(corr[k], red);
            const double b = sub_reduce(s2[k], red);
            if (tid == k) {
                rc = a;
                r2 = b;
            }
#pragma unroll
            for (int c = 0; c < kS1; ++c) {
                const double s = sub_reduce(s1[k][c], red);
                if (tid == k) r1[c] = s;
            }
        }
        if (tid >= 9) return;
        const int dy = tid / 3 - 1, dx = tid % 3 - 1;
        const int wy = P.y + dy, wx = P.x + dx;
        float score = NAN;
        if (wy >= 0 && wx >= 0 && wy <= img.rows - h && wx <= img.cols - w) {
            if constexpr (kMasked) {
                score = finish_masked(method, rc, r2, S.T);
            } else {
                // win_score's statistics from float64 sums
                const bool centred = method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED;
                double mean2 = 0.0;
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    if (centred) mean2 += r1[c] * r1[c];
                const double inv_area = 1.0 / ((double)h * (double)w);
                const double wnd_mean2 = mean2 * inv_area;
                score = finish_unmasked_with(
                    method, rc, [&](int c) { return c < CH ? r1[c < CH ? c : 0] : 0.0; }, [&]() { return r2; },
                    [&]() { return window_norm(r2, wnd_mean2); }, S.T, CH);
            }
        }
        out[(size_t)blockIdx.x * 9 + tid] = score;
    }
}

}  // namespace mtm

namespace {

// A template of the last mtm_set_templates as its bytes in mtm_ctx::templ_blob: any pixel type, with its mask rows.
struct SubBlob {
    int rows, cols, chans, dtype, masked;
    const uint8_t* px;          // rows of `row` bytes, each followed by the mask's row when masked
    size_t row;
};

int parse_sub_blob(const std::vector<uint8_t>& b, std::vector<SubBlob>& out, const char* who) {
    size_t off = 0;
    auto rd = [&](void* dst, size_t n) {
        if (off + n > b.size()) return false;
        std::memcpy(dst, b.data() + off, n);
        off += n;
        return true;
    };
    int n_templ = 0, method = 0, n_var = 0;
    if (!rd(&n_templ, sizeof(int)) || !rd(&method, sizeof(int)) || !rd(&n_var, sizeof(int))) {
        set_error(std::string(who) + ": no templates set");
        return MTM_E_STATE;
    }
    if (n_var != 0) {
        set_error(std::string(who) + ": takes the templates of mtm_set_templates (not an augmented set)");
        return MTM_E_INVALID;
    }
    out.clear();
    for (int i = 0; i < n_templ; ++i) {
        int hdr[5];
        if (!rd(hdr, sizeof(hdr))) return MTM_E_STATE;
        SubBlob t{hdr[0], hdr[1], hdr[2], hdr[3], hdr[4], b.data() + off,
                  (size_t)hdr[1] * hdr[2] * elem_size(hdr[3])};
        const size_t bytes = t.row * t.rows * (t.masked ? 2 : 1);
        if (off + bytes > b.size()) return MTM_E_STATE;
        out.push_back(t);
        off += bytes;
    }
    return MTM_OK;
}

// pixel k (interleaved index y * cols * chans + x * chans + ch) of the template (mask = false) or of its mask
double blob_value(const SubBlob& t, int y, int x, int ch, bool mask) {
    const uint8_t* r = t.px + (size_t)y * t.row * (t.masked ? 2 : 1) + (mask ? t.row : 0);
    const size_t e = (size_t)x * t.chans + ch;
    if (t.dtype == MTM_U8) return (double)r[e];
    if (t.dtype == MTM_U16) {
        uint16_t v;
        std::memcpy(&v, r + 2 * e, 2);
        return (double)v;
    }
    float f;
    std::memcpy(&f, r + 4 * e, 4);
    return (double)f;
}

// The operands of every template of the current set (byte arena, float64 weights, SubTempl table), built once per template
// set (sub_gen).
int prepare_sub_templates(mtm_ctx* c, const std::vector<SubBlob>& tl) {
    if (c->sub_gen == c->templ_gen) return MTM_OK;
    const size_t n = tl.size();
    if (c->templs.size() != n) {
        set_error("mtm_hit_neighbourhoods: template set and its statistics differ in size");
        return MTM_E_STATE;
    }
    c->sub_gen = 0;
    std::vector<uint8_t> bytes;
    std::vector<double> wts;
    std::vector<SubTempl> st(n);
    for (size_t i = 0; i < n; ++i) {
        const SubBlob& t = tl[i];
        const HostTempl& ht = c->templs[i];
        SubTempl& s = st[i];
        s.T = TemplDev{};
        for (int k = 0; k < kMaxChans; ++k) s.T.mean[k] = ht.st.mean[k];
        s.T.templ_norm = ht.st.templ_norm;
        s.T.templ_sum2 = ht.st.templ_sum2;
        s.T.templ2_mask2_sum = ht.st.templ2_mask2_sum;
        s.T.all_ones = ht.st.all_ones;
        s.T.rows = t.rows;
        s.T.cols = t.cols;
        s.px_off = s.mk_off = s.k1_off = s.k2_off = -1;
        const size_t plane = (size_t)t.rows * t.cols;
        if (t.dtype == MTM_F32) {
            s.k1_off = (long long)wts.size();
            s.k2_off = t.masked ? s.k1_off + (long long)(plane * t.chans) : -1;
            wts.resize(wts.size() + plane * t.chans * (t.masked ? 2 : 1));
            double* k1 = wts.data() + s.k1_off;
            for (int ch = 0; ch < t.chans; ++ch)
                for (int y = 0; y < t.rows; ++y)
                    for (int x = 0; x < t.cols; ++x) {
                        const size_t p = (size_t)ch * plane + (size_t)y * t.cols + x;
                        const double v = blob_value(t, y, x, ch, false);
                        if (t.masked) {                 // as the exhaustive kernel's weights: K1 = T M^2, K2 = M^2
                            const double m = blob_value(t, y, x, ch, true);
                            const double m2 = m * m;
                            k1[p] = v * m2;
                            wts[(size_t)s.k2_off + p] = m2;
                        } else {
                            k1[p] = v;
                        }
                    }
            continue;
        }
        s.px_off = (long long)bytes.size();
        if (t.dtype == MTM_U16) {               // high-byte plane, then low-byte plane
            bytes.resize(bytes.size() + 2 * plane);
            uint8_t* d = bytes.data() + s.px_off;
            for (int y = 0; y < t.rows; ++y)
                for (int x = 0; x < t.cols; ++x) {
                    const unsigned v = (unsigned)blob_value(t, y, x, 0, false);
                    d[(size_t)y * t.cols + x] = (uint8_t)(v >> 8);
                    d[plane + (size_t)y * t.cols + x] = (uint8_t)(v & 255u);
                }
            continue;
        }
        // uint8: planar T (masked: T * M, M binary as CV_8U masks are), then the mask bytes 0xFF / 0x00
        bytes.resize(bytes.size() + plane * t.chans * (t.masked ? 2 : 1));
        uint8_t* d = bytes.data() + s.px_off;
        if (t.masked) s.mk_off = s.px_off + (long long)(plane * t.chans);
        for (int ch = 0; ch < t.chans; ++ch)
            for (int y = 0; y < t.rows; ++y)
                for (int x = 0; x < t.cols; ++x) {
                    const size_t p = (size_t)ch * plane + (size_t)y * t.cols + x;
                    const uint8_t v = (uint8_t)blob_value(t, y, x, ch, false);
                    const bool on = !t.masked || blob_value(t, y, x, ch, true) > 0.0;
                    d[p] = on ? v : 0;
                    if (t.masked) d[plane * t.chans + p] = on ? 0xFF : 0x00;
                }
    }
    if (!bytes.empty()) {
        MTMC(c->sub_bytes.ensure(bytes.size()));
        HIPC(hipMemcpy(c->sub_bytes.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    }
    if (!wts.empty()) {
        MTMC(c->sub_wts.ensure(sizeof(double) * wts.size()));
        HIPC(hipMemcpy(c->sub_wts.p, wts.data(), sizeof(double) * wts.size(), hipMemcpyHostToDevice));
    }
    if (n > 0) {
        MTMC(c->sub_td.ensure(sizeof(SubTempl) * n));
        HIPC(hipMemcpy(c->sub_td.p, st.data(), sizeof(SubTempl) * n, hipMemcpyHostToDevice));
    }
    c->sub_gen = c->templ_gen;
    return MTM_OK;
}

}  // namespace

extern "C" {

int mtm_hit_neighbourhoods(mtm_ctx* c, const void* px, int rows, int cols, int chans, int dtype, int64_t row_stride_bytes,
                           const mtm_point* pts, int n, float* out) {
    const char* who = "mtm_hit_neighbourhoods";
    if (!c || n < 0 || (n > 0 && (!pts || !out))) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, who));
    if (!(((dtype == MTM_U8 || dtype == MTM_F32) && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        set_error(std::string(who) + ": takes uint8 and float32 images with 1 or 3 channels and single-channel uint16 images");
        return MTM_E_INVALID;
    }
    if (!c->have_templ) {
        set_error(std::string(who) + ": no templates set");
        return MTM_E_STATE;
    }
    std::vector<SubBlob> tl;
    MTMC(parse_sub_blob(c->templ_blob, tl, who));
    const int method = c->method;
    bool any_masked = false;
    for (int i = 0; i < n; ++i) {
        const mtm_point& p = pts[i];
        const std::string where = std::string(who) + ": point " + std::to_string(i);
        if (p.templ_idx < 0 || p.templ_idx >= (int)tl.size()) {
            set_error(where + ": template index out of range");
            return MTM_E_INVALID;
        }
        const SubBlob& t = tl[(size_t)p.templ_idx];
        if (t.dtype != dtype || t.chans != chans) {
            set_error(where + ": template and image differ in pixel type or channel count");
            return MTM_E_INVALID;
        }
        if (t.masked && (dtype == MTM_U16 || method > MTM_TM_CCORR_NORMED)) {
            set_error(where + ": masked templates take uint8 or float32 pixels and methods 0..3");
            return MTM_E_INVALID;
        }
        if (p.x < 0 || p.y < 0 || p.x > cols - t.cols || p.y > rows - t.rows) {
            set_error(where + ": window outside the image's score map");
            return MTM_E_INVALID;
        }
        // (uint16: correlations of up to 2^21 pixels stay below 2^53, exact in float64 as the exhaustive kernels need)
        if (dtype == MTM_U16 && (long long)t.rows * t.cols > (1ll << 21)) {
            set_error(where + ": uint16 template of more than 2^21 pixels");
            return MTM_E_INVALID;
        }
        any_masked = any_masked || t.masked;
    }
    if (n == 0) return MTM_OK;
    HIPC(hipSetDevice(c->device));
    MTMC(prepare_sub_templates(c, tl));

    // ONE upload of the image; every point reads its patch from the same planes
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    MTMC(upload_image(c, c->slot[c->cur], px, row_stride_bytes, rows, cols, chans, dtype, c->stream, 1));
    adopt_image(c, rows, cols, chans, dtype);

    // masked and unmasked templates are separate kernels: the points of each kind go in a launch of their own
    std::vector<SubPoint> sp;
    std::vector<int> where;                 // sp[k] is point where[k]
    sp.reserve((size_t)n);
    where.reserve((size_t)n);
    for (int pass = 0; pass < (any_masked ? 2 : 1); ++pass)
        for (int i = 0; i < n; ++i)
            if ((tl[(size_t)pts[i].templ_idx].masked != 0) == (pass == 1)) {
                sp.push_back(SubPoint{pts[i].templ_idx, pts[i].x, pts[i].y});
                where.push_back(i);
            }
    size_t n_plain = 0;
    while (n_plain < sp.size() && !tl[(size_t)sp[n_plain].t].masked) ++n_plain;
    MTMC(c->sub_pts.ensure(sizeof(SubPoint) * sp.size()));
    MTMC(c->sub_out.ensure(sizeof(float) * 9 * sp.size()));
    HIPC(hipMemcpyAsync(c->sub_pts.p, sp.data(), sizeof(SubPoint) * sp.size(), hipMemcpyHostToDevice, c->stream));

    const ImageDev img = image_dev(c);
    const uint8_t* lo_b = c->slot[c->cur].u8b.as<uint8_t>() + img.u8_plane;     // uint16: [high ^ 0x80][low ^ 0x80]
    for (int pass = 0; pass < 2; ++pass) {
        const size_t b0 = pass == 0 ? 0 : n_plain, b1 = pass == 0 ? n_plain : sp.size();
        const bool masked = pass == 1;
        for (size_t p0 = b0; p0 < b1; p0 += kSubLaunchPoints) {
            const unsigned np = (unsigned)std::min(kSubLaunchPoints, b1 - p0);
#define MTM_SUB_LAUNCH(CH, KIND)                                                                                             \
    hipLaunchKernelGGL((sub_nbhd_kernel<CH, KIND>), dim3(np), dim3(256), 0, c->stream, img, lo_b, c->sub_bytes.as<uint8_t>(), \
                       c->sub_wts.as<double>(), c->sub_td.as<SubTempl>(), c->sub_pts.as<SubPoint>() + p0,                    \
                       c->sub_out.as<float>() + 9 * p0, method)
            if (dtype == MTM_U16) MTM_SUB_LAUNCH(1, kSubU16);
            else if (dtype == MTM_U8 && !masked && chans == 1) MTM_SUB_LAUNCH(1, kSubU8);
            else if (dtype == MTM_U8 && !masked) MTM_SUB_LAUNCH(3, kSubU8);
            else if (dtype == MTM_U8 && chans == 1) MTM_SUB_LAUNCH(1, kSubU8Mask);
            else if (dtype == MTM_U8) MTM_SUB_LAUNCH(3, kSubU8Mask);
            else if (!masked && chans == 1) MTM_SUB_LAUNCH(1, kSubF32);
            else if (!masked) MTM_SUB_LAUNCH(3, kSubF32);
            else if (chans == 1) MTM_SUB_LAUNCH(1, kSubF32Mask);
            else MTM_SUB_LAUNCH(3, kSubF32Mask);
#undef MTM_SUB_LAUNCH
            HIPC(hipGetLastError());
        }
    }
    std::vector<float> res(9 * sp.size());
    HIPC(hipMemcpyAsync(res.data(), c->sub_out.p, sizeof(float) * res.size(), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < sp.size(); ++k) std::memcpy(out + 9 * (size_t)where[k], res.data() + 9 * k, 9 * sizeof(float));
    return MTM_OK;
}

}  // extern "C"
