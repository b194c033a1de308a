// libmtm_hip.so - template sets: pixels -> size classes, device-resident sources and unit views, operand packs for every
// kernel family, per-template constants (place_templates).
#include <functional>
#include "mtm_ctx.h"

using namespace mtm;
using namespace mtmi;
#include "mtm_templates.hip.h"

namespace {

// Packs one uint8 template for ncc_dot4_kernel (layout documented in mtm_k_score.hip.h).
size_t dot_pack_bytes(int h, int w, int chans) {
    const int w4 = (w + 3) & ~3;
    const int ncy = (h + kDotChunk - 1) / kDotChunk, ncx = (w4 + kDotChunk - 1) / kDotChunk;
    return (size_t)chans * ncy * ncx * kDotChunkBytes;
}

void pack_template_dot4(const HostTempl& t, uint8_t* out) {
    const int h = t.rows, w = t.cols;
    const int w4 = (w + 3) & ~3;
    const int ncy = (h + kDotChunk - 1) / kDotChunk, ncx = (w4 + kDotChunk - 1) / kDotChunk;
    std::memset(out, 0, dot_pack_bytes(h, w, t.chans));
    for (int c = 0; c < t.chans; ++c)
        for (int cy = 0; cy < ncy; ++cy)
            for (int cx = 0; cx < ncx; ++cx) {
                uint8_t* chunk = out + ((size_t)(c * ncy + cy) * ncx + cx) * kDotChunkBytes;
                const int ch = std::min(kDotChunk, h - cy * kDotChunk);
                const int cw = std::min(kDotChunk, w - cx * kDotChunk);
                for (int dy = 0; dy < ch; ++dy)
                    for (int dx = 0; dx < cw; ++dx)
                        chunk[(dy + kDotPadRows) * kDotChunk + dx] =
                            (uint8_t)t.px[((size_t)c * h + cy * kDotChunk + dy) * w + cx * kDotChunk + dx];
            }
}

// A-operand packs of ncc_mfma_kernel for one size class: per group of 16 templates (list order),
// [channel][template row][64-tap block][lane = 16*q + i][16 bytes]: lane (i, q) holds taps
// 64*b + 16*q .. +15 of template i, biased to int8 (T ^ 0x80); taps beyond the template width and
// templates beyond the list are 0 (the signed zero), so they add nothing.
std::vector<SizeClass::Slab> slab_layout(const mtm_ctx* c, const SizeClass& sc) {
    std::vector<SizeClass::Slab> out;
    if (sc.masked || !sc.all_u8 || c->dtype != MTM_U8) return out;
    for (int m : sc.members)
        if (!c->templs[(size_t)m].on_device) return out;
    auto layout = [&](int cw) {
        std::vector<SizeClass::Slab> v;
        const int rows_max = 131071 / std::min(cw, ((sc.w + 63) / 64) * 64);
        const int nrb = (sc.h + rows_max - 1) / rows_max, rh = (sc.h + nrb - 1) / nrb;
        for (int ch = 0; ch < c->chans; ++ch)
            for (int r0 = 0; r0 < sc.h; r0 += rh)
                for (int c0 = 0; c0 < sc.w; c0 += cw)
                    v.push_back(SizeClass::Slab{r0, std::min(sc.h, r0 + rh), c0, std::min(sc.w, c0 + cw), ch, 0, 0});
        if (v.size() > 24) v.clear();            // absurdly large: the VALU kernel takes it
        return v;
    };
    if (sc.members.size() > 16) return layout(256);
    // <= 16 templates (row-multiplexed raw launches): column blocks of 128 or 64 taps.  A slab launch is few, long work
    // items - 91 of 128 output rows x 256 columns for 2048^2 x 414x400 - whose waves cannot be split: with 128-tap slabs
    // that shape is 1.24 waves' worth of work per SIMD and the launches take as long as the SIMDs that got two.  Half as
    // wide slabs are twice as many waves of half the length (and more raw planes for slab_combine_kernel to add): the
    // width whose greedy schedule over the CUs ends first is taken.
    std::vector<SizeClass::Slab> best = layout(128);
    if (!c->have_image || c->rows < sc.h || c->cols < sc.w) return best;
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    const int cus = c->n_cus > 0 ? c->n_cus : 256;
    auto makespan = [&](const std::vector<SizeClass::Slab>& v) {
        if (v.empty()) return 1e300;
        int hs = 0, ws = 0;
        for (const auto& sl : v) {
            hs = std::max(hs, sl.r1 - sl.r0);
            ws = std::max(ws, sl.c1 - sl.c0);
        }
        const int R = 16 / rm_group_templates((int)sc.members.size(), hs, ws);
        const long long items = (long long)((ow + kMfSeg - 1) / kMfSeg) * ((oh + 8 * R - 1) / (8 * R));
        std::vector<double> cost;                         // one entry per work-group, longest first
        for (const auto& sl : v)
            cost.insert(cost.end(), (size_t)items, (double)((sl.c1 - sl.c0 + 63) / 64) * (sl.r1 - sl.r0 + 2 * R - 1));
        std::sort(cost.begin(), cost.end(), std::greater<double>());
        std::vector<double> load((size_t)cus, 0.0);       // min-heap of CU loads
        auto cmp = std::greater<double>();
        for (double x : cost) {
            std::pop_heap(load.begin(), load.end(), cmp);
            load.back() += x;
            std::push_heap(load.begin(), load.end(), cmp);
        }
        // every slab's raw plane is written once and read once by the combine pass: ~5 us per 4 B x 2 x oh x ow at
        // 2048^2, against ~0.2 us per (block x template row) step of a work-group - in units of steps
        return *std::max_element(load.begin(), load.end()) + 25.0 * (double)v.size() * ((double)oh * ow / 2.7e6);
    };
    std::vector<SizeClass::Slab> narrow = layout(64);
    if (makespan(narrow) < 0.9 * makespan(best)) best.swap(narrow);
    return best;
}

bool mfma_class_ok(const mtm_ctx* c, const SizeClass& sc) {
    if (c->dtype == MTM_U8 && sc.all_u8 && !sc.masked && (sc.w > kMfmaMaxW || (long long)c->chans * sc.w * sc.h > 131071))
        return !slab_layout(c, sc).empty();
    if (!(c->dtype == MTM_U8 && sc.all_u8 && sc.w <= kMfmaMaxW && (long long)c->chans * sc.w * sc.h <= 131071))
        return false;
    // masked: single channel, sum I^2*M must fit the uint32 dot4 accumulator (w*h*255^2 < 2^32)
    if (sc.masked) return c->chans == 1 && (long long)sc.w * sc.h <= 66051;
    return true;
}
// the binary mask of a masked class as the single "template" (nt = 1, R = 16) of the sum I^2 M pass
void pack_mask_rm(const mtm_ctx* c, const SizeClass& sc, uint8_t* out) {
    const int h = sc.h, w = sc.w, nb = (w + 63) / 64, R = 16;
    std::memset(out, 0, (size_t)rm_pack_bytes(h, w, R));
    const HostTempl& ht = c->templs[sc.members[0]];
    for (int sp = 0; sp < h + 3 * R - 1; ++sp)
        for (int i = 0; i < 16; ++i) {
            const int dy = sp - R - i;
            if (dy < 0 || dy >= h) continue;
            for (int dx = 0; dx < w; ++dx) {
                const int b = dx / 64, q = (dx % 64) / 16, byte = dx % 16;
                const uint8_t v = ht.mask[(size_t)dy * w + dx] > 0.0 ? 1 : 0;
                out[(((size_t)sp * nb + b) * 64 + (16 * q + i)) * 16 + byte] = v;           // int8 0 / 1: the mask is not biased
            }
        }
}

void pack_class_rm(const mtm_ctx* c, const SizeClass& sc, uint8_t* out, size_t bytes) {
    const int h = sc.h, w = sc.w, nb = (w + 63) / 64, R = sc.rm_R, nt = sc.rm_nt, nseg = sc.kp_nseg;
    const int chans = sc.masked ? 1 : c->chans;                 // one pack per channel, class_rm_pack_bytes apart
    const size_t cstride = (size_t)class_rm_pack_bytes(sc);
    std::memset(out, 0, bytes);
    if (nseg) {                                  // packed K: [ch][group g][step][lane][16], stream row r: dy = r - g R - rho
        const size_t gbytes = cstride / 2;
        for (int ch = 0; ch < chans; ++ch)
            for (int g = 0; g < 2; ++g)
                for (int r = 0; r < h + 2 * R - 1; ++r)
                    for (int i = 0; i < 16; ++i) {
                        const int t = i % nt, rho = i / nt, dy = r - g * R - rho;
                        if (t >= (int)sc.members.size() || dy < 0 || dy >= h) continue;
                        const HostTempl& ht = c->templs[sc.members[(size_t)t]];
                        for (int dx = 0; dx < w; ++dx) {
                            const size_t k = ((size_t)ch * h + dy) * w + dx;
                            const int sidx = r * nseg + dx / 16;
                            const uint8_t v = (uint8_t)(ht.masked ? ht.px[k] * ht.mask[k] : ht.px[k]);   // masked: T*M
                            out[ch * cstride + g * gbytes + (((size_t)(sidx / 4) * 64) + (16 * (sidx % 4) + i)) * 16 + dx % 16] =
                                v ^ 0x80;
                        }
                    }
        return;
    }
    for (int ch = 0; ch < chans; ++ch)
        for (int sp = 0; sp < h + 3 * R - 1; ++sp)
            for (int i = 0; i < 16; ++i) {
                const int t = i % nt, rho = i / nt, dy = sp - R - rho;
                if (t >= (int)sc.members.size() || dy < 0 || dy >= h) continue;
                const HostTempl& ht = c->templs[sc.members[(size_t)t]];
                for (int dx = 0; dx < w; ++dx) {
                    const size_t k = ((size_t)ch * h + dy) * w + dx;
                    const uint8_t v = (uint8_t)(ht.masked ? ht.px[k] * ht.mask[k] : ht.px[k]);   // masked: T*M, M in {0,1}
                    const size_t blk = (size_t)sp * nb + dx / 64;
                    const int q = (dx % 64) / 16;
                    out[ch * cstride + ((blk * 64) + (16 * q + i)) * 16 + dx % 16] = v ^ 0x80;
                }
            }
}

// uint16 image + uint16 templates, one channel, no mask: four uint8 byte-plane correlations on the int8
// MFMA kernel (a raw pass over the high bytes, a finishing pass over the low bytes).  The two middle correlations,
// I_hi x T_lo + I_lo x T_hi, share ONE int32 accumulator (a_mid of the uint16 epilogue): up to 2 x 16384 w h where both
// biased operands are -128 (zero bytes), which fits up to w h = 65535 - half the uint8 path's bound.  (The bound was the
// uint8 one until tests/test_gpu_tilings.py ran 511 x 256: zero regions under zero templates wrapped a_mid.)  Larger
// classes take the float64 kernel.
constexpr long long kMfma16MaxArea = 65535;
static_assert(2 * 16384 * kMfma16MaxArea <= 2147483647LL, "a_mid of the uint16 epilogue must fit an int32");
bool mfma16_class_ok(const mtm_ctx* c, const SizeClass& sc) {
    return c->dtype == MTM_U16 && sc.all_u16 && c->chans == 1 && !sc.masked && sc.w <= kMfmaMaxW &&
           (long long)sc.w * sc.h <= kMfma16MaxArea;
}

// float32 image + float32 templates, no mask: bfloat16 pieces on the bf16 matrix cores.  The normalised methods' outputs
// are O(1) and stay within ~1e-5 of the float64 result; the raw sums (TM_SQDIFF, TM_CCORR, TM_CCOEFF) can cancel to values
// far smaller than the sums they are built from (an exact copy: SQDIFF = 0), so no RELATIVE margin holds for them - their
// lists are decided by an absolute per-output bound and exact re-scoring (mtm_api.hip), their maps by the float64 kernel.
bool bf16_class_ok(const mtm_ctx* c, const SizeClass& sc) {
    // All six methods (round 4).  The raw-sum methods only take this kernel for the refined global extremum
    // (N_object == 1; mtm_api.hip decides per call) - everything else they do runs the float64 kernel, for which a
    // bf16 class carries its float64 weights anyway.
    // (1-D and 1x1 score maps go through scipy's find_peaks on the host, which has no refinement: float64 kernel)
    return c->f32_mfma && c->dtype == MTM_F32 && sc.all_f32 && !sc.masked && sc.w <= kBfMaxW &&
           c->rows > sc.h && c->cols > sc.w;
}
// float32 class with masks (float weights or binary), one channel, TM_SQDIFF / TM_CCORR_NORMED - the methods the reference
// lets masks through for (MTM/__init__.py:78): two raw bf16 correlations as a screen + exact re-scoring (mtm_maskf32.hip.h)
bool masked_bf16_class_ok(const mtm_ctx* c, const SizeClass& sc) {
    return f32_refined(c) && c->dtype == MTM_F32 && sc.all_f32 && sc.masked && c->chans == 1 && sc.w <= kBfMaxW &&
           c->rows > sc.h && c->cols > sc.w && (c->method == MTM_TM_SQDIFF || c->method == MTM_TM_CCORR_NORMED);
}

// The kernel that runs a class, recorded by placement in SizeClass::kernel.  Everything it reads re-places when it changes:
// opt_kernel and f32_mfma (mtm_set_option, which bf16_class_ok only tests for non-zero), dtype and the image dimensions
// (adopt_image), method (a new template set); auto_kernel is fixed at construction.
int resolved_kernel(const mtm_ctx* c, const SizeClass& sc) {
    const bool dot_ok = c->dtype == MTM_U8 && sc.all_u8 && !sc.masked;
    int kernel = c->opt_kernel;
    if (c->dtype == MTM_F32) {
        if ((kernel == MTM_KERNEL_AUTO || kernel == MTM_KERNEL_MFMA) && bf16_class_ok(c, sc)) return MTM_KERNEL_MFMA_F32;
        return kernel == MTM_KERNEL_NAIVE ? MTM_KERNEL_NAIVE : MTM_KERNEL_AUTO;
    }
    if (c->dtype == MTM_U16) {
        if ((kernel == MTM_KERNEL_AUTO || kernel == MTM_KERNEL_MFMA) && mfma16_class_ok(c, sc)) return MTM_KERNEL_MFMA16;
        return kernel == MTM_KERNEL_NAIVE ? MTM_KERNEL_NAIVE : MTM_KERNEL_AUTO;
    }
    if (kernel == MTM_KERNEL_AUTO) kernel = c->auto_kernel;
    if (kernel == MTM_KERNEL_MFMA && (!mfma_class_ok(c, sc) || (sc.masked && c->method > 3))) kernel = MTM_KERNEL_DOT4;
    if (kernel == MTM_KERNEL_DOT4 && !dot_ok) kernel = MTM_KERNEL_AUTO;
    return kernel;
}

// A packs of a float32 class for ncc_bf16_kernel: [piece 0 | piece 1][group of 16][ch][dy][32-tap block][lane = 16 q + i]
// [8 bf16]: lane (i, q) holds taps 32 kb + 8 q .. + 7 of template i, centred by its channel mean and split
// v = v0 + v1 (bfloat16, round to nearest even).  centre[] receives the means (TemplDev::centre).
// `which`: 0 = the template's pixels; 1 = U = T M^2, 2 = V = M^2 (masked classes, single channel: mtm_maskf32.hip.h) - then
// td_host is the U / V copy of the table: centre and centred_sum2 of the packed values go there
// `gb`: bytes per group of 16 templates, `bytes`: of both pieces.
void pack_class_bf16(const mtm_ctx* c, const SizeClass& sc, uint8_t* out, long long gb, size_t bytes,
                     std::vector<TemplDev>& td_host, int which) {
    const int h = sc.h, w = sc.w, nkb = bf16_nkb(w), chans = c->chans;
    const size_t piece = bytes / 2;
    std::memset(out, 0, bytes);
    auto rne = [](float v) {
        uint32_t b;
        std::memcpy(&b, &v, 4);
        return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
    };
    for (size_t li = 0; li < sc.members.size(); ++li) {
        const HostTempl& t = c->templs[sc.members[li]];
        TemplDev& d = td_host[(size_t)sc.members[li]];
        uint8_t* g = out + (li / 16) * gb;
        const int i = (int)(li % 16);
        const size_t plane = (size_t)h * w;
        auto val = [&](size_t k) {
            if (which == 0) return t.px[k];
            const double m2 = t.mask[k] * t.mask[k];
            return which == 1 ? t.px[k] * m2 : m2;
        };
        if (which) d.centred_sum2 = 0.0;
        for (int ch = 0; ch < chans; ++ch) {
            double mean = 0.0;
            for (size_t k = 0; k < plane; ++k) mean += val(ch * plane + k);
            mean /= (double)plane;
            d.centre[ch] = mean;
            if (which)
                for (size_t k = 0; k < plane; ++k) d.centred_sum2 += (val(ch * plane + k) - mean) * (val(ch * plane + k) - mean);
            for (int dy = 0; dy < h; ++dy)
                for (int dx = 0; dx < w; ++dx) {
                    const float v = (float)(val(ch * plane + (size_t)dy * w + dx) - mean);
                    const uint16_t v0 = rne(v);
                    const uint16_t v1 = rne(v - bf16_to_float(v0));
                    const int kb = dx / 32, q = (dx % 32) / 8, e = dx % 8;
                    const size_t o = ((((size_t)ch * h + dy) * nkb + kb) * 64 + (16 * q + i)) * 16 + 2 * e;
                    std::memcpy(g + o, &v0, 2);
                    std::memcpy(g + piece + o, &v1, 2);
                }
        }
    }
}

// A packs of a uint16 class: 2 * n_pad pseudo-templates in 16-template groups [high bytes of members 16 g .. 16 g + 15]
// [low bytes of the same members] - one work item of ncc_mfma_kernel (32 pseudo-templates) holds both byte planes of
// 16 templates.  Same lane order as pack_class_mfma.  Also the byte sums of every member (bias terms of the
// combination): tsum[li] high bytes, tsum[n_pad + li] low bytes.
void pack_class_mfma16(const mtm_ctx* c, const SizeClass& sc, uint8_t* out, size_t bytes, double* tsum) {
    const int h = sc.h, w = sc.w, nb = (w + 63) / 64, n_pad = sc.n_pad, nseg = sc.kp_nseg;
    const long long gb = sc.group_bytes;
    std::memset(out, 0, bytes);
    for (int k = 0; k < 2 * n_pad; ++k) tsum[k] = 0.0;
    for (size_t li = 0; li < sc.members.size(); ++li) {
        const HostTempl& t = c->templs[sc.members[li]];
        for (int part = 0; part < 2; ++part) {
            uint8_t* g = out + (2 * (li / 16) + (size_t)part) * gb;
            const int i = (int)(li % 16);
            double sum = 0.0;
            for (int dy = 0; dy < h; ++dy)
                for (int dx = 0; dx < w; ++dx) {
                    const unsigned v16 = (unsigned)t.px[(size_t)dy * w + dx];
                    const uint8_t v = part == 0 ? (uint8_t)(v16 >> 8) : (uint8_t)(v16 & 255u);
                    sum += v;
                    const int b = dx / 64, q = (dx % 64) / 16, byte = dx % 16;
                    if (nseg) {                                  // packed K: segment dy * nseg + dx / 16 of the row stream
                        const int sidx = dy * nseg + dx / 16;
                        g[(((size_t)(sidx / 4)) * 64 + (16 * (sidx % 4) + i)) * 16 + byte] = v ^ 0x80;
                        continue;
                    }
                    g[(((size_t)dy * nb + b) * 64 + (16 * q + i)) * 16 + byte] = v ^ 0x80;
                }
            tsum[(size_t)part * n_pad + li] = sum;
        }
    }
}

void pack_class_mfma(const mtm_ctx* c, const SizeClass& sc, uint8_t* out, size_t bytes) {
    const int h = sc.h, w = sc.w, nb = (w + 63) / 64, chans = c->chans, nseg = sc.kp_nseg;
    // multi-row variant: groups of h + r2 - 1 rows (one channel), the extra rows stay zero; packed K: kp_blocks steps per channel
    const long long gb = sc.group_bytes;
    std::memset(out, 0, bytes);
    for (size_t li = 0; li < sc.members.size(); ++li) {
        const HostTempl& t = c->templs[sc.members[li]];
        uint8_t* g = out + (li / 16) * gb;
        const int i = (int)(li % 16);
        for (int ch = 0; ch < chans; ++ch)
            for (int dy = 0; dy < h; ++dy)
                for (int dx = 0; dx < w; ++dx) {
                    const int b = dx / 64, q = (dx % 64) / 16, byte = dx % 16;
                    const size_t k = ((size_t)ch * h + dy) * w + dx;
                    const uint8_t v = (uint8_t)(t.masked ? t.px[k] * t.mask[k] : t.px[k]);   // masked: T*M, M in {0,1}
                    if (nseg) {                                  // packed K: segment dy * nseg + dx / 16 of the row stream
                        const int sidx = dy * nseg + dx / 16;
                        g[((((size_t)ch * kp_blocks(h, nseg) + sidx / 4) * 64) + (16 * (sidx % 4) + i)) * 16 + byte] = v ^ 0x80;
                        continue;
                    }
                    g[((((size_t)ch * (sc.r2 ? h + sc.r2 - 1 : h) + dy) * nb + b) * 64 + (16 * q + i)) * 16 + byte] = v ^ 0x80;
                }
    }
}

// Pixels (and binary mask) of a device-resident uint8 template as the planar float64 arrays the host-side packers
// take: one gather kernel + one copy.  Only the fallback kernels (float64, dot4) ever need it.
int ensure_host_pixels(mtm_ctx* c, int i) {
    HostTempl& t = c->templs[(size_t)i];
    if (!t.on_device || !t.px.empty()) return MTM_OK;
    const size_t n = (size_t)t.chans * t.rows * t.cols;
    MTMC(c->tgather.ensure(2 * n));
    uint8_t* dpx = c->tgather.as<uint8_t>();
    uint8_t* dmk = t.masked ? dpx + n : nullptr;
    hipLaunchKernelGGL(gather_unit_kernel, dim3((t.cols + 63) / 64, t.rows, t.chans), dim3(64), 0, c->stream,
                       c->tsrc.as<uint8_t>(), t.src, dpx, dmk);
    HIPC(hipGetLastError());
    std::vector<uint8_t> host(2 * n);
    HIPC(hipMemcpyAsync(host.data(), dpx, (t.masked ? 2 : 1) * n, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    t.px.resize(n);
    for (size_t k = 0; k < n; ++k) t.px[k] = (double)host[k];
    if (t.masked) {
        t.mask.resize(n);
        for (size_t k = 0; k < n; ++k) t.mask[k] = host[n + k] ? 1.0 : 0.0;
    }
    return MTM_OK;
}

// A packs of one MFMA class gathered on the device from the unit views (pack_units_kernel); layouts as the host
// packers above.  The class's template list must already be in c->tlist.
int pack_class_on_device(mtm_ctx* c, const SizeClass& sc) {
    const uint8_t* arena = c->tsrc.as<uint8_t>();
    const UnitSrc* units = c->usrc_dev.as<UnitSrc>();
    const int* tl = c->tlist.as<int>() + sc.tlist_off;
    PackParams p{};
    p.h = sc.h;
    p.hv = sc.h;
    p.w = sc.w;
    p.nb = (sc.w + 63) / 64;
    p.n = (int)sc.members.size();
    auto launch = [&](long long off) {
        hipLaunchKernelGGL(pack_units_kernel, dim3((unsigned)((p.n_chunks + 255) / 256)), dim3(256), 0, c->stream, p, arena,
                           units, tl, c->apacks.as<uint8_t>() + off);
    };
    if (sc.mask_rm_off >= 0) {            // the binary mask as the single "template" of the sum I^2 M pass
        p.mode = 2;
        p.chans = 1;
        p.nt = 1;
        p.R = 16;
        p.masked = 0;
        p.cstride = rm_pack_bytes(sc.h, sc.w, 16);
        p.n_chunks = p.cstride / 16;
        launch(sc.mask_rm_off);
    }
    if (!sc.slabs.empty()) {               // every slab is a class of its own: its view list, its dimensions
        for (const auto& sl : sc.slabs) {
            p.h = p.hv = sl.r1 - sl.r0;
            p.w = sl.c1 - sl.c0;
            p.nb = (p.w + 63) / 64;
            p.chans = 1;
            p.masked = 0;
            tl = c->tlist.as<int>() + sl.tlist_off;
            if (sc.slab_R > 0) {
                p.mode = 1;
                p.nt = sc.slab_nt;
                p.R = sc.slab_R;
                p.cstride = rm_pack_bytes(p.h, p.w, sc.slab_R);
                p.n_chunks = p.cstride / 16;
            } else {
                p.mode = 0;
                p.group_bytes = mfma_group_bytes(p.h, p.w, 1);
                p.n_chunks = p.group_bytes * mfma_groups_alloc(p.n) / 16;
            }
            launch(sl.apack_off);
        }
        HIPC(hipGetLastError());
        return MTM_OK;
    }
    p.masked = sc.masked ? 1 : 0;
    p.nseg = sc.kp_nseg;
    if (sc.rm_R > 0) {
        p.mode = 1;
        p.chans = sc.masked ? 1 : c->chans;
        p.nt = sc.rm_nt;
        p.R = sc.rm_R;
        p.cstride = class_rm_pack_bytes(sc);
        p.kblocks = (int)(p.cstride / 2048);             // packed K: steps per MFMA group ([ch][group][step])
        p.n_chunks = p.cstride * p.chans / 16;
    } else if (sc.r2) {
        p.mode = 0;
        p.chans = 1;
        p.h = sc.h + sc.r2 - 1;              // rows per group in the pack; rows >= h are zero (hv = valid template rows)
        p.group_bytes = sc.group_bytes;
        p.n_chunks = p.group_bytes * ((p.n + 15) / 16) / 16;
    } else {
        p.mode = 0;
        p.chans = c->chans;
        p.group_bytes = sc.group_bytes;                  // (packed K: chans * kp_blocks steps)
        p.kblocks = sc.kp_nseg ? kp_blocks(sc.h, sc.kp_nseg) : 0;
        p.n_chunks = p.group_bytes * mfma_groups_alloc(p.n) / 16;
    }
    launch(sc.apack_off);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// Regions of one arena, handed out back to back
struct Bump {
    size_t size = 0;
    long long take(size_t n) {
        size += n;
        return (long long)(size - n);
    }
};

// What place_templates derives from the context before any HIP call: each class's kernel and tiling, the arenas' layout,
// the per-template constants, the template lists and slab views, and which operands the host packs.
struct Placement {
    std::vector<SizeClass> classes;
    std::vector<char> dev_pack;     // per class: A packs gathered on the device (pack_class_on_device)
    std::vector<size_t> a_bytes;    // per class: bytes of its host-packed A packs (masked bf16: of each of its U and V packs)
    std::vector<int> host_px;       // device-resident templates whose pixels the host packers read
    std::vector<TemplDev> td, td_u, td_v;
    std::vector<int> tlist, list2d;
    int list2d_off = 0;
    std::vector<UnitSrc> units;     // the unit table, slab views appended
    Bump maps, w, p, a, ts;         // floats of the score maps; float64 weights; dot4 packs; A packs; uint16 tsums
    bool any_host_pack = false, any_mbf = false;
};

// The tiling of a class on the int8 MFMA kernel - uint8: row-multiplexed, slabs, two-row or packed K; uint16: packed K.
void choose_tiling(const mtm_ctx* c, SizeClass& sc) {
    const int n_cls = (int)sc.members.size(), nseg = (sc.w + 15) / 16;
    sc.rm_nt = sc.rm_R = sc.slab_nt = sc.slab_R = sc.r2 = sc.kp_nseg = 0;
    sc.slabs.clear();
    // packed K for the two byte-plane passes (widths that are not multiples of 64), as for uint8 classes
    if (sc.kernel == MTM_KERNEL_MFMA16) sc.kp_nseg = nseg % 4 != 0 ? nseg : 0;
    if (sc.kernel != MTM_KERNEL_MFMA) return;
    if (sc.w > kMfmaMaxW || (long long)c->chans * sc.w * sc.h > 131071) {
        sc.slabs = slab_layout(c, sc);
        if (n_cls <= 16) {                     // row-multiplexed raw launches: nt templates x R rows per MFMA group
            int hs = 0, ws = 0;
            for (const auto& sl : sc.slabs) {
                hs = std::max(hs, sl.r1 - sl.r0);
                ws = std::max(ws, sl.c1 - sl.c0);
            }
            sc.slab_nt = rm_group_templates(n_cls, hs, ws);
            sc.slab_R = 16 / sc.slab_nt;
        }
        return;
    }
    const bool one_pack = c->chans == 1 || (c->chans == 3 && !sc.masked);
    // row-multiplexed mode: <= 16 templates (one channel, masked or not, or unmasked RGB) whose window statistics the fused
    // kernels produce (the single-channel one also writes the 1/sqrt plane); wide templates take fewer rows per MFMA group
    const mtm::StatsRoute stats = mtm::stats_route(c->dtype, c->chans, sc.h, sc.w, c->cols, c->fuse_stats != 0);
    const bool stats_fused = stats == mtm::kStatsRouteU8 || stats == mtm::kStatsRouteU8MC;
    if (c->row_mux && n_cls <= 16 && one_pack && stats_fused) {
        sc.rm_nt = rm_group_templates(n_cls, sc.h, sc.w);
        sc.rm_R = 16 / sc.rm_nt;
    }
    // packed K: widths that leave part of the last 64-tap block empty, on the normalised methods (the instantiated variants
    // ncc_mfma_kernel<.., KP>).  Replaces the two-row variant where both apply (that one saves template loads, this one
    // whole MFMA steps).
    const bool normed = c->method == MTM_TM_SQDIFF_NORMED || c->method == MTM_TM_CCORR_NORMED ||
                        c->method == MTM_TM_CCOEFF_NORMED;
    if (nseg % 4 != 0 && normed && one_pack && (!sc.masked || c->method != MTM_TM_CCOEFF_NORMED))
        sc.kp_nseg = nseg;
    else if (c->mfma_r2 && sc.rm_R == 0 && n_cls > 16 && sc.w <= 64 && c->chans == 1 && !sc.masked &&
             c->method >= MTM_TM_CCORR && c->fuse_stats)
        sc.r2 = 2;
    // tail screen of the two-row variant (one K chunk, splits 6 .. h - 2).  The split is a call's (tail_split_for); the
    // constants computed here are those of the default threshold's, which a call at another one re-derives
    if (sc.r2 == 2 && sc.h + 1 <= mtm::kMfChunkR2 && sc.h >= 8) {
        sc.tail_ok = true;
        sc.tail_split = c->tail_split_force > 0 ? std::max(6, std::min(c->tail_split_force, sc.h - 2))
                                                : tail_split_rule(sc.h, sc.w, kTailDefaultThr - 1e-6);
    }
}

int queue_tail_consts(mtm_ctx* c, const SizeClass& sc, int split, hipStream_t stream) {
    hipLaunchKernelGGL(tail_consts_kernel, dim3((unsigned)sc.members.size()), dim3(64), 0, stream,
                       c->apacks.as<uint8_t>() + sc.apack_off, sc.group_bytes, sc.h, sc.w, split,
                       c->tlist.as<int>() + sc.tlist_off, c->td.as<TemplDev>());
    HIPC(hipGetLastError());
    return MTM_OK;
}

// A class's regions of the A arena (uint16: and of the tsum arena); returns the bytes of its A packs.  Fields of the
// families a class is not in keep their values.
size_t place_apacks(const mtm_ctx* c, SizeClass& sc, Bump& a, Bump& ts) {
    const int n_cls = (int)sc.members.size(), groups = mfma_groups_alloc(n_cls);
    size_t bytes = 0;
    switch (sc.kernel) {
        case MTM_KERNEL_MFMA:
            sc.mask_rm_off = -1;
            if (sc.masked && c->row_mux && c->fuse_stats) {
                sc.mask_rm_off = a.take((size_t)rm_pack_bytes(sc.h, sc.w, 16));
                const HostTempl& m0 = c->templs[sc.members[0]];
                sc.mask_ones = m0.on_device ? m0.mask_ones : 0.0;
                if (!m0.on_device)
                    for (double m : m0.mask) sc.mask_ones += m > 0.0 ? 1.0 : 0.0;
            }
            if (!sc.slabs.empty()) {          // one pack per slab (a template of its own, one channel)
                sc.apack_off = (long long)a.size;
                for (auto& sl : sc.slabs) {
                    const int hs = sl.r1 - sl.r0, ws = sl.c1 - sl.c0;
                    sl.apack_off = a.take(sc.slab_R > 0 ? (size_t)rm_pack_bytes(hs, ws, sc.slab_R)
                                                        : (size_t)mfma_group_bytes(hs, ws, 1) * groups);
                }
                return 0;
            }
            if (sc.rm_R > 0) {
                sc.group_bytes = sc.kp_nseg ? class_rm_pack_bytes(sc) / 2          // packed K: a pack per MFMA group
                                            : -(long long)sc.rm_R * ((sc.w + 63) / 64) * 1024;
                bytes = (size_t)class_rm_pack_bytes(sc) * (sc.masked ? 1 : c->chans);
            } else if (sc.r2) {
                sc.group_bytes = mfma_group_bytes(sc.h + sc.r2 - 1, sc.w, 1);        // h + r2 - 1 rows, the extra ones zero
                bytes = (size_t)sc.group_bytes * ((n_cls + 15) / 16);
            } else {
                sc.group_bytes = sc.kp_nseg ? (long long)c->chans * kp_blocks(sc.h, sc.kp_nseg) * 1024
                                            : mfma_group_bytes(sc.h, sc.w, c->chans);
                bytes = (size_t)sc.group_bytes * groups;
            }
            break;
        case MTM_KERNEL_MFMA_F32:
            sc.group_bytes = bf16_group_bytes(sc.h, sc.w, c->chans);
            bytes = (size_t)(2 * sc.group_bytes * groups);
            break;
        case MTM_KERNEL_MFMA16:
            sc.group_bytes = sc.kp_nseg ? (long long)kp_blocks(sc.h, sc.kp_nseg) * 1024 : mfma_group_bytes(sc.h, sc.w, 1);
            bytes = (size_t)sc.group_bytes * (2 * sc.n_pad / 16);
            sc.tsum_off = ts.take(2 * (size_t)sc.n_pad);
            break;
        default:                              // masked float32 classes on the bf16 screen: the U and V packs
            if (!sc.mask_bf16) return 0;
            sc.mbf_group_bytes = bf16_group_bytes(sc.h, sc.w, 1);
            bytes = (size_t)(2 * sc.mbf_group_bytes * groups);
            sc.mbf_off_u = a.take(bytes);
            sc.mbf_off_v = a.take(bytes);
            return bytes;
    }
    sc.apack_off = a.take(bytes);
    return bytes;
}

// The layout of a placement (no HIP call, no change to the context).  Errors: a template that does not fit the image.
int plan_placement(const mtm_ctx* c, Placement& P) {
    const int n = (int)c->templs.size();
    P.classes = c->classes;
    for (SizeClass& sc : P.classes) {
        sc.kernel = resolved_kernel(c, sc);
        sc.n_pad = (int)round_up(sc.members.size(), 16);
        choose_tiling(c, sc);
        sc.masked_int = sc.masked && sc.kernel == MTM_KERNEL_MFMA;
        sc.mask_bf16 = sc.kernel == MTM_KERNEL_AUTO && masked_bf16_class_ok(c, sc);      // (AUTO: the float64 kernel)
        sc.mbf_off_u = sc.mbf_off_v = sc.tsum_off = -1;
    }
    P.td.assign((size_t)n, TemplDev{});
    for (int i = 0; i < n; ++i) {
        const HostTempl& t = c->templs[i];
        const int kern = P.classes[(size_t)t.cls].kernel;
        if (t.chans != c->chans) {
            set_error("template " + std::to_string(i) + " has a different channel count than the image");
            return MTM_E_INVALID;
        }
        if (t.rows > c->rows || t.cols > c->cols) {
            set_error("template " + std::to_string(i) + " is larger than the image");
            return MTM_E_INVALID;
        }
        TemplDev& d = P.td[i];
        for (int k = 0; k < kMaxChans; ++k) d.mean[k] = t.st.mean[k];
        d.templ_norm = t.st.templ_norm;
        d.templ_sum2 = t.st.templ_sum2;
        d.centred_sum2 = t.st.centred_sum2;
        d.templ2_mask2_sum = t.st.templ2_mask2_sum;
        d.all_ones = t.st.all_ones;
        double sum_t = t.sum_t;  // exact: integers
        if (t.dtype == MTM_U8 && !t.on_device)
            for (size_t k = 0; k < t.px.size(); ++k) sum_t += t.masked ? t.px[k] * t.mask[k] : t.px[k];
        d.mfma_k = 128.0 * sum_t - 16384.0 * (double)t.rows * (double)t.cols * (double)t.chans;
        d.rows = t.rows;
        d.cols = t.cols;
        d.cls = t.cls;
        d.oh = c->rows - t.rows + 1;
        d.ow = c->cols - t.cols + 1;
        d.map_pitch = map_pitch_of(d.ow);
        d.map_off = P.maps.take((size_t)d.map_pitch * d.oh);
        // float64 weights: the float64 / naive kernels, and the exact re-scoring behind the bf16 kernel
        const size_t plane = (size_t)t.chans * t.rows * t.cols;
        const bool want_f64 = kern == MTM_KERNEL_AUTO || kern == MTM_KERNEL_NAIVE || kern == MTM_KERNEL_MFMA_F32;
        d.k1_off = want_f64 ? P.w.take(plane) : -1;
        d.k2_off = want_f64 && t.masked ? P.w.take(plane) : -1;
        const bool dot4 = kern == MTM_KERNEL_DOT4 && c->dtype == MTM_U8 && t.dtype == MTM_U8 && !t.masked;
        d.pack_off = dot4 ? P.p.take(dot_pack_bytes(t.rows, t.cols, t.chans)) : -1;
    }
    // masked classes on the integer path: one dot4 pack of the (shared, binary) mask bytes per class - the dot4 route of
    // sum I^2 M (otherwise: matrix cores)
    for (SizeClass& sc : P.classes)
        sc.mask_pack_off = sc.masked_int && !(c->row_mux && c->fuse_stats) ? P.p.take(dot_pack_bytes(sc.h, sc.w, 1)) : -1;
    // the A arena by family: int8 MFMA, bf16, masked bf16 (U / V), uint16
    P.a_bytes.assign(P.classes.size(), 0);
    for (int fam : {MTM_KERNEL_MFMA, MTM_KERNEL_MFMA_F32, MTM_KERNEL_AUTO, MTM_KERNEL_MFMA16})
        for (size_t k = 0; k < P.classes.size(); ++k)
            if (P.classes[k].kernel == fam) P.a_bytes[k] = place_apacks(c, P.classes[k], P.a, P.ts);
    // classes whose members all live on the device are packed there (after the uploads); the host packs the rest, and
    // reads the pixels of device-resident templates whose kernel (or class mask pack) is host-packed
    P.dev_pack.assign(P.classes.size(), 0);
    for (size_t k = 0; k < P.classes.size(); ++k) {
        const SizeClass& sc = P.classes[k];
        bool all_dev = sc.kernel == MTM_KERNEL_MFMA;
        for (int m : sc.members) all_dev = all_dev && c->templs[(size_t)m].on_device;
        P.dev_pack[k] = all_dev ? 1 : 0;
        P.any_host_pack = P.any_host_pack || (!all_dev && (sc.kernel == MTM_KERNEL_MFMA || sc.kernel == MTM_KERNEL_MFMA16 ||
                                                           sc.kernel == MTM_KERNEL_MFMA_F32));
        P.any_mbf = P.any_mbf || sc.mask_bf16;
    }
    P.any_host_pack = P.any_host_pack || P.any_mbf;
    for (int i = 0; i < n; ++i) {
        const SizeClass& sc = P.classes[(size_t)c->templs[i].cls];
        if (c->templs[i].on_device && !(P.dev_pack[(size_t)c->templs[i].cls] && sc.mask_pack_off < 0)) P.host_px.push_back(i);
    }
    // masked float32 classes: copies of the template table for the U = T M^2 / V = M^2 packs (centre, centred energy, and
    // where the approximate c1 / c2 maps go: the real maps' layout, twice, in a scratch arena of their own)
    if (P.any_mbf) {
        P.td_u = P.td_v = P.td;
        for (const SizeClass& sc : P.classes) {
            if (!sc.mask_bf16) continue;
            for (int m : sc.members) {
                P.td_u[(size_t)m].all_ones = P.td_v[(size_t)m].all_ones = 0;
                P.td_v[(size_t)m].map_off += (long long)P.maps.size;       // second half of the scratch arena
            }
        }
    }
    // template lists: one per class, then the list of templates with a 2-D score map
    for (SizeClass& sc : P.classes) {
        sc.tlist_off = (int)P.tlist.size();
        P.tlist.insert(P.tlist.end(), sc.members.begin(), sc.members.end());
    }
    for (int i = 0; i < n; ++i)
        if (P.td[i].oh > 1 && P.td[i].ow > 1) P.list2d.push_back(i);
    P.list2d_off = (int)P.tlist.size();
    P.tlist.insert(P.tlist.end(), P.list2d.begin(), P.list2d.end());
    // slab views: windows into the units of a large-template class, appended to the unit table (a view of a view:
    // the offsets move, the orientation stays)
    P.units.assign(c->usrc_host.begin(), c->usrc_host.begin() + (long)std::min(c->usrc_units, c->usrc_host.size()));
    for (SizeClass& sc : P.classes)
        for (auto& sl : sc.slabs) {
            sl.tlist_off = (int)P.tlist.size();
            for (int m : sc.members) {
                UnitSrc v = c->templs[(size_t)m].src;
                v.off += (long long)sl.ch * v.sh * v.sw;
                v.moff = -1;
                v.cy += v.ay * sl.r0 + v.by * sl.c0;
                v.cx += v.ax * sl.r0 + v.bx * sl.c0;
                v.h = sl.r1 - sl.r0;
                v.w = sl.c1 - sl.c0;
                v.chans = 1;
                P.tlist.push_back((int)P.units.size());
                P.units.push_back(v);
            }
        }
    return MTM_OK;
}

// The host-packed operands of a plan; the centres of the bf16 packs go to the plan's template tables.
struct HostArenas {
    std::vector<double> wts, tsums;
    std::vector<uint8_t> packs, apacks;
};
void pack_on_host(const mtm_ctx* c, Placement& P, HostArenas& H) {
    H.wts.resize(P.w.size);
    H.packs.resize(P.p.size);
    H.apacks.resize(P.any_host_pack ? P.a.size : 0);
    H.tsums.resize(P.ts.size);
    uint8_t* a = H.apacks.data();
    for (size_t i = 0; i < P.td.size(); ++i) {
        const HostTempl& t = c->templs[i];
        const TemplDev& d = P.td[i];
        if (d.k1_off >= 0 && t.masked) {        // weights (float64): K1 = T (or T*M^2), K2 = M^2
            for (size_t k = 0; k < t.px.size(); ++k) {
                const double m2 = t.mask[k] * t.mask[k];
                H.wts[d.k1_off + k] = t.px[k] * m2;
                H.wts[d.k2_off + k] = m2;
            }
        } else if (d.k1_off >= 0) {
            std::copy(t.px.begin(), t.px.end(), H.wts.begin() + d.k1_off);
        }
        if (d.pack_off >= 0) pack_template_dot4(t, H.packs.data() + d.pack_off);
    }
    for (size_t k = 0; k < P.classes.size(); ++k) {
        const SizeClass& sc = P.classes[k];
        if (sc.mask_pack_off >= 0) {
            HostTempl mk = c->templs[sc.members[0]];
            for (size_t q = 0; q < mk.px.size(); ++q) mk.px[q] = mk.mask[q] > 0.0 ? 255.0 : 0.0;
            pack_template_dot4(mk, H.packs.data() + sc.mask_pack_off);
        }
        if (sc.mask_bf16) {
            pack_class_bf16(c, sc, a + sc.mbf_off_u, sc.mbf_group_bytes, P.a_bytes[k], P.td_u, 1);
            pack_class_bf16(c, sc, a + sc.mbf_off_v, sc.mbf_group_bytes, P.a_bytes[k], P.td_v, 2);
        }
        if (P.dev_pack[k]) continue;
        if (sc.kernel == MTM_KERNEL_MFMA && sc.mask_rm_off >= 0) pack_mask_rm(c, sc, a + sc.mask_rm_off);
        if (sc.kernel == MTM_KERNEL_MFMA && sc.rm_R > 0)
            pack_class_rm(c, sc, a + sc.apack_off, P.a_bytes[k]);
        else if (sc.kernel == MTM_KERNEL_MFMA)
            pack_class_mfma(c, sc, a + sc.apack_off, P.a_bytes[k]);
        if (sc.kernel == MTM_KERNEL_MFMA16) pack_class_mfma16(c, sc, a + sc.apack_off, P.a_bytes[k], H.tsums.data() + sc.tsum_off);
        if (sc.kernel == MTM_KERNEL_MFMA_F32) pack_class_bf16(c, sc, a + sc.apack_off, sc.group_bytes, P.a_bytes[k], P.td, 0);
    }
}

// Uploads a plan and its host-packed operands, packs the device-packed classes and hands the tables to the context.
int upload_placement(mtm_ctx* c, Placement& P, HostArenas& H) {
    // From here on copies from P's and H's vectors are in flight: an error return drains the stream before they go out of
    // scope (the normal path hands the long-lived ones to the context and says so in place_pending).
    struct DrainGuard {
        hipStream_t s;
        bool armed = true;
        ~DrainGuard() {
            if (armed) (void)hipStreamSynchronize(s);
        }
    } drain{c->stream};
    const size_t n = P.td.size(), a_off = P.a.size, w_off = P.w.size, p_off = P.p.size, ts_off = P.ts.size;
    const bool new_units = P.units.size() > c->usrc_units;
    if (new_units) {
        MTMC(c->usrc_dev.ensure(sizeof(UnitSrc) * P.units.size()));
        HIPC(hipMemcpyAsync(c->usrc_dev.p, P.units.data(), sizeof(UnitSrc) * P.units.size(), hipMemcpyHostToDevice, c->stream));
    }
    MTMC(c->td.ensure(sizeof(TemplDev) * n));
    MTMC(c->tlist.ensure(sizeof(int) * std::max<size_t>(1, P.tlist.size())));
    MTMC(c->weights.ensure(sizeof(double) * std::max<size_t>(1, w_off)));
    MTMC(c->packs.ensure(std::max<size_t>(4, p_off)));
    MTMC(c->apacks.ensure(std::max<size_t>(16, a_off) + 16384));     // the K loop requests up to two steps past a pack
    // host-packed classes (device-packed regions of the same arena are written afterwards, in stream order, by
    // pack_units_kernel below)
    if (a_off && P.any_host_pack) HIPC(hipMemcpyAsync(c->apacks.p, H.apacks.data(), a_off, hipMemcpyHostToDevice, c->stream));
    // the score-map arena (4 bytes per pixel and template) is only allocated when something writes maps:
    // mtm_find_matches in hits-only mode never does (ensure_maps, called by the launch paths)
    HIPC(hipMemcpyAsync(c->td.p, P.td.data(), sizeof(TemplDev) * n, hipMemcpyHostToDevice, c->stream));
    if (!P.tlist.empty())
        HIPC(hipMemcpyAsync(c->tlist.p, P.tlist.data(), sizeof(int) * P.tlist.size(), hipMemcpyHostToDevice, c->stream));
    if (w_off) HIPC(hipMemcpyAsync(c->weights.p, H.wts.data(), sizeof(double) * w_off, hipMemcpyHostToDevice, c->stream));
    if (p_off) HIPC(hipMemcpyAsync(c->packs.p, H.packs.data(), p_off, hipMemcpyHostToDevice, c->stream));
    if (P.any_mbf) {
        MTMC(c->td_u.ensure(sizeof(TemplDev) * n));
        MTMC(c->td_v.ensure(sizeof(TemplDev) * n));
        HIPC(hipMemcpyAsync(c->td_u.p, P.td_u.data(), sizeof(TemplDev) * n, hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemcpyAsync(c->td_v.p, P.td_v.data(), sizeof(TemplDev) * n, hipMemcpyHostToDevice, c->stream));
    }
    MTMC(c->tsum.ensure(sizeof(double) * std::max<size_t>(2, ts_off)));
    if (ts_off) HIPC(hipMemcpyAsync(c->tsum.p, H.tsums.data(), sizeof(double) * ts_off, hipMemcpyHostToDevice, c->stream));
    // device-side packing: gathers the A operands straight from the unit views (the template list is in place)
    for (size_t k = 0; k < P.classes.size(); ++k)
        if (P.dev_pack[k]) MTMC(pack_class_on_device(c, P.classes[k]));
    // the tail screen's constants, from the packs just placed (host- or device-packed alike)
    for (const SizeClass& sc : P.classes)
        if (sc.tail_split > 0 && sc.kernel == MTM_KERNEL_MFMA && !sc.members.empty())
            MTMC(queue_tail_consts(c, sc, sc.tail_split, c->stream));
    // host staging vectors go out of scope; the tables that stay in the context (td, tlist) need no wait
    // (set_templates_device)
    const bool local_sources = P.any_host_pack || P.any_mbf || w_off || p_off || ts_off || new_units;
    if (local_sources) HIPC(hipStreamSynchronize(c->stream));
    c->place_pending = !local_sources;
    drain.armed = false;
    if (new_units) c->usrc_host.swap(P.units);
    c->classes.swap(P.classes);
    c->tail_valid.assign(c->classes.size(), 0);
    c->tail_last.assign(c->classes.size(), 0);
    c->dot_last.assign(c->classes.size(), -1);
    for (size_t k = 0; k < c->classes.size(); ++k) {
        const SizeClass& sc = c->classes[k];
        if (sc.tail_split > 0 && sc.kernel == MTM_KERNEL_MFMA && !sc.members.empty()) c->tail_valid[k] = sc.tail_split;
    }
    c->td_host.swap(P.td);
    c->tlist_host.swap(P.tlist);
    c->list2d.swap(P.list2d);
    c->list2d_off = P.list2d_off;
    c->maps_floats = P.maps.size;
    c->placed = true;
    return MTM_OK;
}

}  // namespace

namespace mtmi {

int launch_tail_consts(mtm_ctx* c, const SizeClass& sc, int split, hipStream_t stream) { return queue_tail_consts(c, sc, split, stream); }

int place_templates(mtm_ctx* c) {
    if (!c->have_image || !c->have_templ) {
        set_error("set the image and the templates first");
        return MTM_E_STATE;
    }
    if (c->placed) return MTM_OK;
    if (c->place_pending) {             // the previous placement's tables are released below: their copies first
        HIPC(hipStreamSynchronize(c->stream));
        c->place_pending = false;
    }
    // Everything is derived into the plan and committed at the end: a failure half-way (an allocation, a copy) leaves the
    // context as it was - templates set, not placed (the host copies of device-resident templates may have been fetched).
    Placement P;
    MTMC(plan_placement(c, P));
    for (int i : P.host_px) MTMC(ensure_host_pixels(c, i));
    HostArenas H;
    pack_on_host(c, P, H);
    return upload_placement(c, P, H);
}

// The templates of the last mtm_set_templates, read back from the bytes the context keeps of them (mtm_ctx::templ_blob,
// written by set_templates_impl: n_templ, method, n_var, then per template {rows, cols, chans, dtype, has_mask} + rows).
// Unmasked uint8 templates; with `u16_ok` also unmasked single-channel uint16 ones.
int parse_templ_blob(const std::vector<uint8_t>& b, std::vector<BlobTempl>& out, const char* who, bool u16_ok) {
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
        const bool u16 = u16_ok && hdr[3] == MTM_U16 && hdr[2] == 1;
        if ((hdr[3] != MTM_U8 && !u16) || hdr[4] != 0) {
            set_error(std::string(who) + ": template " + std::to_string(i) +
                      (u16_ok ? " is not an unmasked uint8 or single-channel uint16 template"
                              : " is not an unmasked uint8 template"));
            return MTM_E_INVALID;
        }
        const size_t bytes = (size_t)hdr[0] * hdr[1] * hdr[2] * (u16 ? 2 : 1);
        if (off + bytes > b.size()) return MTM_E_STATE;
        out.push_back(BlobTempl{hdr[0], hdr[1], hdr[2], hdr[3], b.data() + off});
        off += bytes;
    }
    return MTM_OK;
}

// The byte planes of every template for the window searches (mtm_find_matches_pyramid / _boxes): uint8 [C][h][w], a
// single-channel uint16 template its high bytes, then its low bytes; template t's at win_tpx + win_toff[t].  Built once
// per template set (win_gen).
int prepare_window_templates(mtm_ctx* c, const std::vector<BlobTempl>& tl) {
    if (c->win_gen != c->templ_gen && !c->win_blob.empty() && c->win_blob == c->templ_blob) {
        // the set they were made from, set again after others (sets used in turn on one context): every cache made for
        // it moves to the new generation
        if (c->pyr_gen == c->win_gen) c->pyr_gen = c->templ_gen;
        if (c->box_gen == c->win_gen) c->box_gen = c->templ_gen;
        c->win_gen = c->templ_gen;
    }
    if (c->win_gen == c->templ_gen) return MTM_OK;
    c->win_gen = 0;
    c->win_blob.clear();
    const size_t n = tl.size();
    std::vector<uint8_t> planar;
    std::vector<long long> toff(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const BlobTempl& t = tl[i];
        const size_t plane = (size_t)t.rows * t.cols;
        toff[i] = (long long)planar.size();
        if (t.dtype == MTM_U16) {
            planar.resize(planar.size() + 2 * plane);
            uint8_t* dst = planar.data() + toff[i];
            for (size_t p = 0; p < plane; ++p) {
                uint16_t v;
                std::memcpy(&v, t.px + 2 * p, sizeof(v));
                dst[p] = (uint8_t)(v >> 8);
                dst[plane + p] = (uint8_t)(v & 255u);
            }
        } else {
            planar.resize(planar.size() + plane * t.chans);
            uint8_t* dst = planar.data() + toff[i];
            for (size_t p = 0; p < plane; ++p)
                for (int k = 0; k < t.chans; ++k) dst[(size_t)k * plane + p] = t.px[p * t.chans + k];
        }
    }
    if (!planar.empty()) {
        MTMC(c->win_tpx.ensure(planar.size()));
        HIPC(hipMemcpy(c->win_tpx.p, planar.data(), planar.size(), hipMemcpyHostToDevice));
    }
    if (n > 0) {
        MTMC(c->win_toff.ensure(sizeof(long long) * n));
        HIPC(hipMemcpy(c->win_toff.p, toff.data(), sizeof(long long) * n, hipMemcpyHostToDevice));
    }
    c->win_blob = c->templ_blob;
    c->win_gen = c->templ_gen;
    return MTM_OK;
}

}  // namespace mtmi

extern "C" {

namespace {

// unit (y, x) -> source (row, col) of a view, composed from the augmentation steps (numpy semantics)
struct View {
    int ay = 1, by = 0, cy = 0, ax = 0, bx = 1, cx = 0, h = 0, w = 0;
    void fliplr() {                  // new(y, x) = cur(y, w - 1 - x)
        cy += by * (w - 1);
        cx += bx * (w - 1);
        by = -by;
        bx = -bx;
    }
    void flipud() {                  // new(y, x) = cur(h - 1 - y, x)
        cy += ay * (h - 1);
        cx += ax * (h - 1);
        ay = -ay;
        ax = -ax;
    }
    void rot90() {                   // np.rot90: new(i, j) = cur(j, w - 1 - i); new dims (w, h)
        const int nay = -by, nby = ay, ncy = cy + by * (w - 1);
        const int nax = -bx, nbx = ax, ncx = cx + bx * (w - 1);
        ay = nay; by = nby; cy = ncy;
        ax = nax; bx = nbx; cx = ncx;
        std::swap(h, w);
    }
};

inline unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// uint8 template sets, plain or augmented: the bases go to the device source arena (planar), resized copies are
// made there, every unit becomes a view (UnitSrc), statistics come from exact sums per source - on the host for
// the bases (one pass over the bytes that are being copied anyway), by a device reduction for resized copies.
// No per-unit pixel work on the host, no per-unit upload.
int set_templates_device(mtm_ctx* c, const mtm_templ* bases, int n_bases, const mtm_variant* variants, int n_var,
                         int method, std::vector<HostTempl>& hts) {
    HIPC(hipSetDevice(c->device));
    static const mtm_variant kIdentity = {0, 0, 0, 0, 0, 0};
    if (n_var <= 0) {
        variants = &kIdentity;
        n_var = 1;
    }
    struct Source {
        long long off = 0, moff = -1;
        int sh = 0, sw = 0, chans = 0;
        bool on_host = false;                       // sums computed on the host
        double s[kMaxChans] = {0, 0, 0, 0}, sq[kMaxChans] = {0, 0, 0, 0}, sm[kMaxChans] = {0, 0, 0, 0},
               sqm[kMaxChans] = {0, 0, 0, 0}, mones = 0.0;
        unsigned long long mask_hash = 0;
    };
    std::vector<Source> srcs;
    // The host image of the arena prefix (the bases), the unit table and - place_templates - the constants tables are
    // copied from context-owned vectors that live until the next template set: no host wait for those copies here, the
    // template work queues ahead of the call's image upload and runs under it.  Before the vectors are rewritten the
    // stream is drained (idle by then in any ordinary sequence of calls).
    if (c->stage_pending) {
        HIPC(hipStreamSynchronize(c->stream));
        c->stage_pending = false;
    }
    std::vector<uint8_t>& stage = c->tstage;
    stage.clear();
    auto alloc = [&](size_t& cursor, size_t bytes) {
        const size_t off = cursor;
        cursor = round_up(cursor + bytes, 16);
        return (long long)off;
    };
    size_t cursor = 0;
    // ---- bases: planarise into the staging image, exact sums on the way
    for (int b = 0; b < n_bases; ++b) {
        const mtm_templ& t = bases[b];
        Source sc;
        sc.sh = t.rows;
        sc.sw = t.cols;
        sc.chans = t.chans;
        sc.on_host = true;
        const size_t plane = (size_t)t.rows * t.cols, n = plane * t.chans;
        sc.off = alloc(cursor, n);
        if (t.mask) sc.moff = alloc(cursor, n);
        stage.resize(cursor);
        uint8_t* dpx = stage.data() + sc.off;
        uint8_t* dmk = t.mask ? stage.data() + sc.moff : nullptr;
        unsigned long long mh = 1469598103934665603ull;
        for (int ch = 0; ch < t.chans; ++ch) {
            unsigned long long s = 0, sq = 0, sm = 0, sqm = 0, ones = 0;
            for (int y = 0; y < t.rows; ++y) {
                const uint8_t* rp = (const uint8_t*)t.px + (size_t)y * t.row_stride + ch;
                const uint8_t* mp = t.mask ? (const uint8_t*)t.mask + (size_t)y * t.mask_row_stride + ch : nullptr;
                uint8_t* o = dpx + ch * plane + (size_t)y * t.cols;
                uint8_t* om = dmk ? dmk + ch * plane + (size_t)y * t.cols : nullptr;
                if (t.chans == 1 && !mp) {       // the common case: a row is a run of bytes
                    std::memcpy(o, rp, (size_t)t.cols);
                    u8_run_sums(rp, (size_t)t.cols, &s, &sq);
                    continue;
                }
                for (int x = 0; x < t.cols; ++x) {
                    const unsigned v = rp[(size_t)x * t.chans];
                    o[x] = (uint8_t)v;
                    s += v;
                    sq += v * v;
                    if (mp) {
                        // the arena keeps the mask bytes as given (a resized mask is the resize of THOSE bytes);
                        // every reader binarises: CV_8U masks are binary masks (matchTemplateMask)
                        om[x] = mp[(size_t)x * t.chans];
                        const unsigned m = om[x] > 0 ? 1u : 0u;
                        sm += v * m;
                        sqm += v * v * m;
                        ones += m;
                    }
                }
                if (om) mh = fnv(mh, om, (size_t)t.cols);
            }
            sc.s[ch] = (double)s;
            sc.sq[ch] = (double)sq;
            sc.sm[ch] = (double)sm;
            sc.sqm[ch] = (double)sqm;
            if (ch == 0) sc.mones = (double)ones;
        }
        sc.mask_hash = t.mask ? mh : 0ull;
        srcs.push_back(sc);
    }
    // ---- resized copies: one source per (base, resize rule), shared by the variants that use it
    struct Resize { int rows, cols, down; };
    std::vector<Resize> rules;
    std::vector<int> rule_of_var((size_t)n_var, -1);
    for (int v = 0; v < n_var; ++v) {
        const mtm_variant& q = variants[v];
        if (q.rot90 < 0 || q.rot90 > 3 || q.rows < 0 || q.cols < 0 || q.down < 0 || ((q.rows > 0) != (q.cols > 0)) ||
            (q.rows > 0 && q.down > 1)) {
            set_error("mtm_set_templates_augmented: bad variant " + std::to_string(v));
            return MTM_E_INVALID;
        }
        if (q.rows == 0 && q.down <= 1) continue;
        for (size_t r = 0; r < rules.size(); ++r)
            if (rules[r].rows == q.rows && rules[r].cols == q.cols && rules[r].down == (q.down > 1 ? q.down : 0)) rule_of_var[(size_t)v] = (int)r;
        if (rule_of_var[(size_t)v] < 0) {
            rule_of_var[(size_t)v] = (int)rules.size();
            rules.push_back(Resize{q.rows, q.cols, q.down > 1 ? q.down : 0});
        }
    }
    const size_t n_host_src = srcs.size();
    for (int b = 0; b < n_bases; ++b)
        for (size_t r = 0; r < rules.size(); ++r) {
            const Source& base = srcs[(size_t)b];
            Source sc;
            sc.chans = base.chans;
            sc.sh = rules[r].down ? base.sh / rules[r].down : rules[r].rows;
            sc.sw = rules[r].down ? base.sw / rules[r].down : rules[r].cols;
            if (sc.sh < 1 || sc.sw < 1) {
                set_error("mtm_set_templates_augmented: a resize leaves no pixel of base " + std::to_string(b));
                return MTM_E_INVALID;
            }
            const size_t n = (size_t)sc.sh * sc.sw * sc.chans;
            sc.off = alloc(cursor, n);
            if (base.moff >= 0) sc.moff = alloc(cursor, n);
            const int key[4] = {sc.sh, sc.sw, rules[r].down, 0};
            sc.mask_hash = base.moff >= 0 ? fnv(base.mask_hash, key, sizeof(key)) : 0ull;
            srcs.push_back(sc);
        }
    MTMC(c->tsrc.ensure(std::max<size_t>(16, cursor)));
    // (set BEFORE the copy is queued: an error return further down must not leave a copy from `tstage` in flight unrecorded)
    c->stage_pending = true;
    if (!stage.empty()) HIPC(hipMemcpyAsync(c->tsrc.p, stage.data(), stage.size(), hipMemcpyHostToDevice, c->stream));
    uint8_t* arena = c->tsrc.as<uint8_t>();
    for (int b = 0; b < n_bases; ++b)
        for (size_t r = 0; r < rules.size(); ++r) {
            const Source& base = srcs[(size_t)b];
            const Source& d = srcs[n_host_src + (size_t)b * rules.size() + r];
            const dim3 grd((d.sw + 63) / 64, d.sh, d.chans);
            for (int pass = 0; pass < (base.moff >= 0 ? 2 : 1); ++pass) {
                const uint8_t* sp = arena + (pass ? base.moff : base.off);
                uint8_t* dp = arena + (pass ? d.moff : d.off);
                if (rules[r].down)
                    hipLaunchKernelGGL(downscale_int_kernel, grd, dim3(64), 0, c->stream, sp, base.sh, base.sw, dp, rules[r].down,
                                       d.chans);
                else
                    hipLaunchKernelGGL(resize_area_kernel, grd, dim3(64), 0, c->stream, sp, base.sh, base.sw, dp, d.sh, d.sw,
                                       d.chans);
            }
        }
    // exact sums of the device-made sources: one reduction, one small copy back
    if (srcs.size() > n_host_src) {
        const size_t nd = srcs.size() - n_host_src;
        std::vector<SourceDesc> desc(nd);
        for (size_t k = 0; k < nd; ++k) {
            const Source& d = srcs[n_host_src + k];
            desc[k] = SourceDesc{d.off, d.moff, d.sh, d.sw, d.chans, 0};
        }
        MTMC(c->tsums_dev.ensure(sizeof(SourceDesc) * nd + sizeof(unsigned long long) * kSumsPerSource * nd));
        SourceDesc* ddesc = c->tsums_dev.as<SourceDesc>();
        unsigned long long* dsums = reinterpret_cast<unsigned long long*>(c->tsums_dev.as<uint8_t>() + sizeof(SourceDesc) * nd);
        HIPC(hipMemcpyAsync(ddesc, desc.data(), sizeof(SourceDesc) * nd, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(source_sums_kernel, dim3((unsigned)nd), dim3(256), 0, c->stream, arena, ddesc, dsums);
        HIPC(hipGetLastError());
        std::vector<unsigned long long> sums((size_t)kSumsPerSource * nd);
        HIPC(hipMemcpyAsync(sums.data(), dsums, sizeof(unsigned long long) * sums.size(), hipMemcpyDeviceToHost, c->stream));
        HIPC(hipStreamSynchronize(c->stream));
        for (size_t k = 0; k < nd; ++k) {
            Source& d = srcs[n_host_src + k];
            const unsigned long long* q = sums.data() + k * kSumsPerSource;
            for (int ch = 0; ch < d.chans; ++ch) {
                d.s[ch] = (double)q[4 * ch + 0];
                d.sq[ch] = (double)q[4 * ch + 1];
                d.sm[ch] = (double)q[4 * ch + 2];
                d.sqm[ch] = (double)q[4 * ch + 3];
            }
            d.mones = (double)q[4 * kMaxChans];
        }
    }
    // ---- units: base-major, variants in the order given
    const int n_units = n_bases * n_var;
    hts.assign((size_t)n_units, HostTempl{});
    std::vector<UnitSrc> units((size_t)n_units);
    for (int b = 0; b < n_bases; ++b)
        for (int v = 0; v < n_var; ++v) {
            const mtm_variant& q = variants[v];
            const Source& sc = rule_of_var[(size_t)v] < 0 ? srcs[(size_t)b]
                                                          : srcs[n_host_src + (size_t)b * rules.size() + (size_t)rule_of_var[(size_t)v]];
            View vw;
            vw.h = sc.sh;
            vw.w = sc.sw;
            if (q.flip_lr) vw.fliplr();
            if (q.flip_ud) vw.flipud();
            for (int k = 0; k < q.rot90; ++k) vw.rot90();
            const int ui = b * n_var + v;
            UnitSrc& u = units[(size_t)ui];
            u = UnitSrc{sc.off, sc.moff, sc.sh, sc.sw, vw.ay, vw.by, vw.cy, vw.ax, vw.bx, vw.cx, vw.h, vw.w, sc.chans, 0};
            HostTempl& t = hts[(size_t)ui];
            t.rows = vw.h;
            t.cols = vw.w;
            t.chans = sc.chans;
            t.dtype = MTM_U8;
            t.masked = sc.moff >= 0;
            t.on_device = true;
            t.src = u;
            double tm2 = 0.0;
            for (int ch = 0; ch < sc.chans; ++ch) {
                t.sum_t += t.masked ? sc.sm[ch] : sc.s[ch];
                tm2 += sc.sqm[ch];
            }
            t.mask_ones = sc.mones;
            t.st = templ_stats_from_sums(sc.s, sc.sq, tm2, t.masked, t.rows, t.cols, t.chans, method);
            if (t.masked) {
                const int key[8] = {vw.ay, vw.by, vw.cy, vw.ax, vw.bx, vw.cx, vw.h, vw.w};
                t.mask_key = fnv(sc.mask_hash, key, sizeof(key));
                if (t.mask_key == 0) t.mask_key = 1;
            }
        }
    MTMC(c->usrc_dev.ensure(sizeof(UnitSrc) * std::max<size_t>(1, units.size())));
    if (!units.empty())
        HIPC(hipMemcpyAsync(c->usrc_dev.p, units.data(), sizeof(UnitSrc) * units.size(), hipMemcpyHostToDevice, c->stream));
    c->usrc_units = units.size();
    c->usrc_host.swap(units);                   // (the previous table - now `units` - was drained above)
    c->stage_pending = true;
    return MTM_OK;
}

int set_templates_impl(mtm_ctx* c, const mtm_templ* templs, int n_templ, const mtm_variant* variants, int n_var, int method,
                       const char* who);

}  // namespace

int mtm_set_templates(mtm_ctx* c, const mtm_templ* templs, int n_templ, int method) {
    return set_templates_impl(c, templs, n_templ, nullptr, 0, method, "mtm_set_templates");
}

int mtm_set_templates_augmented(mtm_ctx* c, const mtm_templ* bases, int n_bases, const mtm_variant* variants, int n_variants,
                                int method) {
    if (n_variants < 1 || !variants) {
        set_error("mtm_set_templates_augmented: at least one variant is needed");
        return MTM_E_INVALID;
    }
    return set_templates_impl(c, bases, n_bases, variants, n_variants, method, "mtm_set_templates_augmented");
}

namespace {

// Templates of other pixel types, or with MTM_TEMPL_ON_DEVICE=0: planar float64 copies on the host, statistics.
void host_templates(const mtm_templ* templs, int n_templ, int method, std::vector<HostTempl>& hts) {
    hts.assign((size_t)n_templ, HostTempl{});
    for (int i = 0; i < n_templ; ++i) {
        const mtm_templ& s = templs[i];
        HostTempl& t = hts[i];
        t.rows = s.rows;
        t.cols = s.cols;
        t.chans = s.chans;
        t.dtype = s.dtype;
        t.masked = s.mask != nullptr;
        const size_t plane = (size_t)s.rows * s.cols;
        t.px.resize(plane * s.chans);
        if (t.masked) t.mask.resize(plane * s.chans);
        for (int y = 0; y < s.rows; ++y) {
            const uint8_t* rp = (const uint8_t*)s.px + (size_t)y * s.row_stride;
            const uint8_t* mp = t.masked ? (const uint8_t*)s.mask + (size_t)y * s.mask_row_stride : nullptr;
            for (int x = 0; x < s.cols; ++x)
                for (int k = 0; k < s.chans; ++k) {
                    const size_t src = (size_t)x * s.chans + k;
                    const size_t dst = (size_t)k * plane + (size_t)y * s.cols + x;
                    if (s.dtype == MTM_U8) {
                        t.px[dst] = (double)rp[src];
                        // CV_8U masks are binary masks (matchTemplateMask)
                        if (mp) t.mask[dst] = mp[src] > 0 ? 1.0 : 0.0;
                    } else if (s.dtype == MTM_U16) {
                        // the reference casts uint16 to float32 (exact) before cv2 (MTM/__init__.py:71-74):
                        // a mask is then a float32 weight image, not a binary mask
                        t.px[dst] = (double)((const uint16_t*)rp)[src];
                        if (mp) t.mask[dst] = (double)((const uint16_t*)mp)[src];
                    } else {
                        t.px[dst] = (double)((const float*)rp)[src];
                        if (mp) t.mask[dst] = (double)((const float*)mp)[src];
                    }
                }
        }
        t.st = compute_templ_stats(t.px.data(), t.masked ? t.mask.data() : nullptr, t.rows, t.cols, t.chans,
                                   method, s.dtype == MTM_U8 || s.dtype == MTM_U16);
    }
}

// Size classes, in order of first appearance; every template's `cls`.
void size_classes(std::vector<HostTempl>& hts, std::vector<SizeClass>& classes) {
    // masked templates only share a class (and its masked window statistics) when their masks are equal
    auto mask_hash = [](const HostTempl& t) {
        unsigned long long hsh = 1469598103934665603ull;
        for (double v : t.mask) {
            unsigned long long bits;
            std::memcpy(&bits, &v, 8);
            hsh = (hsh ^ bits) * 1099511628211ull;
        }
        if (t.on_device) return t.masked ? t.mask_key : 0ull;
        return t.masked ? hsh : 0ull;
    };
    std::map<std::tuple<int, int, bool, unsigned long long>, int> index;
    for (size_t i = 0; i < hts.size(); ++i) {
        const auto key = std::make_tuple(hts[i].rows, hts[i].cols, hts[i].masked, mask_hash(hts[i]));
        auto it = index.find(key);
        if (it == index.end()) {
            SizeClass sc;
            sc.h = hts[i].rows;
            sc.w = hts[i].cols;
            sc.masked = hts[i].masked;
            sc.mask_hash = std::get<3>(key);
            it = index.emplace(key, (int)classes.size()).first;
            classes.push_back(sc);
        }
        SizeClass& sc = classes[it->second];
        sc.members.push_back((int)i);
        sc.all_u8 = sc.all_u8 && hts[i].dtype == MTM_U8;
        sc.all_u16 = sc.all_u16 && hts[i].dtype == MTM_U16;
        sc.all_f32 = sc.all_f32 && hts[i].dtype == MTM_F32;
        hts[i].cls = it->second;
    }
}

int set_templates_impl(mtm_ctx* c, const mtm_templ* templs, int n_templ, const mtm_variant* variants, int n_var, int method,
                       const char* who) {
    if (!c || n_templ < 0 || (n_templ > 0 && !templs) || method < 0 || method > 5) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    bool all_u8 = true;
    for (int i = 0; i < n_templ; ++i) {
        const mtm_templ& s = templs[i];
        if (!s.px || s.rows <= 0 || s.cols <= 0 || s.chans < 1 || s.chans > kMaxChans ||
            (s.dtype != MTM_U8 && s.dtype != MTM_F32 && s.dtype != MTM_U16)) {
            set_error(std::string(who) + ": bad template " + std::to_string(i));
            return MTM_E_INVALID;
        }
        all_u8 = all_u8 && s.dtype == MTM_U8;
    }
    if (n_var > 0 && !all_u8) {
        set_error("mtm_set_templates_augmented takes uint8 bases (augment other pixel types on the host)");
        return MTM_E_INVALID;
    }
    // The same templates again (a loop of matchTemplates calls over different images): keep everything that
    // was derived from them - statistics, size classes, device packs.  The test is on the pixel bytes: the
    // caller's rows are compared in place with the copy kept from the call that built the current state.
    {
        auto walk = [&](auto&& emit) {
            emit(&n_templ, sizeof(n_templ));
            emit(&method, sizeof(method));
            emit(&n_var, sizeof(n_var));
            if (n_var > 0) emit(variants, sizeof(mtm_variant) * (size_t)n_var);
            for (int i = 0; i < n_templ; ++i) {
                const mtm_templ& s = templs[i];
                const int hdr[5] = {s.rows, s.cols, s.chans, s.dtype, s.mask ? 1 : 0};
                emit(hdr, sizeof(hdr));
                const size_t row = (size_t)s.cols * s.chans * elem_size(s.dtype);
                if (!s.mask && s.row_stride == (int64_t)row) {      // contiguous template: one piece
                    emit(s.px, row * s.rows);
                    continue;
                }
                for (int y = 0; y < s.rows; ++y) {
                    emit((const uint8_t*)s.px + (size_t)y * s.row_stride, row);
                    if (s.mask) emit((const uint8_t*)s.mask + (size_t)y * s.mask_row_stride, row);
                }
            }
        };
        if (c->have_templ) {
            size_t off = 0;
            bool same = true;
            const std::vector<uint8_t>& old = c->templ_blob;
            walk([&](const void* p, size_t n) {
                if (!same) return;
                if (off + n > old.size() || std::memcmp(old.data() + off, p, n) != 0) same = false;
                off += n;
            });
            if (same && off == old.size()) return MTM_OK;
        }
        std::vector<uint8_t> blob;
        size_t total = 0;
        walk([&](const void*, size_t n) { total += n; });
        blob.reserve(total);
        walk([&](const void* p, size_t n) { blob.insert(blob.end(), (const uint8_t*)p, (const uint8_t*)p + n); });
        c->templ_blob.swap(blob);
        ++c->templ_gen;
        c->have_templ = false;          // until the new set is complete
    }
    std::vector<HostTempl> hts;
    if (all_u8 && (c->templ_on_device || n_var > 0)) {       // augmented sets only exist as device views
        const int rc = set_templates_device(c, templs, n_templ, variants, n_var, method, hts);
        if (rc != MTM_OK) {
            c->templ_blob.clear();
            ++c->templ_gen;
            return rc;
        }
    } else {
        host_templates(templs, n_templ, method, hts);
    }
    std::vector<SizeClass> classes;
    size_classes(hts, classes);
    c->templs.swap(hts);
    c->classes.swap(classes);
    c->method = method;
    c->have_templ = true;
    c->placed = false;
    return MTM_OK;
}

}  // namespace

}  // extern "C"
