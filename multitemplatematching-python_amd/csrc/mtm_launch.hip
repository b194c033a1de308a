// libmtm_hip.so - the score pass: the score maps of a size class on whichever kernel runs it (launch_ncc and one launcher
// per kernel family), the sum I^2 M pass of masked classes, the masked float32 screen, the float32 refinement behind the
// bf16 kernel, and the score pass of a whole call - classes over lanes, plain and with a banded image upload.  The window
// statistics a score launch reads come from launch_stats (mtm_stats.hip).
#include "mtm_ctx.h"

using namespace mtm;
using namespace mtmi;
#include "mtm_k_score.hip.h"
#include "mtm_refine.hip.h"
#include "mtm_maskf32.hip.h"

namespace {

// dot4 kernel variants
struct DotVariant {
    int px, py, nt;
    bool wide;
    void (*fn)(DotParams, const TemplDev*, const int*, const uint8_t*, StatPlanes, float*);
};
#define DOTV(PX, PY, NT, W) {PX, PY, NT, W, ncc_dot4_kernel<PX, PY, NT, W>}
const DotVariant kDotVariants[] = {
    DOTV(4, 4, 4, false),   // 0: default
    DOTV(4, 4, 2, false),   // 1
    DOTV(8, 2, 4, false),   // 2
    DOTV(8, 4, 2, false),   // 3
    DOTV(4, 2, 4, false),   // 4
    DOTV(8, 2, 2, false),   // 5
    DOTV(4, 2, 8, false),   // 6
    DOTV(4, 2, 2, true),    // 7: uint64 totals for templates with C*w*h*255^2 >= 2^32
};
constexpr int kDotWideVariant = 7;
constexpr int kNumDotVariants = sizeof(kDotVariants) / sizeof(kDotVariants[0]);

// raw-mode instantiations of ncc_mfma_kernel (biased int32 accumulators stored as they are)
MfmaFn mfma_raw_fn(bool row_mux, bool packed_k) {
    MfmaSel s;
    s.method = kMfRaw;
    s.rm = row_mux;
    s.kp = packed_k;
    return mfma_kernel(s);
}

// the index of `sc` among the context's size classes; -1: a class that is not the context's (a caller's own record)
int class_index(const mtm_ctx* c, const SizeClass& sc) {
    const bool mine = !c->classes.empty() && &sc >= c->classes.data() && &sc < c->classes.data() + c->classes.size();
    return mine ? (int)(&sc - c->classes.data()) : -1;
}

// work items in whole groups of 8 work-groups
dim3 work_grid(int n_work) { return dim3((unsigned)(((n_work + 7) / 8) * 8)); }

// the timing event pair `i` of `evs` (mtm_ctx::ncc_ev, sq_ev), created on first use
int event_pair(std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs, int i, std::pair<hipEvent_t, hipEvent_t>** out) {
    if ((int)evs.size() <= i) {
        hipEvent_t a, b;
        HIPC(hipEventCreate(&a));
        HIPC(hipEventCreate(&b));
        evs.emplace_back(a, b);
    }
    *out = &evs[(size_t)i];
    return MTM_OK;
}

// An ncc_mfma_kernel launch over an h x w template (or slab) and `chans` byte planes of the int8 image at `img`: the image
// and tile fields every launch shares, everything else zero
MfmaParams mfma_geometry(const uint8_t* img, const ImageDev& d, int chans, int h, int w, int oh, int ow, int method) {
    MfmaParams p{};
    p.img = img;
    p.pitch = d.u8_pitch;
    p.plane = d.u8_plane;
    p.chans = chans;
    p.h = h;
    p.w = w;
    p.oh = oh;
    p.ow = ow;
    p.nb = (w + 63) / 64;
    p.nseg = (ow + kMfSeg - 1) / kMfSeg;
    p.method = method;
    p.lds_pitch = mfma_lds_pitch(p.nb);
    p.cpr = p.lds_pitch / 16;
    p.cpr_rstep = 256 / p.cpr;
    p.cpr_dstep = 256 % p.cpr;
    p.cpr_magic = 65536 / p.cpr + 1;
    p.only_li = -1;
    return p;
}

// image rows of a plain (one output row per wave) tile
int plain_tile_rows(int h) { return std::min(h, kMfChunkH) + kMfRows - 1; }

// LDS layout of an ncc_mfma_kernel work-group: the image tile of `tile_rows` rows (aliased by the epilogue's buffers,
// `epi_bytes` per wave), the per-template constants, the work-group scratch words.  Returns the bytes up to st_off, where
// the statistics prefetch region starts.
size_t mfma_lds_layout(MfmaParams& p, int tile_rows, size_t epi_bytes) {
    const size_t lds_main = (std::max<size_t>((size_t)tile_rows * p.lds_pitch, (size_t)kMfRows * epi_bytes) + 15) & ~(size_t)15;
    p.tc_off = (int)lds_main;
    p.st_off = (int)((lds_main + sizeof(MfTemplConst) * 32 + kMfItemBytes + 15) & ~(size_t)15);
    return (size_t)p.st_off;
}

// row-multiplexed tiling, nt templates x R output rows per MFMA group: its fields and work grid.  Returns the tile rows.
int mfma_row_mux(MfmaParams& p, int R, int nt) {
    p.rm_R = R;
    p.rm_nt = nt;
    while ((1 << p.rm_log2nt) < nt) ++p.rm_log2nt;
    p.rm_steps = p.h + 2 * R - 1;
    p.nyb = (p.oh + 8 * R - 1) / (8 * R);
    p.ntg = 1;
    return rm_tile_rows(p.h, R);
}

// the candidate list (mtm_ctx::cands: a 16-byte header, then the records) a score kernel appends to, `cap` records long
template <class P>
void wire_candidates(P& p, const mtm_ctx* c, const CallRoute& R, unsigned long long cap) {
    p.cand_on = R.cand_on ? 1 : 0;
    p.hits_only = (p.cand_on && R.hits_only) ? 1 : 0;
    p.cand_min = R.cand_min ? 1 : 0;
    p.cand_thr = R.cand_thr;
    p.cand_cap = cap;
    p.cand_counter = c->cands.as<unsigned long long>();
    p.cand_hits = reinterpret_cast<mtm_hit*>(c->cands.as<uint8_t>() + 16);
}

// ... of an ncc_mfma_kernel launch: with the hits-only screen's thresholds and the head of the list also into the host's
// landing buffer
void wire_mfma_candidates(MfmaParams& p, const mtm_ctx* c, const CallRoute& R, unsigned long long cap) {
    wire_candidates(p, c, R, cap);
    p.cand_thr_lo = (double)R.cand_thr - 1e-6 * std::max(1.0, std::fabs((double)R.cand_thr));
    p.screen_hi = std::min(p.cand_thr_lo, 0.999999) - 1e-6;
    p.sq_floor = 0.99 / std::sqrt((double)p.w * (double)p.h);
    p.screen_l1 = c->screen_l1;
    if (R.cand_pin && p.cand_on && c->pinned) {
        p.cand_pin = reinterpret_cast<mtm_hit*>(static_cast<uint8_t*>(c->pinned) + 16);
        p.cand_pin_n = (unsigned long long)R.cand_pin_n;
    }
}

// The fused global extremum (keys instead of maps or candidates: 4 waves x 32 in LDS) or else, with a candidate list, the
// wave-private candidate staging buffers (see emit_at), behind the first `lds` bytes.  Returns the work-group's LDS bytes.
size_t mfma_ext_or_staging(MfmaParams& p, const mtm_ctx* c, bool ext, size_t lds) {
    if (ext) {
        p.ext_off = (int)lds;
        lds += (size_t)kMfRows * 32 * sizeof(unsigned long long);
        p.ext_best = c->counters.as<unsigned long long>();
        p.cand_on = 1;
        p.hits_only = 1;
    } else if (p.cand_on) {
        lds = (lds + 15) & ~(size_t)15;
        p.cs_off = (int)lds;
        lds += (size_t)kMfRows * kMfCandStageBytes;
    }
    return lds;
}

// An ncc_bf16_kernel launch over the class's templates in groups of 16 mb (`group_bytes` per group and piece) and `chans`
// float32 planes of the image: geometry and work grid, everything else zero
Bf16Params bf16_geometry(const mtm_ctx* c, const SizeClass& sc, int chans, int mb, long long group_bytes, int method) {
    const ImageDev d = image_dev(c);
    const int n = (int)sc.members.size();
    Bf16Params p{};
    p.img = d.f32;
    p.pitch = d.f32_pitch;
    p.plane = d.f32_plane;
    p.chans = chans;
    p.rows = c->rows;
    p.cols = c->cols;
    p.h = sc.h;
    p.w = sc.w;
    p.oh = c->rows - sc.h + 1;
    p.ow = c->cols - sc.w + 1;
    p.nkb = bf16_nkb(sc.w);
    p.chunk_h = p.nkb <= 2 ? 64 : 32;
    p.lds_cols = kBfSeg + 32 * p.nkb;
    p.n_list = n;
    p.nseg = (p.ow + kBfSeg - 1) / kBfSeg;
    p.nyb = (p.oh + kBfRows - 1) / kBfRows;
    p.ntg = (n + 16 * mb - 1) / (16 * mb);
    p.method = method;
    p.group_bytes = group_bytes;
    p.piece_bytes = group_bytes * mfma_groups_alloc(n);
    p.only_li = -1;
    p.n_work = p.nseg * p.nyb * p.ntg;
    return p;
}

// A launch of dot4 kernel variant `v` over n_list templates h x w and `chans` planes of the uint8 image
DotParams dot_params(const mtm_ctx* c, const DotVariant& v, int chans, int h, int w, int n_list) {
    const ImageDev d = image_dev(c);
    DotParams p{};
    p.img = d.u8;
    p.pitch = d.u8_pitch;
    p.plane = d.u8_plane;
    p.chans = chans;
    p.h = h;
    p.w = w;
    p.oh = c->rows - h + 1;
    p.ow = c->cols - w + 1;
    const int w4 = (w + 3) & ~3;
    p.ncy = (h + kDotChunk - 1) / kDotChunk;
    p.ncx = (w4 + kDotChunk - 1) / kDotChunk;
    p.n_list = n_list;
    p.ntx = (p.ow + 32 * v.px - 1) / (32 * v.px);
    p.nty = (p.oh + 8 * v.py - 1) / (8 * v.py);
    p.nchunks = (n_list + v.nt - 1) / v.nt;
    p.n_work = p.ntx * p.nty * p.nchunks;
    p.method = c->method;
    return p;
}

}  // namespace

namespace mtmi {

bool dot_variant_ok(int64_t v) { return v >= 0 && v < kNumDotVariants && !kDotVariants[v].wide; }

// The tail screen's split for a launch of class `sc` on route R (MfmaParams::tail_split), 0 = off: hits-only candidate lists of
// a two-row uint8 class in one K chunk, TM_CCOEFF_NORMED / TM_CCORR_NORMED, a non-negative threshold, neither the fused
// extremum nor maps in memory - and a threshold the bound can get below early enough to pay.
// The split itself follows the call's threshold (tail_split_rule, mtm_host.cpp), or is the forced one (MTM_TAIL_SPLIT).
// The rule's value is computed once per call and kept in the route: every statistics and score launch of every band of the
// call carries the same split (the route's other fields can change between a call's passes - they are tested every time).
int tail_split_for(const mtm_ctx* c, CallRoute& R, const SizeClass& sc) {
    if (!c->tail_screen || !c->screen_l1 || !sc.tail_ok || sc.r2 != 2 || sc.masked || sc.kernel != MTM_KERNEL_MFMA) return 0;
    if (!R.cand_on || !R.hits_only || R.ext || R.sparse || R.cand_min || c->chans != 1 || c->dtype != MTM_U8) return 0;
    if (c->method != MTM_TM_CCOEFF_NORMED && c->method != MTM_TM_CCORR_NORMED) return 0;
    if (sc.h + 1 > kMfChunkR2 || sc.w > 64) return 0;
    const double thr_lo = (double)R.cand_thr - 1e-6 * std::max(1.0, std::fabs((double)R.cand_thr));
    if (!(thr_lo >= 0.0)) return 0;
    if (c->tail_split_force > 0) return std::max(6, std::min(c->tail_split_force, sc.h - 2));
    if (R.tail_h != sc.h || R.tail_w != sc.w || R.tail_thr != R.cand_thr) {
        R.tail_s = tail_split_rule(sc.h, sc.w, thr_lo);
        R.tail_h = sc.h;
        R.tail_w = sc.w;
        R.tail_thr = R.cand_thr;
    }
    return R.tail_s;
}

// The templates' tail constants (TemplDev::tail_*) hold for ONE split: a launch whose split is not the one they were last
// computed for (mtm_ctx::tail_valid) re-derives them first - tail_consts_kernel, 64 threads per template, on the score
// stream: ahead of the call's first score launch (launch_stats asks before the launch waits for its band, so the kernel
// runs under band 0's copy) and behind the previous call's, never on the copy-side stream.
int ensure_tail_consts(mtm_ctx* c, const SizeClass& sc, int split) {
    if (split <= 0 || sc.members.empty()) return MTM_OK;
    const int k = class_index(c, sc);
    const bool kept = k >= 0 && (size_t)k < c->tail_valid.size();
    if (kept && c->tail_valid[(size_t)k] == split) return MTM_OK;
    MTMC(launch_tail_consts(c, sc, split, c->stream));
    if (kept) c->tail_valid[(size_t)k] = split;
    return MTM_OK;
}

// The byte planes of I^2 (masked classes: sum I^2 M on the matrix cores), once per image; a no-op for everything but
// single-channel uint8 images with a masked class on the MFMA kernel.
int ensure_square_planes(mtm_ctx* c) {
    if (c->sq_valid || c->dtype != MTM_U8 || c->chans != 1) return MTM_OK;
    bool any = false;
    for (const SizeClass& sc : c->classes)
        any = any || (sc.masked && sc.mask_rm_off >= 0 && sc.kernel == MTM_KERNEL_MFMA);
    if (!any) return MTM_OK;
    const ImageDev img = image_dev(c);
    const size_t plane_bytes = (size_t)img.u8_plane;
    MTMC(c->sq_planes.ensure(2 * plane_bytes));
    const size_t n16 = plane_bytes / 16;
    hipLaunchKernelGGL(square_planes_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream, img.u8, n16,
                       c->sq_planes.as<uint8_t>(), c->sq_planes.as<uint8_t>() + plane_bytes);
    HIPC(hipGetLastError());
    c->sq_valid = true;
    return MTM_OK;
}

// sum I^2 * M over every window of a masked uint8 class on the MFMA kernel, into `sum2`, the sum2 plane of `st` (it
// overwrites the unmasked window sum of squares, which the masked path never uses).  `fused_stats`: launch_stats ran the
// fused kernel.  The last step of launch_stats (mtm_stats.hip), on c->stream behind the statistics launch.
int launch_masked_sumsq(mtm_ctx* c, const SizeClass& sc, bool fused_stats, const StatPlanes& st, double* sum2) {
    const int h = sc.h, w = sc.w, oh = c->rows - h + 1, ow = c->cols - w + 1;
    const ImageDev img = image_dev(c);
    if (sc.mask_rm_off >= 0 && fused_stats) {
        // on the matrix cores (see square_planes_kernel): two row-multiplexed raw correlations of the byte planes of I^2
        // with the mask, combined into the sum2 plane
        const size_t plane_bytes = (size_t)img.u8_plane;
        MTMC(ensure_square_planes(c));
        const int map_pitch = (int)round_up((size_t)ow, 4);
        const long long raw_map = (long long)oh * map_pitch;
        // (one launch only while its int32 accumulator holds 256 a_h + a_l: kMasksqFusedMaxOnes)
        const bool fused_sq = c->masksq_fused != 0 && sc.mask_ones <= (double)kMasksqFusedMaxOnes;
        if (!fused_sq) MTMC(c->raw16.ensure(sizeof(int) * (size_t)(2 * raw_map)));
        MfmaParams p = mfma_geometry(nullptr, img, 1, h, w, oh, ow, c->method);
        const size_t lds = mfma_lds_layout(p, mfma_row_mux(p, 16, 1), kMfEpiBytesPerWave);
        p.n_list = 1;
        p.n_work = p.nseg * p.nyb;
        p.group_bytes = -(long long)16 * p.nb * 1024;
        p.raw_map = raw_map;
        p.raw_pitch = map_pitch;
        const uint8_t* ap = c->apacks.as<uint8_t>() + sc.mask_rm_off + (long long)16 * p.nb * 1024;
        const double km257 = 257.0 * 128.0 * sc.mask_ones;      // the mask operand is not biased
        // the pass is part of the masked class's score work: its own event pair (bench.py: roofline.masked_stat)
        std::pair<hipEvent_t, hipEvent_t>* sqe;
        MTMC(event_pair(c->sq_ev, c->timing.sq_launches, &sqe));
        HIPC(hipEventRecord(sqe->first, c->stream));
        if (fused_sq) {
            // ONE launch: the byte planes of I^2 are its two channels, the epilogue writes sum2 and the block minima
            // (the kernel's output planes travel in the plane table)
            p.chans = 2;
            p.img = c->sq_planes.as<uint8_t>();
            p.plane = (long long)plane_bytes;
            p.sq_fused = 1;
            p.sq_k = km257;
            hipLaunchKernelGGL(mfma_raw_fn(true, false), work_grid(p.n_work), dim3(256), lds, c->stream, p,
                               c->td.as<TemplDev>(), c->tlist.as<int>(), ap, st, c->maps.as<float>());
        } else {
            for (int x = 0; x < 2; ++x) {
                p.img = c->sq_planes.as<uint8_t>() + (size_t)x * plane_bytes;
                p.raw_out = c->raw16.as<int>() + (size_t)x * raw_map;
                hipLaunchKernelGGL(mfma_raw_fn(true, false), work_grid(p.n_work), dim3(256), lds, c->stream, p,
                                   c->td.as<TemplDev>(), c->tlist.as<int>(), ap, st, c->maps.as<float>());
            }
            hipLaunchKernelGGL(masksq_combine_kernel, dim3((ow + 255) / 256, oh), dim3(256), 0, c->stream, c->raw16.as<int>(),
                               c->raw16.as<int>() + raw_map, map_pitch, sum2, st.pitch, km257, oh, ow,
                               const_cast<double*>(st.blk), st.blk_pitch);
        }
        HIPC(hipGetLastError());
        HIPC(hipEventRecord(sqe->second, c->stream));
        c->timing.sq_launches++;
        return MTM_OK;
    }
    // otherwise the dot4 kernel with the mask bytes as the "template"
    if (sc.mask_pack_off < 0) {
        set_error("internal: masked class without a dot4 mask pack");
        return MTM_E_STATE;
    }
    const DotVariant v = {4, 4, 1, false, ncc_dot4_kernel<4, 4, 1, false, true>};
    DotParams p = dot_params(c, v, 1, h, w, 1);
    p.sumsq_out = sum2;
    // the kernel addresses its single template through td[tlist[0]].pack_off: point a scratch
    // TemplDev at the class's mask pack (only pack_off is read on the MASKSQ path)
    TemplDev mk = c->td_host[sc.members[0]];
    mk.pack_off = sc.mask_pack_off;
    MTMC(c->mask_td.ensure(sizeof(TemplDev) + sizeof(int)));
    HIPC(hipMemcpyAsync(c->mask_td.p, &mk, sizeof(TemplDev), hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemsetAsync(c->mask_td.as<uint8_t>() + sizeof(TemplDev), 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(v.fn, work_grid(p.n_work), dim3(256), 0, c->stream, p, c->mask_td.as<TemplDev>(),
                       reinterpret_cast<const int*>(c->mask_td.as<uint8_t>() + sizeof(TemplDev)),
                       c->packs.as<uint8_t>(), st, c->maps.as<float>());
    HIPC(hipGetLastError());
    return MTM_OK;
}

// Masked float32 class on the bf16 matrix cores (mtm_maskf32.hip.h), in the stages launch_masked_bf16 and the test-support
// entry mtm_debug_maskf32_screen both run: mbf_prepare (J = I^2, the window sums of I and J, the buffers and the raw
// launches' geometry), mbf_raw (two raw launches of ncc_bf16_kernel - I x U = T M^2, J x V = M^2 - into scratch maps, with
// `np` piece products), mbf_list (placeholders + the list of outputs that could pass; the count comes back to the host),
// mbf_rescore (exact re-scoring of the list into the score maps).
struct MaskBf16Plan {
    int h, w, oh, ow, n_all, mb, st_pitch;
    double* s1i;                // window sums (float64) of I, I^2, J, J^2
    double* s2i;
    double* s1j;
    double* s2j;
    Bf16Params p;               // the raw launches' geometry (img and mu_out per launch)
    size_t n_tiles, lds;
    const int* tl_k;
    unsigned long long cap;     // records the list holds
};

static int mbf_prepare(mtm_ctx* c, const SizeClass& sc, MaskBf16Plan* out) {
    MaskBf16Plan P{};
    const int h = sc.h, w = sc.w, oh = c->rows - h + 1, ow = c->cols - w + 1, n_all = (int)sc.members.size();
    P.h = h, P.w = w, P.oh = oh, P.ow = ow, P.n_all = n_all;
    const ImageDev img = image_dev(c);
    const size_t plane_floats = (size_t)img.f32_plane;
    MTMC(c->f32_sq.ensure(sizeof(float) * plane_floats));
    if (!c->f32_sq_valid) {
        hipLaunchKernelGGL(square_f32_kernel, dim3((unsigned)((plane_floats / 4 + 255) / 256)), dim3(256), 0, c->stream, img.f32,
                           c->f32_sq.as<float>(), plane_floats / 4);
        c->f32_sq_valid = true;
    }
    // window sums (float64): S1, S2 of I and of J - the two-pass kernels of the float32 statistics, on both planes
    const int st_pitch = (int)round_up((size_t)ow, 4);
    const size_t st_plane = (size_t)st_pitch * oh;
    MTMC(c->mbf_stats.ensure(sizeof(double) * 4 * st_plane));
    P.st_pitch = st_pitch;
    P.s1i = c->mbf_stats.as<double>();
    P.s2i = P.s1i + st_plane;
    P.s1j = P.s2i + st_plane;
    P.s2j = P.s1j + st_plane;
    {
        const int hs_pitch = (int)round_up((size_t)ow, 4);
        const size_t hs_plane = (size_t)hs_pitch * c->rows;
        MTMC(c->hs1.ensure(sizeof(double) * hs_plane));
        MTMC(c->hs2.ensure(sizeof(double) * hs_plane));
        const StatGeom g = stat_geom(c->rows, c->cols, 1, h, w);
        const StatScratch hs{c->hs1.p, c->hs2.p, hs_pitch, (long long)hs_plane};
        for (int pl = 0; pl < 2; ++pl) {
            const float* src = pl == 0 ? img.f32 : c->f32_sq.as<float>();
            StatOut o{};                    // sums only: num_type 0, no sqrt plane
            o.want_t = 1, o.t[0] = pl == 0 ? P.s1i : P.s1j, o.sum2 = pl == 0 ? P.s2i : P.s2j, o.st_pitch = st_pitch;
            MTMC(launch_stats_f64_lds(c->stream, src, img.f32_pitch, img.f32_plane, g, hs, o, 0, c->rows, 0, oh));
        }
    }
    // the two raw launches' buffers and geometry
    MTMC(c->mbf_maps.ensure(sizeof(float) * 2 * std::max<size_t>(4, c->maps_floats)));
    P.mb = n_all > 16 ? 2 : 1;
    P.p = bf16_geometry(c, sc, 1, P.mb, sc.mbf_group_bytes, MTM_TM_CCORR);      // raw sums: acc + centre * S1
    P.n_tiles = (size_t)P.p.nseg * P.p.nyb;
    MTMC(c->mbf_mu.ensure(sizeof(float) * 2 * P.n_tiles));
    P.lds = bf16_lds_bytes(P.p.chunk_h, P.p.lds_cols);
    P.tl_k = c->tlist.as<int>() + sc.tlist_off;
    P.cap = (unsigned long long)std::min<int64_t>(std::max<int64_t>(c->hit_cap, 1 << 18), kCandListMax);
    if (c->mbf_cap_debug > 0) P.cap = std::min<unsigned long long>(P.cap, (unsigned long long)c->mbf_cap_debug);  // (test support)
    MTMC(c->mbf_list.ensure(16 + sizeof(mtm_hit) * (size_t)P.cap));
    *out = P;
    return MTM_OK;
}

static int mbf_raw(mtm_ctx* c, const SizeClass& sc, const MaskBf16Plan& P, int np) {
    const ImageDev img = image_dev(c);
    Bf16Params p = P.p;
    StatPlanes st{};
    st.pitch = P.st_pitch;
    for (int pl = 0; pl < 2; ++pl) {
        p.img = pl == 0 ? img.f32 : c->f32_sq.as<float>();
        p.mu_out = c->mbf_mu.as<float>() + (size_t)pl * P.n_tiles;
        st.t[0] = pl == 0 ? P.s1i : P.s1j;
        st.sum2 = pl == 0 ? P.s2i : P.s2j;
        st.sq = st.sum2;                                        // (not read by a raw-sum launch)
        const uint8_t* ap = c->apacks.as<uint8_t>() + (pl == 0 ? sc.mbf_off_u : sc.mbf_off_v);
        const TemplDev* tdp = (pl == 0 ? c->td_u : c->td_v).as<TemplDev>();
        hipLaunchKernelGGL(bf16_kernel(P.mb, np), work_grid(p.n_work), dim3(256), P.lds, c->stream, p, tdp, P.tl_k, ap, st,
                           c->mbf_maps.as<float>());
    }
    return MTM_OK;
}

// what the listing kernels (and the test-support dump of the bounds) read: the launches' maps and constants, the statistics,
// the eps of the launch that ran (`np`)
static MaskF32Params mbf_params(mtm_ctx* c, const MaskBf16Plan& P, int np, float thr, float* maps) {
    MaskF32Params q{};
    q.m1 = q.m2 = c->mbf_maps.as<float>();
    q.td = c->td.as<TemplDev>();
    q.td_u = c->td_u.as<TemplDev>();
    q.td_v = c->td_v.as<TemplDev>();
    q.tlist = P.tl_k;
    q.s1i = P.s1i;
    q.s2i = P.s2i;
    q.s1j = P.s1j;
    q.s2j = P.s2j;
    q.st_pitch = P.st_pitch;
    q.mu_i = c->mbf_mu.as<float>();
    q.mu_j = c->mbf_mu.as<float>() + P.n_tiles;
    q.nseg = P.p.nseg;
    q.method = c->method;
    q.mode_min = c->method == MTM_TM_SQDIFF ? 1 : 0;
    q.thr = thr;
    q.eps = bf16_rig_eps(1, P.h, P.p.nkb, np);
    q.h = P.h;
    q.w = P.w;
    q.oh = P.oh;
    q.ow = P.ow;
    q.maps = maps;
    q.list = reinterpret_cast<mtm_hit*>(c->mbf_list.as<uint8_t>() + 16);
    q.counter = c->mbf_list.as<unsigned long long>();
    q.cap = P.cap;
    return q;
}

// combine: placeholders into the score maps, the rest listed; *count: how many the device counted (one small read-back: this
// path is milliseconds long, and an overflowing list changes the route)
static int mbf_list(mtm_ctx* c, const MaskBf16Plan& P, const MaskF32Params& q, bool global, unsigned long long* count) {
    const int oh = P.oh, ow = P.ow, n_all = P.n_all;
    HIPC(hipMemsetAsync(c->mbf_list.p, 0, 16, c->stream));
    if (global) {
        // N_object == 1: the templates' best lower bounds first (ordered-float keys behind the list's header + records), then
        // everything that reaches them
        MTMC(c->mbf_best.ensure(sizeof(unsigned int) * c->templs.size()));
        HIPC(hipMemsetAsync(c->mbf_best.p, 0, sizeof(unsigned int) * c->templs.size(), c->stream));
        hipLaunchKernelGGL(maskf32_best_kernel, dim3((ow + 255) / 256, oh), dim3(256), 0, c->stream, q, n_all, c->mbf_best.as<unsigned int>());
        hipLaunchKernelGGL(maskf32_list_best_kernel, dim3((ow + 255) / 256, oh), dim3(256), 0, c->stream, q, n_all,
                           c->mbf_best.as<unsigned int>());
    } else {
        hipLaunchKernelGGL(maskf32_combine_kernel, dim3((ow + 255) / 256, oh), dim3(256), 0, c->stream, q, n_all);
    }
    HIPC(hipGetLastError());
    *count = 0;
    HIPC(hipMemcpyAsync(count, c->mbf_list.p, sizeof(*count), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return MTM_OK;
}

static int mbf_rescore(mtm_ctx* c, const SizeClass& sc, const MaskF32Params& q, unsigned long long count) {
    if (count == 0) return MTM_OK;
    RefineParams r{};
    r.img = image_dev(c);
    r.td = c->td.as<TemplDev>();
    r.weights = c->weights.as<double>();
    r.method = c->method;
    r.cls = c->td_host[(size_t)sc.members[0]].cls;
    r.ring = 0;
    r.list = q.list;
    r.count = q.counter;
    r.cap = q.cap;
    r.maps = q.maps;
    const unsigned rgrid = (unsigned)std::min<unsigned long long>(count, 16384ull);
    hipLaunchKernelGGL(refine_rescore_masked_kernel, dim3(rgrid), dim3(64), 0, c->stream, r);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// The whole route.  *done = false: the list overflowed (a threshold that passes nearly everything) - the caller runs the
// float64 kernel.
static int launch_masked_bf16(mtm_ctx* c, CallRoute& R, const SizeClass& sc, float* maps, bool* done) {
    *done = false;
    MaskBf16Plan P;
    MTMC(mbf_prepare(c, sc, &P));
    MaskF32Params q{};
    unsigned long long count = 0;
    // Round 6: ONE piece product first (ncc_bf16_kernel<MB, 1>: bounds 2^-7 instead of 2^-15 of the norms' products - the
    // combine pass states them with the eps of the launch that ran); a list that overflows repeats the screen with three
    for (int np = R.bf16_np == 1 ? 1 : 3;; np = 3) {
        MTMC(mbf_raw(c, sc, P, np));
        c->timing.f32_pieces = np;
        q = mbf_params(c, P, np, R.mbf_thr, maps);
        MTMC(mbf_list(c, P, q, R.mbf_global, &count));
        if (count <= P.cap) {
            if (np == 1) c->np1_backoff_len = 16;
            break;
        }
        if (np == 3) return MTM_OK;                                 // *done stays false: float64 kernel
        R.bf16_np = 3;                                              // (this call's other classes and the next calls start with three)
        c->np1_backoff = c->np1_backoff_len;
        c->np1_backoff_len = std::min(2 * c->np1_backoff_len, 1024);
    }
    MTMC(mbf_rescore(c, sc, q, count));
    R.mbf_used = true;
    *done = true;
    return MTM_OK;
}

// naive kernel (float64 accumulation straight from the image: MTM_KERNEL_NAIVE)
static int launch_naive(mtm_ctx* c, const SizeClass& sc, const int* tl, int n_list, const StatPlanes& st) {
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    MTMC(ensure_f32_plane(c));
    hipLaunchKernelGGL(ncc_naive_kernel, dim3((ow + 63) / 64, (oh + 3) / 4, n_list), dim3(64, 4), 0, c->stream, image_dev(c),
                       c->td.as<TemplDev>(), tl, c->weights.as<double>(), st, c->method, sc.masked ? 1 : 0, c->maps.as<float>());
    c->timing.kernel_used = MTM_KERNEL_NAIVE;
    return MTM_OK;
}

// Large templates on the MFMA kernel: one RAW launch per slab (a template of its own against the image shifted by the
// slab's offset), then slab_combine_kernel adds the slabs up, restores the bias terms and normalises.  *ev_own: the
// timing pair `ev` went to the side stream of a merged launch (on the score stream it would bracket the fork and the
// join, not the launch).
static int launch_mfma_slabs(mtm_ctx* c, CallRoute& R, const SizeClass& sc, const StatPlanes& st, int only_li,
                             const std::pair<hipEvent_t, hipEvent_t>& ev, bool* ev_own) {
    const int h = sc.h, w = sc.w, oh = c->rows - h + 1, ow = c->cols - w + 1;
    const ImageDev img = image_dev(c);
    const TemplDev* td = c->td.as<TemplDev>();
    float* maps = c->maps.as<float>();
    const hipStream_t ncc_s = c->stream;
    const int n_all = (int)sc.members.size();
    const int map_pitch = (int)round_up((size_t)ow, 4);
    const long long raw_map = (long long)oh * map_pitch;
    const int S = (int)sc.slabs.size();
    MTMC(c->slab_raw.ensure(sizeof(int) * (size_t)S * n_all * (size_t)raw_map));
    const bool rmr = sc.slab_R > 0;
    // The slabs' launches are independent.  One of them is (output rows / 8R) x (columns / 256) work items - 91 for the
    // reference's own benchmark shape (2048^2 image, one 414 x 400 template: four slabs), against 512 resident
    // work-group slots: launches that do not fill the chip twice over run side by side on up to slab_concurrency
    // streams, forked from and joined into the score stream.
    int n_side = 1;
    {
        const int rows_per_item = rmr ? 8 * sc.slab_R : kMfRows;
        const long long items = (long long)((ow + kMfSeg - 1) / kMfSeg) * ((oh + rows_per_item - 1) / rows_per_item) *
                                (rmr ? 1 : (n_all + 31) / 32);
        const int cus = c->n_cus > 0 ? c->n_cus : 256;
        if (items < 4LL * cus) n_side = (int)std::min<long long>(std::min(S, kSlabStreams), (4LL * cus + items - 1) / items);
    }
    // MTM_SLAB_MERGE (default 1): slabs of equal height and block count go out as ONE launch (MfmaParams::n_slab) - the
    // hardware fills the chip from one grid and back-fills as work-groups finish, where several launches on several
    // streams share four hardware queues (the fourth of four side-by-side slab launches started when the first had
    // ended: profiles/r04_r04v_slab) - on one side stream, so that the statistics pass still runs under it.
    bool merged = rmr && S > 1;
    for (int k = 1; k < S && merged; ++k) {
        const SizeClass::Slab &a = sc.slabs[0], &b = sc.slabs[(size_t)k];
        merged = (b.r1 - b.r0) == (a.r1 - a.r0) && (b.c1 - b.c0 + 63) / 64 == (a.c1 - a.c0 + 63) / 64 &&
                 b.apack_off - a.apack_off == (long long)k * rm_pack_bytes(a.r1 - a.r0, a.c1 - a.c0, sc.slab_R);
    }
    if (merged) n_side = c->slab_fork_early ? 2 : 1;        // (2: "side streams in use"; only the first one is)
    if (n_side > 1) {
        while ((int)c->slab_streams.size() < n_side) {
            hipStream_t s2;
            hipEvent_t e2;
            HIPC(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            HIPC(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
            c->slab_streams.push_back(s2);
            c->slab_done.push_back(e2);
        }
        if (!c->slab_fork) HIPC(hipEventCreateWithFlags(&c->slab_fork, hipEventDisableTiming));
        if (!c->slab_fork_early) HIPC(hipEventRecord(c->slab_fork, ncc_s));      // (else: recorded ahead of the statistics)
        for (int i = 0; i < n_side; ++i) HIPC(hipStreamWaitEvent(c->slab_streams[(size_t)i], c->slab_fork, 0));
    }
    for (int k = 0; k < (merged ? 1 : S); ++k) {
        const SizeClass::Slab& sl = sc.slabs[(size_t)k];
        const int hs = sl.r1 - sl.r0, ws = sl.c1 - sl.c0;
        hipStream_t slab_s = n_side > 1 ? c->slab_streams[(size_t)(merged ? 0 : k % n_side)] : ncc_s;
        MfmaParams p = mfma_geometry(c->slot[c->cur].u8b.as<uint8_t>() + (size_t)sl.ch * img.u8_plane + (size_t)sl.r0 * img.u8_pitch + sl.c0,
                                     img, 1, hs, ws, oh, ow, c->method);
        p.n_list = n_all;
        p.raw_map = raw_map;
        p.raw_pitch = map_pitch;
        p.raw_out = c->slab_raw.as<int>() + (size_t)k * n_all * (size_t)raw_map;
        int tile_rows;
        if (rmr) {
            tile_rows = mfma_row_mux(p, sc.slab_R, sc.slab_nt);
            p.rm_cstride = rm_pack_bytes(hs, ws, sc.slab_R);
            p.group_bytes = -(long long)sc.slab_R * p.nb * 1024;
        } else {
            p.nyb = (oh + kMfRows - 1) / kMfRows;
            p.ntg = (n_all + 31) / 32;
            p.group_bytes = mfma_group_bytes(hs, ws, 1);
            tile_rows = plain_tile_rows(hs);
        }
        p.n_work = p.nseg * p.nyb * p.ntg;
        if (merged) {                       // every slab of the class: slab 0's geometry (the widest), S times the items
            int ncb = 0;
            for (const auto& q : sc.slabs) ncb += (q.ch == sl.ch && q.r0 == sl.r0) ? 1 : 0;
            p.n_slab = S;
            p.slab_ncb = ncb;
            p.slab_nrb = S / (ncb * c->chans);
            p.slab_cw = ncb > 1 ? sc.slabs[1].c0 - sl.c0 : 0;
            p.slab_rh = hs;
            p.slab_ap_step = rm_pack_bytes(hs, ws, sc.slab_R);
            p.slab_raw_step = (long long)n_all * raw_map;
            p.n_work *= S;
        }
        // statistics prefetch region: none for the row-multiplexed launches (differs by tiling; this code does not decide whether it should)
        const size_t lds = mfma_lds_layout(p, tile_rows, kMfEpiBytesPerWave) + (rmr ? 0 : (size_t)kMfRows * kMfStatBytesPerWave);
        const uint8_t* ap = c->apacks.as<uint8_t>() + sl.apack_off + (rmr ? (long long)sc.slab_R * p.nb * 1024 : 0);
        if (merged && slab_s != ncc_s) HIPC(hipEventRecord(ev.first, slab_s));
        hipLaunchKernelGGL(mfma_raw_fn(rmr, false), work_grid(p.n_work), dim3(256), lds, slab_s, p, td,
                           c->tlist.as<int>() + sc.tlist_off, ap, st, maps);
        if (merged && slab_s != ncc_s) {
            HIPC(hipEventRecord(ev.second, slab_s));
            *ev_own = true;
        }
    }
    for (int i = 0; i < (merged ? 1 : n_side) && n_side > 1; ++i) {
        HIPC(hipEventRecord(c->slab_done[(size_t)i], c->slab_streams[(size_t)i]));
        HIPC(hipStreamWaitEvent(ncc_s, c->slab_done[(size_t)i], 0));
    }
    SlabParams q{};
    q.raw = c->slab_raw.as<int>();
    q.raw_slab = (long long)n_all * raw_map;
    q.raw_map = raw_map;
    q.n_slabs = S;
    q.oh = oh;
    q.ow = ow;
    q.pitch = map_pitch;
    q.n_list = n_all;
    q.method = c->method;
    q.w = w;
    q.h = h;
    q.chans = c->chans;
    wire_candidates(q, c, R, cand_list_cap(c));     // (cand_cap differs from the plain int8 launch; not decided here)
    if (R.ext) {                                  // fused global extremum: keys instead of maps / candidates
        q.ext_on = 1;
        q.ext_best = c->counters.as<unsigned long long>();
        q.cand_on = 0;
        q.hits_only = 1;
    }
    hipLaunchKernelGGL(slab_combine_kernel, dim3((ow + 255) / 256, oh, n_all), dim3(256), 0, c->stream, q, td,
                       c->tlist.as<int>() + sc.tlist_off, st, maps, only_li);
    c->timing.kernel_used = MTM_KERNEL_MFMA;
    return MTM_OK;
}

// uint8 classes on the MFMA kernel: plain, two-row (r2) or row-multiplexed tiling.  The kernel works on whole 16-template
// groups of the class list; a single-template request (mtm_score_map) computes its group and stores only that template.
static int launch_mfma(mtm_ctx* c, CallRoute& R, const SizeClass& sc, const StatPlanes& st, int only_li, int yb0, int yb1) {
    const int h = sc.h, w = sc.w, oh = c->rows - h + 1, ow = c->cols - w + 1;
    const int n_all = (int)sc.members.size();
    const bool rm = sc.rm_R > 0;
    const bool r2 = sc.r2 > 0;
    const int mb = r2 ? sc.r2 : (n_all > 16 || rm) ? 2 : 1;
    const int tgsz = r2 ? 16 : 16 * mb;          // templates per work item
    // (the int8 view: bytes ^ 0x80, same geometry as img.u8)
    MfmaParams p = mfma_geometry(c->slot[c->cur].u8b.as<uint8_t>(), image_dev(c), c->chans, h, w, oh, ow, c->method);
    p.nyb = r2 ? (oh + mb * kMfRows - 1) / (mb * kMfRows) : (oh + kMfRows - 1) / kMfRows;
    p.ntg = (n_all + tgsz - 1) / tgsz;
    p.group_bytes = sc.group_bytes;
    // (cand_cap is the whole hit_cap here, min(hit_cap, kCandListMax) on the other launches: differs; not decided here)
    wire_mfma_candidates(p, c, R, (unsigned long long)c->hit_cap);
    // the 8 spare bytes of the candidate header - or of the host's landing buffer - carry the shader clock the kernel
    // measured (fetched with it).  (Only this launch sets clk_out: differs; not decided here.)
    if (p.cand_pin)
        p.clk_out = reinterpret_cast<float*>(static_cast<uint8_t*>(c->pinned) + 8);
    else if (p.cand_on && c->cands.p)
        p.clk_out = reinterpret_cast<float*>(c->cands.as<uint8_t>() + 8);
    if (R.sparse) {                         // maps in memory + a flag per row segment that holds something above the threshold
        p.seg_flags = c->seg_flags.as<uint8_t>();
        p.flag_tstride = R.flag_tstride;
        p.flag_rstride = R.flag_rstride;
        const bool normed_m = c->method == MTM_TM_SQDIFF_NORMED || c->method == MTM_TM_CCORR_NORMED || c->method == MTM_TM_CCOEFF_NORMED;
        p.seg_skip = (c->seg_skip && !sc.masked && normed_m) ? 1 : 0;
        R.seg_skip_used = R.seg_skip_used || p.seg_skip != 0;
    }
    int tg0 = 0;
    if (only_li >= 0 && !rm) {   // one template: just its group
        tg0 = only_li / tgsz;
        p.ntg = 1;
    }
    int tile_rows = r2 ? std::min(h + mb - 1, kMfChunkR2) + (kMfRows - 1) * mb : plain_tile_rows(h);
    if (rm) {
        tile_rows = mfma_row_mux(p, sc.rm_R, sc.rm_nt);
        p.rm_cstride = class_rm_pack_bytes(sc);
        p.rm_rsq = c->stats_rsq.as<double>();
    }
    if (yb1 >= 0) {                     // banded launch: row blocks yb0 .. yb1 - 1 (the caller keeps the range non-empty)
        p.yb0 = yb0;
        p.nyb = std::min(yb1, p.nyb) - yb0;
    }
    p.n_work = p.nseg * p.nyb * p.ntg;
    // statistics prefetch region: (channels + 2) planes per wave; none for the row-multiplexed tiling (it loads its
    // statistics directly), (mb + 1) / 2 KB per wave for the two-row one (differs by tiling; not decided here)
    // (tail screen: the tail boxes' records and the templates' tail constants behind them)
    p.tail_split = (r2 && st.blkq != nullptr && only_li < 0 && !p.seg_skip) ? tail_split_for(c, R, sc) : 0;
    MTMC(ensure_tail_consts(c, sc, p.tail_split));          // (launch_stats has seen to it: a no-op)
    if (const int k = class_index(c, sc); k >= 0 && (size_t)k < c->tail_last.size())
        c->tail_last[(size_t)k] = p.tail_split;                // (what mtm_debug_class_tilings reports)
    const size_t stat_bytes = rm ? 0 : r2 ? (size_t)kMfRows * ((mb + 1) / 2) * 1024 + (p.tail_split ? mf_tail_lds_bytes() : 0)
                                          : (size_t)kMfRows * mf_stat_bytes_per_wave(c->chans == 3 ? 3 : 1);
    const bool ext = R.ext;                          // plan_call checked the class
    const size_t lds = mfma_ext_or_staging(p, c, ext, mfma_lds_layout(p, tile_rows, kMfEpiBytesPerWave) + stat_bytes);
    p.kp_nseg = sc.kp_nseg;
    p.kp_blocks = sc.kp_nseg ? kp_blocks(h, sc.kp_nseg) : 0;
    const uint8_t* ap = c->apacks.as<uint8_t>() + sc.apack_off +
                        (rm ? (sc.kp_nseg ? 0LL : (long long)sc.rm_R * p.nb * 1024)
                            : (long long)tg0 * (r2 ? 1 : mb) * sc.group_bytes);
    // with a group offset the kernel's list positions must stay class-relative: shift the list
    // pointer and the counts instead (positions inside the kernel are relative to tg0)
    p.n_list = n_all - tg0 * tgsz;
    if (only_li >= 0) p.only_li = only_li - tg0 * tgsz;
    const int* tl_k = c->tlist.as<int>() + sc.tlist_off + tg0 * tgsz;
    // the instantiation of ncc_mfma_kernel for this class (the kernels live in the mtm_mfma_*.hip units)
    MfmaSel sel;
    sel.mb = mb;
    sel.masked = sc.masked;
    sel.rm = rm;
    sel.ch = (c->chans == 3 && !sc.masked) ? 3 : 1;
    sel.method = (c->chans == 1 || sel.ch == 3) ? c->method : -1;     // other channel counts: the generic epilogue
    sel.ext = ext;
    // IEEE division in the epilogue (the default since round 5: measured free on the hits-only path, profiles/r05*).  The
    // fused global extremum of MASKED classes only exists with the reciprocal normalisation (<= 1 ulp(float32) on ~1e-8
    // of the outputs); exact_div == 2 (strict) sends those calls through maps + extremum_kernel instead (fm_begin).
    // (The uint16 launch does not leave `ext && sc.masked` out: differs; not decided here.)
    sel.exact_div = c->exact_div != 0 && !(ext && sc.masked);
    sel.r2 = r2;
    sel.kp = sc.kp_nseg > 0;
    const MfmaFn fn = mfma_kernel(sel);
    if (!fn) {
        set_error("internal: no ncc_mfma_kernel instantiation for this class");
        return MTM_E_STATE;
    }
    hipLaunchKernelGGL(fn, work_grid(p.n_work), dim3(256), lds, c->stream, p, c->td.as<TemplDev>(), tl_k, ap, st,
                       c->maps.as<float>());
    c->timing.kernel_used = MTM_KERNEL_MFMA;
    return MTM_OK;
}

// uint16: ONE launch over the image's two byte planes (the "channels" of the launch) x [T_hi | T_lo] of 16 templates
// per work item; the high-byte partial sums stay in registers while the low-byte plane is walked, and the epilogue
// finishes the exact 16-bit correlation + normalisation (kMfU16, mtm_mfma.hip.h).
static int launch_mfma16(mtm_ctx* c, CallRoute& R, const SizeClass& sc, const StatPlanes& st, int only_li, int yb0, int yb1) {
    const int h = sc.h, w = sc.w, oh = c->rows - h + 1, ow = c->cols - w + 1;
    const int n_all = (int)sc.members.size(), n_pad = sc.n_pad;
    // (plane 0: high bytes, plane 1: low bytes)
    MfmaParams p = mfma_geometry(c->slot[c->cur].u8b.as<uint8_t>(), image_dev(c), 2, h, w, oh, ow, c->method);
    p.nyb = (oh + kMfRows - 1) / kMfRows;
    p.ntg = n_pad / 16;
    p.group_bytes = sc.group_bytes;
    int tg0 = 0;
    if (only_li >= 0) {                 // one template: just its group of 16
        tg0 = only_li / 16;
        p.ntg = 1;
    }
    if (yb1 >= 0) {                     // banded launch: row blocks yb0 .. yb1 - 1
        p.yb0 = yb0;
        p.nyb = std::min(yb1, p.nyb) - yb0;
    }
    p.n_work = p.nseg * p.nyb * p.ntg;
    p.kp_nseg = sc.kp_nseg;
    p.kp_blocks = sc.kp_nseg ? kp_blocks(h, sc.kp_nseg) : 0;
    p.n_list = n_all - tg0 * 16;                            // list positions inside the kernel are relative to tg0
    if (only_li >= 0) p.only_li = only_li - tg0 * 16;
    p.u16_tsum = c->tsum.as<double>() + sc.tsum_off + tg0 * 16;
    p.u16_npad = n_pad;
    p.u16_area = (double)h * (double)w;
    wire_mfma_candidates(p, c, R, cand_list_cap(c));       // (cand_cap differs from the plain int8 launch; not decided here)
    // (no statistics prefetch: the epilogue reads them from memory - differs from the int8 launch; not decided here)
    const bool ext = R.ext;                          // fused global extremum (plan_call checked the classes)
    const size_t lds = mfma_ext_or_staging(p, c, ext, mfma_lds_layout(p, plain_tile_rows(h), kMfU16EpiBytesPerWave));
    const uint8_t* ap = c->apacks.as<uint8_t>() + sc.apack_off + (long long)tg0 * 2 * sc.group_bytes;
    const int* tl_k = c->tlist.as<int>() + sc.tlist_off + tg0 * 16;
    MfmaSel sel16;
    sel16.method = kMfU16;
    sel16.kp = sc.kp_nseg > 0;
    sel16.ext = ext;
    sel16.exact_div = c->exact_div != 0;            // (differs from the int8 launch's rule; not decided here)
    hipLaunchKernelGGL(mfma_kernel(sel16), work_grid(p.n_work), dim3(256), lds, c->stream, p, c->td.as<TemplDev>(), tl_k, ap,
                       st, c->maps.as<float>());
    c->timing.kernel_used = MTM_KERNEL_MFMA16;
    return MTM_OK;
}

// float32 classes on the bf16 matrix cores (ncc_bf16_kernel: two or three bf16 piece products per tap)
static int launch_bf16(mtm_ctx* c, CallRoute& R, const SizeClass& sc, const StatPlanes& st, int only_li, int yb0, int yb1) {
    const int h = sc.h;
    const int n_all = (int)sc.members.size();
    const int mb = n_all > 16 ? 2 : 1;
    Bf16Params p = bf16_geometry(c, sc, c->chans, mb, sc.group_bytes, c->method);
    if (yb1 >= 0) {                             // a band of row blocks (run_score_banded, float32 uploads)
        p.yb0 = yb0;
        p.nyb = std::min(yb1, p.nyb) - yb0;
    }
    int tg0 = 0;
    if (only_li >= 0) {
        tg0 = only_li / (16 * mb);
        p.ntg = 1;
        p.n_list = n_all - tg0 * 16 * mb;
        p.only_li = only_li - tg0 * 16 * mb;
    }
    p.n_work = p.nseg * p.nyb * p.ntg;
    // (cand_cap min(hit_cap, kCandListMax) and no cand_pin: both differ from the int8 launch; not decided here)
    wire_candidates(p, c, R, cand_list_cap(c));
    const bool raw_m = c->method == MTM_TM_SQDIFF || c->method == MTM_TM_CCORR || c->method == MTM_TM_CCOEFF;
    // piece products of this launch: one where only a list leaves the kernel and every listing decision rests on a
    // bound that knows it (below: rig 1 / 2, the refined extremum by bounds); three everywhere else
    int np = 3;
    if (R.bf16_np == 1 && R.refine && (p.hits_only || R.ext) && (!raw_m || R.ext || R.raw_rig)) np = 1;
    if (R.refine && !raw_m) {
        // Round 5: the listing decisions of the refined routes by the rigorous per-output bound (Bf16Params::rig)
        p.rig = 1;
        p.rig_eps = bf16_rig_eps(c->chans, h, p.nkb, np);
        p.rig_thr = R.rig_thr;
        p.list_all = R.cand_min ? (R.rig_thr < -1.0f ? 1 : 0) : (R.rig_thr < 0.0f ? 1 : 0);
        if (R.refine_scan) {                // map mode: the scan's tolerances hold while no bound exceeds the cap
            p.rig_cap = R.rig_cap;
            p.rig_flag = reinterpret_cast<unsigned int*>(c->cands.as<uint8_t>() + 8);
        }
    }
    if (R.refine && raw_m && R.raw_rig && !R.ext) {
        // raw sums with a threshold (round 5): everything whose UPPER bound passes is listed and re-scored exactly
        p.rig = 2;
        p.rig_eps = bf16_rig_eps(c->chans, h, p.nkb, np);
        p.rig_thr = R.rig_thr;
        p.list_all = 0;
    }
    if (R.ext) {                                      // fused global extremum (plan_call checked the classes)
        p.ext_on = 1;
        p.ext_best = c->counters.as<unsigned long long>();
        p.cand_on = 1;
        p.hits_only = 1;
        p.ext_margin = R.refine ? kRefineThrMargin : 0.0f;
        // (the spare word of the candidate header, as rig_flag in map mode: collect_global_extremum reads it with the count)
        if (R.refine) p.nf_flag = reinterpret_cast<unsigned int*>(c->cands.as<uint8_t>() + 8);
        if (raw_m && R.refine) {
            // rigorous bounds instead of a relative margin (Bf16Params::ext_raw): 2^-15 for the dropped piece products
            // and the two 16-bit representations, 2^-24 per float32 accumulation (three MFMAs per 32-tap block)
            p.ext_raw = 1;
            p.ext_eps = bf16_ext_eps(c->chans, h, p.nkb, np);
        } else if (p.rig) {
            p.ext_raw = 1;                              // (bounds of the quality instead of scores: the rig branch of the epilogue)
            p.list_all = 0;
        }
    }
    const size_t lds = bf16_lds_bytes(p.chunk_h, p.lds_cols);
    const uint8_t* ap = c->apacks.as<uint8_t>() + sc.apack_off + (long long)tg0 * mb * sc.group_bytes;
    const int* tl_k = c->tlist.as<int>() + sc.tlist_off + tg0 * 16 * mb;
    // (a launch that is neither listing by a bound nor the bound-keeping extremum must not run the screen: its scores
    // would be taken at face value)
    if (np == 1 && !(p.rig != 0 || (p.ext_on && p.ext_raw))) np = 3;
    if (np == 1 && !p.hits_only) np = 3;
    if (c->f32_mfma == 4) np = 1;               // (diagnostic: the screen's scores as they are)
    hipLaunchKernelGGL(bf16_kernel(mb, np), work_grid(p.n_work), dim3(256), lds, c->stream, p, c->td.as<TemplDev>(), tl_k, ap,
                       st, c->maps.as<float>());
    c->timing.kernel_used = MTM_KERNEL_MFMA_F32;
    c->timing.f32_pieces = np;
    return MTM_OK;
}

// uint8 classes on the dot4 (VALU) kernel
static void launch_dot4(mtm_ctx* c, const SizeClass& sc, const int* tl, int n_list, const StatPlanes& st) {
    const bool wide = (double)c->chans * sc.w * sc.h * 65025.0 >= 4294967296.0;
    const int vi = wide ? kDotWideVariant : c->dot_variant;
    const DotVariant& v = kDotVariants[vi];
    if (const int k = class_index(c, sc); k >= 0 && (size_t)k < c->dot_last.size())
        c->dot_last[(size_t)k] = vi;                            // (what mtm_debug_class_tilings reports)
    const DotParams p = dot_params(c, v, c->chans, sc.h, sc.w, n_list);
    hipLaunchKernelGGL(v.fn, work_grid(p.n_work), dim3(256), 0, c->stream, p, c->td.as<TemplDev>(), tl, c->packs.as<uint8_t>(),
                       st, c->maps.as<float>());
    c->timing.kernel_used = MTM_KERNEL_DOT4;
}

// The float64 kernel.  A masked float32 class, local extrema against a threshold: two raw launches of the bf16 kernel as
// a screen + exact re-scoring of everything that could pass (mtm_maskf32.hip.h); the float64 kernel only if that list
// overflows.
static int launch_f64(mtm_ctx* c, CallRoute& R, const SizeClass& sc, int kernel, const int* tl, int n_list, const StatPlanes& st) {
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    const int ntx = (ow + kF64BX - 1) / kF64BX, nty = (oh + kF64BY - 1) / kF64BY;
    const dim3 grd(ntx * nty, n_list);
    const ImageDev img = image_dev(c);
    float* maps = c->maps.as<float>();
    MTMC(ensure_f32_plane(c));
    bool screened = false;
    if (sc.masked && sc.mask_bf16 && R.mbf_thr_on && n_list == (int)sc.members.size() && kernel == MTM_KERNEL_AUTO)
        MTMC(launch_masked_bf16(c, R, sc, maps, &screened));
    if (screened)
        c->timing.kernel_used = MTM_KERNEL_MFMA_F32;
    else if (sc.masked)
        hipLaunchKernelGGL(ncc_f64_kernel<true>, grd, dim3(256), 0, c->stream, img, c->td.as<TemplDev>(), tl,
                           c->weights.as<double>(), st, c->method, maps, ntx);
    else
        hipLaunchKernelGGL(ncc_f64_kernel<false>, grd, dim3(256), 0, c->stream, img, c->td.as<TemplDev>(), tl,
                           c->weights.as<double>(), st, c->method, maps, ntx);
    if (c->timing.kernel_used == 0) c->timing.kernel_used = MTM_KERNEL_AUTO;
    return MTM_OK;
}

// Score maps of `n_list` templates of class `sc` (device list at tlist + list_off), on the kernel family the class resolves to.
// `yb0`, `yb1`: range of output row blocks (MFMA and bf16 kernels; banded image upload), yb1 < 0 = all.
int launch_ncc(mtm_ctx* c, CallRoute& R, const SizeClass& sc, int list_off, int n_list, const StatPlanes& st, int only_li,
               int yb0, int yb1) {
    const int kernel = sc.kernel;
    const int* tl = c->tlist.as<int>() + list_off;
    // timing events around the dominant kernel
    // (The events are stream commands of their own.  Handing them to the launch itself - hipExtLaunchKernelGGL's start /
    // stop events - was measured in round 4: the gaps around the launches stayed, the call got 14 us SLOWER;
    // profiles/r04_r04w.)
    std::pair<hipEvent_t, hipEvent_t>* evp;
    MTMC(event_pair(c->ncc_ev, c->timing.ncc_launches, &evp));
    HIPC(hipEventRecord(evp->first, c->stream));
    bool ev_own = false;                // the slab launcher recorded the pair itself (on the stream its launch went to)
    if (kernel == MTM_KERNEL_NAIVE)
        MTMC(launch_naive(c, sc, tl, n_list, st));
    else if (kernel == MTM_KERNEL_MFMA && !sc.slabs.empty())
        MTMC(launch_mfma_slabs(c, R, sc, st, only_li, *evp, &ev_own));
    else if (kernel == MTM_KERNEL_MFMA)
        MTMC(launch_mfma(c, R, sc, st, only_li, yb0, yb1));
    else if (kernel == MTM_KERNEL_MFMA16)
        MTMC(launch_mfma16(c, R, sc, st, only_li, yb0, yb1));
    else if (kernel == MTM_KERNEL_MFMA_F32 && !R.f32_exact)
        MTMC(launch_bf16(c, R, sc, st, only_li, yb0, yb1));
    else if (kernel == MTM_KERNEL_DOT4)
        launch_dot4(c, sc, tl, n_list, st);
    else
        MTMC(launch_f64(c, R, sc, kernel, tl, n_list, st));
    HIPC(hipGetLastError());
    if (!ev_own) HIPC(hipEventRecord(evp->second, c->stream));
    c->timing.ncc_launches++;
    return MTM_OK;
}

// side lanes 1 .. n of multi-class calls (mtm_ctx::Lane): a stream + its join event each
int ensure_lanes(mtm_ctx* c, int n) {
    while ((int)c->lanes.size() < n) {
        mtm_ctx::Lane L;
        HIPC(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
        c->lanes.push_back(L);
    }
    return MTM_OK;
}

int ensure_maps(mtm_ctx* c) { return c->maps.ensure(sizeof(float) * std::max<size_t>(4, c->maps_floats)); }

// float32 refinement (mtm_refine.hip.h): the records of the candidate buffer that belong to class `sc` get the scores
// of the exact float64 kernel - `ring`: their whole 3x3 neighbourhoods, written into the maps.  Runs right behind the
// class's score launch: the statistics planes are shared by all classes and only live until the next one starts.
int launch_refine(mtm_ctx* c, const SizeClass& sc, const StatPlanes& st, bool ring, bool patch_maps) {
    MTMC(ensure_f32_plane(c));
    RefineParams p{};
    p.img = image_dev(c);
    p.td = c->td.as<TemplDev>();
    p.weights = c->weights.as<double>();
    p.st = st;
    p.method = c->method;
    p.cls = (int)(&sc - c->classes.data());
    p.ring = ring ? 1 : 0;
    p.list = reinterpret_cast<mtm_hit*>(c->cands.as<uint8_t>() + 16);
    p.count = c->cands.as<unsigned long long>();
    p.cap = cand_list_cap(c);
    p.maps = patch_maps ? c->maps.as<float>() : nullptr;
    // one wave per record, records strided over a grid that fills the chip a few times (the list length is only known
    // on the device; most calls list a few hundred records)
    const unsigned grid = (unsigned)std::min<unsigned long long>(p.cap, 8192ull);
    hipLaunchKernelGGL(refine_rescore_kernel, dim3(grid), dim3(64), 0, c->stream, p);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// refined global extremum: the keys the score kernel kept are approximate - rebuild them from the re-scored list
static int launch_refine_extremum(mtm_ctx* c, const CallRoute& R) {
    const size_t n = c->templs.size();
    HIPC(hipMemsetAsync(c->counters.p, 0, sizeof(unsigned long long) * 2 * n, c->stream));
    const unsigned long long cap = cand_list_cap(c);
    hipLaunchKernelGGL(refine_extremum_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, c->stream,
                       reinterpret_cast<const mtm_hit*>(c->cands.as<uint8_t>() + 16), c->cands.as<unsigned long long>(), cap,
                       c->td.as<TemplDev>(), R.cand_min ? 1 : 0, c->counters.as<unsigned long long>());
    HIPC(hipGetLastError());
    return MTM_OK;
}

// the map scan of the refined route: potential peaks of class `sc` (approximate maps in memory) -> candidate buffer
static int launch_refine_scan(mtm_ctx* c, const CallRoute& R, const SizeClass& sc) {
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    const dim3 grd((ow + kPkCols - 1) / kPkCols, (oh + 4 * kPkRows - 1) / (4 * kPkRows), (unsigned)sc.members.size());
    hipLaunchKernelGGL(refine_scan_kernel, grd, dim3(256), 0, c->stream, c->maps.as<float>(), c->td.as<TemplDev>(),
                       c->tlist.as<int>() + sc.tlist_off, R.cand_min ? 1 : 0, R.scan_thr,
                       2.0f * R.rig_cap, c->opt_border,
                       reinterpret_cast<mtm_hit*>(c->cands.as<uint8_t>() + 16),
                       cand_list_cap(c), c->cands.as<unsigned long long>());
    HIPC(hipGetLastError());
    return MTM_OK;
}

// what follows a bf16 class's score launch on the refined routes: the exact re-scoring of what the screen listed
static int launch_refine_class(mtm_ctx* c, const CallRoute& R, const SizeClass& sc, const StatPlanes& st) {
    if (!R.refine_scan) return launch_refine(c, sc, st, false, !R.hits_only);
    MTMC(launch_refine_scan(c, R, sc));
    return launch_refine(c, sc, st, true, true);
}

namespace {
// The context's stream and per-class scratch exchanged with a lane's for the time a class is queued (everything below
// launch_stats / launch_ncc keeps using c->stream, c->stats ...); swapped back on every path out.
struct LaneScope {
    mtm_ctx* c;
    mtm_ctx::Lane* L;
    void swap_all() {
        std::swap(c->stream, L->stream);
        std::swap(c->stats, L->stats);
        std::swap(c->stats_rsq, L->stats_rsq);
        std::swap(c->stats_blk, L->stats_blk);
        std::swap(c->hs1, L->hs1);
        std::swap(c->hs2, L->hs2);
        std::swap(c->raw16, L->raw16);
        std::swap(c->slab_raw, L->slab_raw);
        std::swap(c->stats_hi, L->stats_hi);
        std::swap(c->mask_td, L->mask_td);          // (the scratch template record of the dot4 sum I^2 M pass)
        std::swap(c->slab_streams, L->slab_streams);    // (side streams + fork / join events of a slab class)
        std::swap(c->slab_done, L->slab_done);
        std::swap(c->slab_fork, L->slab_fork);
    }
    LaneScope(mtm_ctx* c_, mtm_ctx::Lane* L_) : c(c_), L(L_) { if (L) swap_all(); }
    ~LaneScope() { if (L) swap_all(); }
    LaneScope(const LaneScope&) = delete;
    LaneScope& operator=(const LaneScope&) = delete;
};
}  // namespace

// Does anything class `sc` launches read the float32 plane of the image (the float64 / naive score kernels, the two-pass
// statistics)?  A banded uint8 upload leaves that plane out (ensure_f32_plane rebuilds it on demand).
static bool class_reads_f32(const mtm_ctx* c, const SizeClass& sc) {
    if (sc.kernel == MTM_KERNEL_NAIVE || sc.kernel == MTM_KERNEL_AUTO) return true;     // ncc_naive_kernel / ncc_f64_kernel
    // hsum_kernel on the float32 plane of a uint8 image (uint16 / float32 images are uploaded with their float32 plane)
    return stats_route(c->dtype, c->chans, sc.h, sc.w, c->cols, c->fuse_stats != 0) == kStatsRouteU8TwoPassWide;
}

// Statistics + score launches of every size class but `skip` (the class a banded call has already queued; -1: none).
// `fork`: the event the lanes start behind instead of the present end of c->stream (banded calls: the last band's event -
// the image is complete - so that the next class runs under the banded class's last launch).
static int run_score_classes(mtm_ctx* c, CallRoute& R, int skip, hipEvent_t fork) {
    if (!R.hits_only) MTMC(ensure_maps(c));
    // several size classes: alternate them over lanes (see mtm_ctx::Lane).  Not while the float32 refinement is on: its
    // re-scoring kernels walk the candidate list of the class that just ran.
    int n_lanes = 1;
    const size_t n_todo = c->classes.size() - (skip >= 0 ? 1 : 0);
    bool mbf_any = false;                  // (masked float32 classes screened on the bf16 cores share their scratch buffers)
    for (const SizeClass& sc : c->classes) mbf_any = mbf_any || (sc.mask_bf16 && R.mbf_thr_on);
    if (c->classes.size() > 1 && n_todo > 0 && c->class_lanes > 1 && !R.refine && !R.f32_exact && !mbf_any)
        n_lanes = (int)std::min<size_t>(skip >= 0 ? n_todo + 1 : n_todo, (size_t)c->class_lanes);
    if (n_lanes > 1) {
        MTMC(ensure_lanes(c, n_lanes - 1));
        if (!c->lane_fork) HIPC(hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming));
        MTMC(ensure_square_planes(c));                  // shared by the masked classes of every lane: before the fork
        if (fork == nullptr || c->sq_valid) {           // (the planes of I^2 were just queued on c->stream: fork behind them)
            HIPC(hipEventRecord(c->lane_fork, c->stream));
            fork = c->lane_fork;
        } else {                                        // banded call: behind its set-up (lane_fork, recorded by
            for (int i = 0; i + 1 < n_lanes; ++i)       // run_score_banded) and behind the last band (fork)
                HIPC(hipStreamWaitEvent(c->lanes[(size_t)i].stream, c->lane_fork, 0));
        }
        for (int i = 0; i + 1 < n_lanes; ++i) HIPC(hipStreamWaitEvent(c->lanes[(size_t)i].stream, fork, 0));
        // The float32 plane a banded upload left out is built ONCE, ahead of every lane that may read it: built lazily it
        // would be queued on whichever lane asks first while the host already marks it valid, and a class on another
        // lane could read it before it is written.  On the first lane's stream (behind the complete image, not behind
        // the banded class's last score launch on c->stream); every other stream of the call waits for it.
        if (!c->slot[c->cur].f32_valid) {
            bool any = false;
            int k = -1;
            for (const SizeClass& sc : c->classes)
                if (++k != skip) any = any || class_reads_f32(c, sc);
            if (any) {
                mtm_ctx::Lane& L0 = c->lanes[0];
                if (!c->f32_built) HIPC(hipEventCreateWithFlags(&c->f32_built, hipEventDisableTiming));
                std::swap(c->stream, L0.stream);
                const int rc = ensure_f32_plane(c);
                std::swap(c->stream, L0.stream);
                MTMC(rc);
                HIPC(hipEventRecord(c->f32_built, L0.stream));
                HIPC(hipStreamWaitEvent(c->stream, c->f32_built, 0));
                for (int i = 1; i + 1 < n_lanes; ++i) HIPC(hipStreamWaitEvent(c->lanes[(size_t)i].stream, c->f32_built, 0));
            }
        }
    }
    int k_cls = skip >= 0 ? 1 : 0;                      // the banded class went to lane 0 (c->stream)
    int idx = -1;
    for (const SizeClass& sc : c->classes) {
        if (++idx == skip) continue;
        const int lane = n_lanes > 1 ? k_cls % n_lanes : 0;
        ++k_cls;
        LaneScope scope(c, lane > 0 ? &c->lanes[(size_t)(lane - 1)] : nullptr);
        StatPlanes st;
        // slabs: the raw launches read no statistics (slab_combine_kernel does) - their side streams fork HERE, ahead of
        // the statistics pass, which then runs under them (2048^2 x 414x400: hsum + vsum took 0.25 of the call's 1.16 ms)
        c->slab_fork_early = false;
        if (!sc.slabs.empty() && sc.kernel == MTM_KERNEL_MFMA) {
            if (!c->slab_fork) HIPC(hipEventCreateWithFlags(&c->slab_fork, hipEventDisableTiming));
            HIPC(hipEventRecord(c->slab_fork, c->stream));
            c->slab_fork_early = true;
        }
        const int rc_st = launch_stats(c, R, sc, &st);
        const int rc_ncc = rc_st == MTM_OK ? launch_ncc(c, R, sc, sc.tlist_off, (int)sc.members.size(), st) : rc_st;
        c->slab_fork_early = false;
        MTMC(rc_ncc);
        if (R.refine && sc.kernel == MTM_KERNEL_MFMA_F32) MTMC(launch_refine_class(c, R, sc, st));
    }
    for (int i = 0; i + 1 < n_lanes; ++i) {             // join: everything after the score pass is queued on c->stream
        HIPC(hipEventRecord(c->lanes[(size_t)i].done, c->lanes[(size_t)i].stream));
        HIPC(hipStreamWaitEvent(c->stream, c->lanes[(size_t)i].done, 0));
    }
    if (R.refine && R.ext) MTMC(launch_refine_extremum(c, R));
    return MTM_OK;
}

int run_score_all(mtm_ctx* c, CallRoute& R) { return run_score_classes(c, R, -1, nullptr); }

// Time during which at least one score-kernel launch of the call was running: the launches of a banded call
// overlap (two compute streams), so their intervals are laid on the timeline of the first one and united.
int collect_ncc_time(mtm_ctx* c) {
    const int n = c->timing.ncc_launches;
    std::vector<std::pair<float, float>> iv;
    for (int i = 0; i < n; ++i) {
        float a = 0.f, d = 0.f;
        if (i > 0) HIPC(hipEventElapsedTime(&a, c->ncc_ev[0].first, c->ncc_ev[i].first));
        HIPC(hipEventElapsedTime(&d, c->ncc_ev[i].first, c->ncc_ev[i].second));
        iv.emplace_back(a, a + d);
    }
    std::sort(iv.begin(), iv.end());
    float total = 0.f, lo = 0.f, hi = -1.f, sum = 0.f;
    for (const auto& x : iv) sum += x.second - x.first;
    c->timing.ncc_sum_ms = sum;
    for (const auto& x : iv) {
        if (hi < lo || x.first > hi) {
            if (hi >= lo) total += hi - lo;
            lo = x.first;
            hi = x.second;
        } else {
            hi = std::max(hi, x.second);
        }
    }
    if (hi >= lo) total += hi - lo;
    c->timing.ncc_kernel_ms = total;
    float sq_ms = 0.f;
    for (int i = 0; i < c->timing.sq_launches; ++i) {
        float d = 0.f;
        HIPC(hipEventElapsedTime(&d, c->sq_ev[(size_t)i].first, c->sq_ev[(size_t)i].second));
        sq_ms += d;
    }
    c->timing.masked_stat_ms = sq_ms;
    return MTM_OK;
}

// Asynchronous half of mtm_find_matches: statistics, score kernels, the upload of the next image and (usual
// case) the copy of the candidate list into pinned memory are queued; nothing waits for the GPU.
// Can the image of a fused call arrive in row bands (copy / layout / statistics of band k+1 under the score
// kernel of band k)?  One unmasked single-channel uint8 size class on the MFMA kernel with the fused
// statistics kernel; anything else uploads the image in one piece (still without a round trip to the host).
static bool class_bandable(const mtm_ctx* c, const ImageArgs& a, const SizeClass& sc, double* work, bool any_fill = false);

// Several size classes: the class with the most multiply-accumulates among those that qualify is the one that runs under
// the upload (c->banded_cls); the others follow on the complete image (run_score_banded).
bool banded_ok(mtm_ctx* c, const ImageArgs& a, bool* single_band) {
    c->banded_cls = -1;
    double best = 0.0;
    for (size_t i = 0; i < c->classes.size(); ++i) {
        double work = 0.0;
        if (class_bandable(c, a, c->classes[i], &work) && work > best) {
            best = work;
            c->banded_cls = (int)i;
        }
    }
    *single_band = false;
    if (c->banded_cls < 0 && c->classes.size() == 1 && a.dtype == MTM_U8) {
        // Round 5: a call too small to be worth two score launches (1080p x 8 templates) still takes the banded path's
        // kernels, as ONE band - layout conversion inside the statistics launch, the candidate header cleared there: two
        // launches and a fill command fewer than the plain upload path
        double work = 0.0;
        if (class_bandable(c, a, c->classes[0], &work, true)) {
            c->banded_cls = 0;
            *single_band = true;
        }
    }
    return c->banded_cls >= 0;
}

static bool class_bandable(const mtm_ctx* c, const ImageArgs& a, const SizeClass& sc, double* work, bool any_fill) {
    const bool u16 = a.dtype == MTM_U16;
    if (a.dtype == MTM_F32) {
        // Round 6: single-channel float32 images whose one size class runs the bf16 kernel - 33 MB cross PCIe at 4K, 0.7 ms
        // next to a 1.9 ms score launch since the one-product screen; two bands, the second under the first's score launch
        if (any_fill || c->upload_bands.size() < 2 || a.chans != 1 || c->classes.size() != 1 || sc.masked || sc.w > 1024 ||
            sc.kernel != MTM_KERNEL_MFMA_F32)
            return false;
        const int oh = a.rows - sc.h + 1;
        if (!((size_t)a.rows * a.cols >= ((size_t)1 << 20) && oh >= 8 * kVsumBand)) return false;
        *work = (double)oh * (a.cols - sc.w + 1) * sc.h * sc.w * (double)sc.members.size();
        return true;
    }
    if (c->upload_bands.size() < 2 || (a.dtype != MTM_U8 && !u16) || a.chans != 1) return false;
    if (sc.masked || !c->fuse_stats || !sc.slabs.empty() || sc.kernel != (u16 ? MTM_KERNEL_MFMA16 : MTM_KERNEL_MFMA))
        return false;
    const StatsRoute route = stats_route(a.dtype, 1, sc.h, sc.w, a.cols, true);
    if (route != kStatsRouteU8 && route != kStatsRouteU16) return false;                                   // the fused statistics
    if (!any_fill && !((size_t)a.rows * a.cols >= ((size_t)1 << 20) && a.rows - sc.h + 1 >= 256)) return false;
    if (any_fill) return true;
    // A band's score launch must still fill the chip: two work-groups per CU are resident, and a launch of fewer than a
    // couple of such generations runs at the latency of its last one.  1080p x 8 templates is 512 work items in all -
    // banded 0.26 ms per call (two launches of 55 us for 62 us of work), in one piece 0.22 ms.
    const int oh = a.rows - sc.h + 1, ow = a.cols - sc.w + 1, n = (int)sc.members.size();
    const int rows_per_item = u16 ? kMfRows : sc.rm_R > 0 ? 8 * sc.rm_R : (sc.r2 ? sc.r2 * kMfRows : kMfRows);
    const int tg = u16 ? (n + 15) / 16 : sc.rm_R > 0 ? 1 : (n + (sc.r2 ? 16 : 32) - 1) / (sc.r2 ? 16 : 32);
    const long long items = (long long)((ow + kMfSeg - 1) / kMfSeg) * ((oh + rows_per_item - 1) / rows_per_item) * tg;
    const int cus = c->n_cus > 0 ? c->n_cus : 256;
    *work = (double)oh * ow * sc.h * sc.w * n;
    // MTM_BAND_MIN_FILL (default 1: the first band's launch is at least one full generation of resident work-groups; 0:
    // always band).  Measured at 4K (tools/probes/two_class_probe.py): 2 x 16 templates 48x64 (first band = 0.97
    // generations) 0.819 ms unbanded, 0.795 banded; 2 x 8 templates (0.49) 0.591 / 0.582; 1080p x 8 (0.125) 0.22 / 0.26.
    return (double)items * c->upload_bands[0] >= 0.97 * c->band_min_fill * (2.0 * cus);
}

// The score pass of a fused call with a banded upload.  copy_stream: per band the rows' copy, their layout
// conversion and the window statistics of the output rows that became computable; c->stream: the score kernel
// over the row blocks whose statistics exist, behind the band's event.  With a pageable source every copy call
// blocks the host while its rows are staged - the kernels queued before it run meanwhile.
// ... of a float32 image (round 6): two bands; the first ends where ~30 % of the output rows are complete, at a whole number of
// vsum bands (their column sums restart per band: the statistics planes are those of one launch) - the second band's 23 MB
// cross PCIe under the first band's score launch.  The rows go straight into the padded float32 plane.
static int run_score_banded_f32(mtm_ctx* c, CallRoute& R, const ImageArgs& a) {
    const SizeClass& sc = c->classes[(size_t)c->banded_cls];
    if (!R.hits_only) MTMC(ensure_maps(c));
    MTMC(ensure_copy_stream(c));
    mtm_ctx::ImageSlot& sl = c->slot[c->cur];
    SlotGeom g{};
    MTMC(prepare_slot(c, sl, a.rows, a.cols, 1, a.dtype, c->copy_stream, 1, &g));
    while ((int)c->band_ev.size() < 2) {
        hipEvent_t e;
        HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->band_ev.push_back(e);
    }
    const hipStream_t bs0 = c->copy_stream;
    if (R.f32_exact) {
        // (this call's method / mode sends the class to the float64 kernel after all - decided behind the banding decision:
        // the whole image in one piece, then the plain score pass)
        MTMC(upload_rows_f32c1(sl, g, a.px, a.stride, 0, a.rows, bs0));
        HIPC(hipEventRecord(c->band_ev[0], bs0));
        HIPC(hipStreamWaitEvent(c->stream, c->band_ev[0], 0));
        HIPC(hipEventRecord(c->ev[0], c->stream));
        return run_score_all(c, R);
    }
    const int h = sc.h, oh = a.rows - h + 1;
    const int nyb = (oh + kBfRows - 1) / kBfRows;
    const double frac = std::min(0.6, std::max(0.1, c->upload_bands[0] + 0.05));
    const int o_split = std::max(kVsumBand, ((int)(frac * oh) / kVsumBand) * kVsumBand);      // < oh: class_bandable asked for 8 bands
    const hipStream_t bs = c->copy_stream;
    StatPlanes st;
    int r_done = 0;
    for (int k = 0; k < 2; ++k) {
        const bool last = k == 1;
        const int r1 = last ? a.rows : o_split + h - 1;
        MTMC(upload_rows_f32c1(sl, g, a.px, a.stride, r_done, r1, bs));
        if (k == 0) HIPC(hipEventRecord(c->ev[0], c->stream));          // (see fm_begin)
        // (the output rows the band completes, the image rows that have just arrived)
        const StatBand band{bs, last ? o_split / kStatBand4 : 0, last ? -1 : o_split / kStatBand4, r_done, r1};
        MTMC(launch_stats(c, R, sc, &st, band));
        r_done = r1;
        HIPC(hipEventRecord(c->band_ev[(size_t)k], bs));
        (void)hipStreamQuery(bs);
        HIPC(hipStreamWaitEvent(c->stream, c->band_ev[(size_t)k], 0));
        MTMC(launch_ncc(c, R, sc, sc.tlist_off, (int)sc.members.size(), st, -1, last ? o_split / kBfRows : 0, last ? nyb : o_split / kBfRows));
        (void)hipStreamQuery(c->stream);
    }
    // what run_score_all does behind a bf16 class's launch: the exact re-scoring of what the screen listed
    if (R.refine) {
        MTMC(launch_refine_class(c, R, sc, st));
        if (R.ext) MTMC(launch_refine_extremum(c, R));
    }
    return MTM_OK;
}

int run_score_banded(mtm_ctx* c, CallRoute& R, const ImageArgs& a) {
    if (a.dtype == MTM_F32) return run_score_banded_f32(c, R, a);
    const SizeClass& sc = c->classes[(size_t)c->banded_cls];
    host_trace(c, 16);
    if (!R.hits_only) MTMC(ensure_maps(c));
    MTMC(ensure_copy_stream(c));
    host_trace(c, 17);
    mtm_ctx::ImageSlot& sl = c->slot[c->cur];
    SlotGeom g{};
    const bool u16 = a.dtype == MTM_U16;
    static const std::vector<double> kOneBand{1.0};
    const std::vector<double>& bands = R.single_band ? kOneBand : c->upload_bands;
    const int nb = (int)bands.size();
    // (Round 4 measured three other layouts of the same work against this one and round 5 removed their code: the first
    // band on the score stream itself, consecutive bands on two copy-side streams, score launches alternating between two
    // streams - all within +-2 %, docs/HISTORY.md.)
    MTMC(prepare_slot(c, sl, a.rows, a.cols, 1, a.dtype, c->copy_stream, 1, &g));
    host_trace(c, 13);
    while ((int)c->band_ev.size() < nb) {
        hipEvent_t e;
        HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->band_ev.push_back(e);
    }
    int k_prev = -1;                        // the band queued before this one (bands without rows are skipped)
    const int h = sc.h, oh = a.rows - h + 1;
    const int RB = u16 ? kMfRows : sc.rm_R > 0 ? 8 * sc.rm_R : (sc.r2 ? sc.r2 * kMfRows : kMfRows);   // output rows per score-kernel row block
    const int nyb = (oh + RB - 1) / RB, nsb = (oh + kStatBand4 - 1) / kStatBand4;
    int r_done = 0, sb_done = 0, yb_done = 0;
    // Round 5 (MTM_BAND_ALIGN, default 1): a band ends where its score launch is a whole number of generations of resident
    // work-groups (two per CU): the configured fractions are moved to the nearest such boundary, at least one generation
    // per launch.  (A part-filled last generation runs as long as a full one; on some boxes a first band of 0.25 of the
    // rows - 3.46 generations at 4K x 32 templates - cost 11 us of kernel time against 0.28 = 3.93, profiles/r05b.)
    double gen_blocks = 0.0;                // output row blocks per generation
    {
        const int ow = a.cols - sc.w + 1, n = (int)sc.members.size();
        const int tg = u16 ? (n + 15) / 16 : sc.rm_R > 0 ? 1 : (n + (sc.r2 ? 16 : 32) - 1) / (sc.r2 ? 16 : 32);
        const int per_block = ((ow + kMfSeg - 1) / kMfSeg) * tg;
        const int cus = c->n_cus > 0 ? c->n_cus : 256;
        gen_blocks = 2.0 * cus / (double)per_block;
    }
    int yb_target = 0;
    const hipStream_t bs = c->copy_stream;
    for (int k = 0; k < nb; ++k) {
        bool last = k == nb - 1;
        int r1 = last ? a.rows : std::min(a.rows, (int)(bands[(size_t)k] * a.rows) & ~7);
        if (!last && gen_blocks > 0.0) {
            const double want = bands[(size_t)k] * nyb - yb_target;                  // row blocks of this band's launch
            const int gens = std::max(1, (int)std::floor(want / gen_blocks + 0.5));
            yb_target = std::min(nyb, yb_target + std::max(1, (int)std::floor(gens * gen_blocks)));
            // the rows that complete those blocks' windows (and their statistics blocks of kStatBand4 rows)
            const int need = ((yb_target * RB + kStatBand4 - 1) / kStatBand4) * kStatBand4 + h - 1;
            r1 = std::min(a.rows, (need + 7) & ~7);
            if (yb_target >= nyb) r1 = a.rows;
        }
        if (r1 <= r_done) continue;
        last = last || r1 >= a.rows;            // (a band that reaches the end of the image is the last one: every block left)
        if (r_done == 0) host_trace(c, 14);
        // Round 5 (MTM_FUSE_LAYOUT, default 1): a band whose rows complete new statistics blocks gets ONE kernel for layout
        // conversion + window statistics instead of two launches with a kernel boundary between them (stats_u8_kernel's
        // StatLayout; row lengths that are multiples of 4, no float32 plane asked for)
        const int avail = r1 - h + 1;                            // output rows whose windows are complete
        const int sb1 = last ? nsb : std::max(sb_done, avail > 0 ? avail / kStatBand4 : 0);
        const bool fuse_lay = c->fuse_layout != 0 && !u16 && (a.cols % 4) == 0 && sb1 > sb_done;
        if (u16)
            MTMC(upload_rows_u16c1(sl, g, a.px, a.stride, r_done, r1, bs));
        else
            MTMC(upload_rows_u8c1(sl, g, a.px, a.stride, r_done, r1, bs, true, nullptr, nullptr, !fuse_lay));
        // (the band's statistics launch: its row units, and the rows it converts on the way)
        const StatBand band{bs, sb_done, sb1, fuse_lay ? r_done : 0, fuse_lay ? r1 : 0};
        if (r_done == 0) {
            HIPC(hipEventRecord(c->ev[0], c->stream));           // (see fm_begin)
            if (c->classes.size() > 1) {                         // the lanes of the other classes start behind the call's set-up too
                if (!c->lane_fork) HIPC(hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming));
                HIPC(hipEventRecord(c->lane_fork, c->stream));
            }
        }
        r_done = r1;
        host_trace(c, k == 0 ? 4 : 7);                           // the band's copy call returned
        StatPlanes st;
        MTMC(launch_stats(c, R, sc, &st, band));
        sb_done = sb1;
        HIPC(hipEventRecord(c->band_ev[(size_t)k], bs));
        (void)hipStreamQuery(bs);                                // submit now (the runtime batches commands)
        k_prev = k;
        if (k == 0) host_trace(c, 5);                            // layout conversion + statistics of band 0 submitted
        int yb1 = last ? nyb : (sb1 * kStatBand4) / RB;
        if (!last && gen_blocks > 0.0) yb1 = std::min(yb1, yb_target);      // (exactly the whole generations, not the rows' rounding on top)
        if (yb1 > yb_done) {
            if (R.zero_pending) {           // (no statistics launch took the clearing of the candidate header along)
                HIPC(hipMemsetAsync(c->cands.p, 0, 16, c->stream));
                R.zero_pending = false;
            }
            HIPC(hipStreamWaitEvent(c->stream, c->band_ev[(size_t)k], 0));
            const int rc2 = launch_ncc(c, R, sc, sc.tlist_off, (int)sc.members.size(), st, -1, yb_done, yb1);
            MTMC(rc2);
            (void)hipStreamQuery(c->stream);
            host_trace(c, k == 0 ? 6 : 8);                       // the band's score launch is submitted
            yb_done = yb1;
        }
    }
    // the other size classes, on the complete image: the first of them on a lane behind the last band's event - under
    // the banded class's last launch - the rest alternating as in run_score_all
    // (k_prev: the last band that was queued - trailing bands without rows of their own record no event)
    if (c->classes.size() > 1) MTMC(run_score_classes(c, R, c->banded_cls, c->band_ev[(size_t)(k_prev >= 0 ? k_prev : nb - 1)]));
    return MTM_OK;
}

}  // namespace mtmi

extern "C" {

// Test support: the masked float32 screen (tests/test_gpu_maskf32_screen.py) through the stage functions launch_masked_bf16
// runs - mbf_prepare, mbf_raw, mbf_list, mbf_rescore - with what they leave behind copied out in between: the two raw
// launches' sums and the bounds (maskf32_dump_kernel: maskf32_pixel and maskf32_bounds as the listing kernels call them),
// the tile constants, the score maps after the listing pass and after re-scoring, the list and the best[] keys.
int mtm_debug_maskf32_screen(mtm_ctx* c, const mtm_maskf32_screen* a) {
    if (!c || !a) {
        set_error("mtm_debug_maskf32_screen: null context or arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, "mtm_debug_maskf32_screen");
    const auto bad = [](const char* what, int rc = MTM_E_INVALID) {
        set_error(std::string("mtm_debug_maskf32_screen: ") + what);
        return rc;
    };
    if (a->list_cap < 0 || a->list_cap > kCandListMax) return bad("list_cap in 0 .. 2^20");
    if (a->set_cap) {           // only: the capacity the next search calls of this context give the screen's list (0: their own)
        c->mbf_cap_debug = a->list_cap;
        return MTM_OK;
    }
    if ((a->pieces != 1 && a->pieces != 3) || (a->mode != MTM_PEAKS_LOCAL && a->mode != MTM_PEAKS_GLOBAL) || !a->info)
        return bad("pieces 1 or 3, mode MTM_PEAKS_LOCAL or MTM_PEAKS_GLOBAL and info are needed");
    if (!c->have_image || !c->have_templ) return bad("set the image and the templates first", MTM_E_STATE);
    HIPC(hipSetDevice(c->device));
    MTMC(place_templates(c));
    // (SizeClass::mask_bf16: placement's masked_bf16_class_ok on a class of the default kernel choice)
    if (c->classes.size() != 1 || !c->classes[0].masked || !c->classes[0].mask_bf16)
        return bad("the templates are not ONE masked float32 size class the screen takes (single channel, float32 image and "
                   "templates, w <= 256, TM_SQDIFF or TM_CCORR_NORMED, MTM_OPT_F32_MFMA 1 or 3)");
    const SizeClass& sc = c->classes[0];
    const int n = (int)c->templs.size();
    if ((int)sc.members.size() != n) return bad("internal: the class does not hold every template", MTM_E_STATE);
    const int oh = c->rows - sc.h + 1, ow = c->cols - sc.w + 1;
    const size_t n_out = (size_t)n * oh * ow;
    if (a->n_templ != n || a->oh != oh || a->ow != ow) return bad("n_templ, oh, ow do not match the context's templates and image");
    MTMC(ensure_maps(c));
    MTMC(ensure_f32_plane(c));
    c->maps_valid = false;
    float* maps = c->maps.as<float>();
    const long long cap_before = c->mbf_cap_debug;
    if (a->list_cap > 0) c->mbf_cap_debug = a->list_cap;
    MaskBf16Plan P;
    const int rc_prep = mbf_prepare(c, sc, &P);
    c->mbf_cap_debug = cap_before;
    MTMC(rc_prep);
    const int nyb = P.p.nyb, nseg = P.p.nseg;
    constexpr int kCanary = 8;
    const size_t n_rec_max = (size_t)std::min<unsigned long long>(P.cap, n_out);
    if (a->tiles < (int64_t)P.n_tiles || (a->records && a->capacity < (int64_t)n_rec_max + kCanary))
        return bad("tiles below nyb * nseg, or records without room for min(list_cap, n_templ * oh * ow) + 8");
    // the list with a canary of 8 records behind its capacity
    MTMC(c->mbf_list.ensure(16 + sizeof(mtm_hit) * ((size_t)P.cap + kCanary)));
    HIPC(hipMemsetAsync(c->mbf_list.as<uint8_t>() + 16 + sizeof(mtm_hit) * (size_t)P.cap, 0xC5, sizeof(mtm_hit) * kCanary, c->stream));
    MTMC(mbf_raw(c, sc, P, a->pieces));
    HIPC(hipGetLastError());
    const MaskF32Params q = mbf_params(c, P, a->pieces, a->thr, maps);
    // the bounds, ahead of the listing pass
    const size_t o_c1 = 0, o_c2 = round_up(sizeof(float) * n_out, 256), o_lb = 2 * o_c2, o_ub = o_lb + round_up(sizeof(double) * n_out, 256);
    MTMC(c->mbf_dbg.ensure(o_ub + sizeof(double) * n_out));
    uint8_t* d = c->mbf_dbg.as<uint8_t>();
    hipLaunchKernelGGL(maskf32_dump_kernel, dim3((ow + 255) / 256, oh), dim3(256), 0, c->stream, q, n, reinterpret_cast<float*>(d + o_c1),
                       reinterpret_cast<float*>(d + o_c2), reinterpret_cast<double*>(d + o_lb), reinterpret_cast<double*>(d + o_ub));
    HIPC(hipGetLastError());
    unsigned long long count = 0;
    MTMC(mbf_list(c, P, q, a->mode == MTM_PEAKS_GLOBAL, &count));
    const auto fetch = [&](void* to, const void* from, size_t bytes) -> int {
        if (to && bytes) HIPC(hipMemcpy(to, from, bytes, hipMemcpyDeviceToHost));
        return MTM_OK;
    };
    const auto fetch_maps = [&](float* to) -> int {
        if (!to) return MTM_OK;
        for (int t = 0; t < n; ++t) {
            const TemplDev& T = c->td_host[(size_t)t];
            HIPC(hipMemcpy2D(to + (size_t)t * oh * ow, sizeof(float) * ow, maps + T.map_off, sizeof(float) * T.map_pitch,
                             sizeof(float) * ow, (size_t)oh, hipMemcpyDeviceToHost));
        }
        return MTM_OK;
    };
    MTMC(fetch(a->c1, d + o_c1, sizeof(float) * n_out));
    MTMC(fetch(a->c2, d + o_c2, sizeof(float) * n_out));
    MTMC(fetch(a->lb, d + o_lb, sizeof(double) * n_out));
    MTMC(fetch(a->ub, d + o_ub, sizeof(double) * n_out));
    MTMC(fetch(a->mu_i, q.mu_i, sizeof(float) * P.n_tiles));
    MTMC(fetch(a->mu_j, q.mu_j, sizeof(float) * P.n_tiles));
    MTMC(fetch_maps(a->map_listed));
    if (a->mode == MTM_PEAKS_GLOBAL) MTMC(fetch(a->best, c->mbf_best.p, sizeof(unsigned int) * (size_t)n));
    const unsigned long long n_rec = std::min(count, P.cap);
    int rescored = 0;
    if (a->rescore && count <= P.cap) {             // (an overflowing list is not re-scored: production repeats the screen)
        MTMC(mbf_rescore(c, sc, q, count));
        HIPC(hipStreamSynchronize(c->stream));
        rescored = 1;
    }
    MTMC(fetch_maps(a->map_rescored));
    // the records that were written, then the canary
    MTMC(fetch(a->records, q.list, sizeof(mtm_hit) * (size_t)n_rec));
    if (a->records) MTMC(fetch(a->records + n_rec, q.list + P.cap, sizeof(mtm_hit) * kCanary));
    const unsigned long long cap_production = (unsigned long long)std::min<int64_t>(std::max<int64_t>(c->hit_cap, 1 << 18), kCandListMax);
    const int64_t info[12] = {n, sc.h, sc.w, oh, ow, nyb, nseg, P.mb, (int64_t)cap_production, (int64_t)P.cap, (int64_t)count, rescored};
    std::memcpy(a->info, info, sizeof(info));
    return MTM_OK;
}

}  // extern "C"
