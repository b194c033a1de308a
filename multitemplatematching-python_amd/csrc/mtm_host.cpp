// Host-only parts of libmtm_hip.so: error string, template statistics, 1-D peak finding, the NMS,
// and what fm_end decides without the device (the 3x3 test of the candidate list, the overflow
// ladder).  Nothing here touches the GPU, so these entry points also work on a machine without one
// (the CPU test-suite exercises mtm_nms through the C ABI, tests/native/sanitize_host.cpp the rest).
#include <algorithm>
#include <cmath>
#include <cfloat>
#include <cstring>
#include <numeric>
#include <climits>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "mtm_internal.h"
#include "mtm_nms_core.h"

namespace mtm {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

// sum v and sum v^2 of a run of bytes, exact: the per-call cost of a template set the library has not seen before is
// dominated by this pass on the host (32 templates of 64 x 64: 82 us as a scalar loop, 7 us this way)
void u8_run_sums(const uint8_t* p, size_t n, unsigned long long* sum, unsigned long long* sumsq) {
    unsigned long long s = 0, q = 0;
    size_t i = 0;
#if defined(__SSE2__)
    const __m128i zero = _mm_setzero_si128();
    while (n - i >= 16) {
        // 32-bit lanes: each step adds at most 4 * 255^2 to a lane of q -> 8192 steps stay below 2^31
        const size_t steps = std::min<size_t>((n - i) / 16, 8192);
        __m128i vs = zero, vq = zero;
        for (size_t k = 0; k < steps; ++k, i += 16) {
            const __m128i v = _mm_loadu_si128((const __m128i*)(p + i));
            vs = _mm_add_epi64(vs, _mm_sad_epu8(v, zero));
            const __m128i lo = _mm_unpacklo_epi8(v, zero), hi = _mm_unpackhi_epi8(v, zero);
            vq = _mm_add_epi32(vq, _mm_add_epi32(_mm_madd_epi16(lo, lo), _mm_madd_epi16(hi, hi)));
        }
        alignas(16) unsigned long long ls[2];
        alignas(16) uint32_t lq[4];
        _mm_store_si128((__m128i*)ls, vs);
        _mm_store_si128((__m128i*)lq, vq);
        s += ls[0] + ls[1];
        q += (unsigned long long)lq[0] + lq[1] + lq[2] + lq[3];
    }
#endif
    for (; i < n; ++i) {
        const unsigned v = p[i];
        s += v;
        q += v * v;
    }
    *sum += s;
    *sumsq += q;
}

// The tail screen's split (MfmaParams::tail_split: the K steps of the two-row MFMA variant ahead of its tail screen) for an
// h x w class at the candidate threshold thr_lo.  After s steps a noise-like window's bound carries the tail term, about
// (h - s + 1) / h of the normaliser for the longer of a wave's two tails, and a partial score whose standard deviation is
// sigma_P = sqrt(s / h) / sqrt(w h); a wave leaves when all of its 8192 outputs (about 4 sigma_P) stay below the threshold
// with what the screen's block-level ranges cost on top.  The split is the smallest s in [6, h - 2] with
//   thr_lo - (h - s + 1) / h >= z sigma_P          (kTailSplitZ, measured: DESIGN 4.1 "Tail screen")
// and 0 (no screen) where no s qualifies, the threshold is negative, or s / h is above kTailSplitMaxFrac, the fraction
// beyond which a screened call - tail boxes in the statistics launch, the screen itself - no longer beats the full loop.
// Any split is correct (the bound is rigorous for every s); the rule only decides how early the waves that can leave do.
int tail_split_rule(int h, int w, double thr_lo) {
    if (!(thr_lo >= 0.0) || h < 8 || w < 1) return 0;
    for (int s = 6; s <= h - 2; ++s) {
        const double tail = (double)(h - s + 1) / (double)h;
        const double sigma = std::sqrt((double)s / (double)h) / std::sqrt((double)w * (double)h);
        if (thr_lo - tail >= kTailSplitZ * sigma) return (double)s / (double)h <= kTailSplitMaxFrac ? s : 0;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Template constants.  Follows OpenCV's common_matchTemplate (the arithmetic behind the
// cv2.matchTemplate call at reference MTM/__init__.py:92) in the operation order that
// oracle/mtm_oracle.py::match_template uses, so that both sides round identically.
// ---------------------------------------------------------------------------------------------
TemplStats compute_templ_stats(const double* px, const double* mask, int rows, int cols, int chans,
                               int method, bool integer) {
    const size_t plane = (size_t)rows * cols;
    if (mask != nullptr) {
        // matchTemplateMask: templ2_mask2_sum = norm(templ.mul(mask), NORM_L2SQR)
        double s = 0.0;
        for (int c = 0; c < chans; ++c)
            for (size_t i = 0; i < plane; ++i) {
                const double v = px[c * plane + i] * mask[c * plane + i];
                s += v * v;
            }
        return templ_stats_from_sums(nullptr, nullptr, s, true, rows, cols, chans, method);
    }
    double sum[4] = {0, 0, 0, 0}, sumsq[4] = {0, 0, 0, 0};
    for (int c = 0; c < chans && c < 4; ++c) {
        double s = 0.0, sq = 0.0;
        if (integer) {
            long long is = 0, isq = 0;
            for (size_t i = 0; i < plane; ++i) {
                const long long v = (long long)px[c * plane + i];
                is += v;
                isq += v * v;
            }
            s = (double)is;
            sq = (double)isq;
        } else {
            for (size_t i = 0; i < plane; ++i) {
                const double v = px[c * plane + i];
                s += v;
                sq += v * v;
            }
        }
        sum[c] = s;
        sumsq[c] = sq;
    }
    return templ_stats_from_sums(sum, sumsq, 0.0, false, rows, cols, chans, method);
}

// The same from the per-channel sums (sum v, sum v^2) - or, masked, from sum (v*m)^2 alone: what the device
// reduction over a template source delivers (exact integers for uint8 pixels).  The arithmetic is
// templ_stats_from_sums_inl's (mtm_templ_stats.h), which track_adopt_kernel calls on the device.
TemplStats templ_stats_from_sums(const double* sum, const double* sumsq, double templ2_mask2_sum, bool masked, int rows,
                                 int cols, int chans, int method) {
    return templ_stats_from_sums_inl(sum, sumsq, templ2_mask2_sum, masked, rows, cols, chans, method);
}

// ---------------------------------------------------------------------------------------------
// scipy.signal.find_peaks(x, height=height)[0], the 1-D branch of MTM._findLocalMax_
// (reference MTM/__init__.py:33-41): strict local maxima, a plateau yields its middle sample,
// end points are never peaks, the height test is >=.  `negate` evaluates it on -x
// (MTM._findLocalMin_, :51-53).
// ---------------------------------------------------------------------------------------------
std::vector<int> find_peaks_1d(const float* x, int n, int stride, float height, bool negate) {
    std::vector<int> peaks;
    auto at = [&](int i) { const float v = x[(size_t)i * stride]; return negate ? -v : v; };
    int i = 1;
    const int i_max = n - 1;
    while (i < i_max) {
        if (at(i - 1) < at(i)) {
            int ahead = i + 1;
            while (ahead < i_max && at(ahead) == at(i)) ++ahead;
            if (at(ahead) < at(i)) {
                const int left = i, right = ahead - 1;
                const int mid = (left + right) / 2;
                if (at(mid) >= height) peaks.push_back(mid);
                i = ahead;
            }
        }
        ++i;
    }
    return peaks;
}

void line_map_peaks(const float* line, int oh, int ow, float thr, bool mode_min, int templ_idx, int w, int h,
                    std::vector<mtm_hit>& out) {
    const int len = std::max(oh, ow);
    const float thr_q = mode_min ? -thr : thr;
    std::vector<int> pk;
    if (len == 1) {
        if ((mode_min ? -line[0] : line[0]) >= thr_q) pk.push_back(0);
    } else {
        pk = find_peaks_1d(line, len, 1, thr_q, mode_min);
    }
    for (int i : pk) {
        mtm_hit r;
        r.templ_idx = templ_idx;
        r.x = oh == 1 ? i : 0;
        r.y = oh == 1 ? 0 : i;
        r.w = w;
        r.h = h;
        r.score = line[(size_t)i];
        out.push_back(r);
    }
}

// ---------------------------------------------------------------------------------------------
// Extremum keys and published results.
// ---------------------------------------------------------------------------------------------
float order_to_float(uint32_t o) { return key_order_float(o); }

mtm_hit decode_extremum_key(unsigned long long key, bool mode_min, int templ_idx, int ow, int w, int h) {
    const uint32_t o = (uint32_t)(key >> 32);
    return key_record(key ? key_index(key) : 0u, key ? key_order_float(mode_min ? ~o : o) : NAN, templ_idx, 0, 0, ow, w, h);
}

mtm_hit decode_quality_key(unsigned long long key, bool mode_min, int templ_idx, int ow, int w, int h) {
    return quality_key_record(key, mode_min ? 1 : 0, templ_idx, 0, 0, ow, w, h);
}

int copy_out_hits(const std::vector<mtm_hit>& hits, mtm_hit* out, int64_t capacity, int64_t* n_out, const std::string& msg) {
    *n_out = (int64_t)hits.size();
    if ((int64_t)hits.size() > capacity) {
        set_error(msg);
        return MTM_E_OVERFLOW;
    }
    if (!hits.empty()) std::memcpy(out, hits.data(), sizeof(mtm_hit) * hits.size());
    return MTM_OK;
}

int publish_hits(std::vector<mtm_hit>& hits, std::vector<mtm_hit>& last_hits, mtm_hit* out, int64_t capacity,
                 int64_t* n_out, const std::string& msg) {
    last_hits.swap(hits);
    return copy_out_hits(last_hits, out, capacity, n_out, msg);
}

// ---------------------------------------------------------------------------------------------
// mtm_find_matches' synchronising half (fm_end, mtm_api.hip; its peak pass: mtm_peaks.hip): what needs no device.
// ---------------------------------------------------------------------------------------------
void verify_candidates_3x3(const mtm_hit* cd, size_t ncand, const MapDims& dims, bool mode_min, float thr_q, float padv,
                           std::vector<unsigned long long>& hk, std::vector<int>& hv, std::vector<mtm_hit>& hits, int* tflags) {
    // open-addressing table over the candidates (key -> index)
    size_t tsize = 64;
    while (tsize < 2 * ncand + 8) tsize <<= 1;
    hk.assign(tsize, 0ull);
    hv.resize(tsize);
    const size_t tmask = tsize - 1;
    auto key = [](int t, int y, int x) {
        return ((unsigned long long)(t + 1) << 42) | ((unsigned long long)y << 21) | (unsigned long long)x;
    };
    auto slot_of = [&](unsigned long long k) {
        size_t sidx = (size_t)((k * 0x9E3779B97F4A7C15ull) >> 20) & tmask;
        while (hk[sidx] != 0ull && hk[sidx] != k) sidx = (sidx + 1) & tmask;
        return sidx;
    };
    for (int i = 0; i < (int)ncand; ++i) {
        const unsigned long long k = key(cd[i].templ_idx, cd[i].y, cd[i].x);
        const size_t sidx = slot_of(k);
        if (hk[sidx] == 0ull) {         // (a pixel is listed once; keep the first if it ever were not)
            hk[sidx] = k;
            hv[sidx] = i;
        }
    }
    for (int i = 0; i < (int)ncand; ++i) {
        const mtm_hit& h = cd[i];
        const int oh = dims.oh(h.templ_idx), ow = dims.ow(h.templ_idx);
        const float v = mode_min ? -h.score : h.score;
        float mx = v;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!dy && !dx) continue;
                const int yy = h.y + dy, xx = h.x + dx;
                if (yy < 0 || yy >= oh || xx < 0 || xx >= ow) {
                    mx = fmaxf(mx, padv);
                    continue;
                }
                const size_t sidx = slot_of(key(h.templ_idx, yy, xx));
                if (hk[sidx] != 0ull) mx = fmaxf(mx, mode_min ? -cd[hv[sidx]].score : cd[hv[sidx]].score);
            }
        // (v > thr_q: every record the integer kernels list passes; the float32 screen lists with a margin)
        if (v == mx && v > thr_q) {
            hits.push_back(h);
            ++tflags[(size_t)h.templ_idx];
        }
    }
}

bool scan_flags_trivial(unsigned f) { return (f & 0xFFu) == 0 && !((f & 0xFF00u) != 0 && (f & 0xFF0000u) != 0); }
bool fused_count_trivial(long long n_peaks, int oh, int ow) { return n_peaks == (long long)oh * ow; }

LadderStep ladder_next(const mtmi::CallRoute& R, const PassOutcome& o, int attempt) {
    if (R.mode == MTM_PEAKS_GLOBAL) {
        if (!(R.refine && R.ext)) return LadderStep::Done;
        // an output whose accumulator or bound is not finite cannot be screened (Bf16Params::nf_flag): the float64 kernel
        if (o.rig_wide) return LadderStep::Float64;
        if (!o.cands_overflow) return LadderStep::Done;
        // the one-product screen's bounds let more outputs reach their template's best than the list holds: three products;
        // still more within the margin of their template's best (near-flat maps): the float64 kernel
        return R.bf16_np == 1 ? LadderStep::ThreeProducts : LadderStep::Float64;
    }
    // float32 map mode: some output that could pass the threshold has an error bound beyond what the scan's
    // tolerances cover (a low-contrast window beside a brightness step)
    if (R.pp_mode && o.rig_wide) return LadderStep::Float64;
    if (R.fused && o.cands_overflow) {
        if (!R.refine) return LadderStep::Maps;
        if (!R.pp_mode && R.bf16_np == 1) return LadderStep::ThreeProducts;
        if (!R.pp_mode && !R.raw_rig) return LadderStep::MapScan;
        return LadderStep::Float64;         // (the map scan's potential peaks overflowed too: plateau-rich maps)
    }
    if (!o.hits_overflow) return LadderStep::Done;
    return R.sparse && attempt >= 1 ? LadderStep::GrowListLeaveSegments : LadderStep::GrowList;
}

void ladder_apply(mtmi::CallRoute& R, LadderStep s) {
    switch (s) {
        case LadderStep::Done: break;
        case LadderStep::ThreeProducts: R.bf16_np = 3; break;
        case LadderStep::MapScan:
            R.hits_only = false;
            R.pp_mode = R.refine_scan = true;
            break;
        case LadderStep::Float64:
            R.raw_rig = R.refine = R.refine_scan = R.pp_mode = false;
            R.fused = R.hits_only = R.ext = false;
            R.f32_exact = true;
            break;
        case LadderStep::Maps: R.fused = R.hits_only = false; break;
        case LadderStep::GrowListLeaveSegments:
            R.sparse = R.seg_skip_used = false;
            [[fallthrough]];
        case LadderStep::GrowList: R.fused = false; break;
    }
}

// ---------------------------------------------------------------------------------------------
// cv2.dnn.NMSBoxes (OpenCV dnn/nms.cpp + nms.inl.hpp) as called at reference MTM/NMS.py:78.
// ---------------------------------------------------------------------------------------------
static inline float rect_overlap(const mtm_hit& a, const mtm_hit& b) {
    // 1.f - (float)jaccardDistance(a, b) for Rect_<int>
    const long long aa = (long long)a.w * a.h, ab = (long long)b.w * b.h;
    if (aa + ab <= 0) return 1.0f;
    const int x1 = std::max(a.x, b.x), y1 = std::max(a.y, b.y);
    const int x2 = std::min(a.x + a.w, b.x + b.w), y2 = std::min(a.y + a.h, b.y + b.h);
    const int iw = x2 - x1, ih = y2 - y1;
    if (iw <= 0 || ih <= 0) return 0.0f;      // disjoint: 1.f - (float)(1.0 - 0.0 / u), without the division
    const double aab = (double)((long long)iw * ih);
    const double dist = 1.0 - aab / ((double)aa + (double)ab - aab);
    return 1.0f - (float)dist;
}

namespace {

// float -> uint32 whose unsigned order is the float order (-0 == +0 must be normalised by the caller; NaN sorts high)
inline uint32_t float_order(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Stable LSD radix sort (8-bit digits) of `rec` by the `key_bytes` low bytes of Rec::key(), ascending.  Digits that are
// the same in every record cost one histogram pass and no move.
template <typename Rec, int KEY_BYTES>
void radix_sort(std::vector<Rec>& rec) {
    std::vector<Rec> tmp(rec.size());
    Rec* src = rec.data();
    Rec* dst = tmp.data();
    const size_t n = rec.size();
    for (int d = 0; d < KEY_BYTES; ++d) {
        size_t hist[256] = {0};
        for (size_t i = 0; i < n; ++i) ++hist[src[i].digit(d)];
        if (hist[src[0].digit(d)] == n) continue;
        size_t sum = 0;
        for (int b = 0; b < 256; ++b) {
            const size_t c = hist[b];
            hist[b] = sum;
            sum += c;
        }
        for (size_t i = 0; i < n; ++i) dst[hist[src[i].digit(d)]++] = src[i];
        std::swap(src, dst);
    }
    if (src != rec.data()) std::memcpy(rec.data(), src, n * sizeof(Rec));
}

struct HitRec {           // ascending (templ, ~order(quality), y, x)
    uint64_t lo;          // [~order(quality) : 32][y : 16][x : 16]
    uint32_t templ;
    uint32_t idx;
    unsigned digit(int d) const { return d < 8 ? (unsigned)(lo >> (8 * d)) & 255u : (unsigned)(templ >> (8 * (d - 8))) & 255u; }
};

struct ScoreRec {         // ascending ~order(score) = descending score
    uint32_t key, idx;
    unsigned digit(int d) const { return (key >> (8 * d)) & 255u; }
};

}  // namespace

void sort_hits(std::vector<mtm_hit>& hits, bool mode_min) {
    const size_t n = hits.size();
    bool radix = n >= 512;
    for (size_t i = 0; i < n && radix; ++i)
        radix = hits[i].x >= 0 && hits[i].x < 65536 && hits[i].y >= 0 && hits[i].y < 65536 && hits[i].templ_idx >= 0 &&
                hits[i].score == hits[i].score;
    if (!radix) {
        std::sort(hits.begin(), hits.end(), [&](const mtm_hit& a, const mtm_hit& b) {
            if (a.templ_idx != b.templ_idx) return a.templ_idx < b.templ_idx;
            const float qa = mode_min ? -a.score : a.score, qb = mode_min ? -b.score : b.score;
            if (qa != qb) return qa > qb;
            if (a.y != b.y) return a.y < b.y;
            return a.x < b.x;
        });
        return;
    }
    std::vector<HitRec> rec(n);
    for (size_t i = 0; i < n; ++i) {
        const float q = (mode_min ? -hits[i].score : hits[i].score) + 0.0f;      // -0 -> +0: equal qualities, equal keys
        rec[i].lo = ((uint64_t)(~float_order(q)) << 32) | ((uint64_t)(uint32_t)hits[i].y << 16) | (uint32_t)hits[i].x;
        rec[i].templ = (uint32_t)hits[i].templ_idx;
        rec[i].idx = (uint32_t)i;
    }
    radix_sort<HitRec, 12>(rec);
    std::vector<mtm_hit> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = hits[rec[i].idx];
    hits.swap(out);
}

static void nms_greedy(const mtm_hit* hits, const std::vector<int32_t>& cand, float nms_threshold, std::vector<int32_t>& keep,
                       int64_t n_sure = 0);

void nms_boxes(const mtm_hit* hits, int64_t n, const float* scores, float score_threshold,
               float nms_threshold, std::vector<int32_t>& keep) {
    std::vector<int32_t> cand;
    cand.reserve((size_t)n);
    bool radix = n >= 512;
    for (int64_t i = 0; i < n; ++i)
        if (scores[i] > score_threshold) {            // (false for NaN)
            cand.push_back((int32_t)i);
        }
    if (radix) {
        // descending score, ties in input order: a stable radix sort on the ordered bits (-0 normalised: -0 == +0 in the
        // comparison-based sort below)
        std::vector<ScoreRec> rec(cand.size());
        for (size_t k = 0; k < cand.size(); ++k) {
            rec[k].key = ~float_order(scores[cand[k]] + 0.0f);
            rec[k].idx = (uint32_t)cand[k];
        }
        if (!rec.empty()) radix_sort<ScoreRec, 4>(rec);
        for (size_t k = 0; k < cand.size(); ++k) cand[k] = (int32_t)rec[k].idx;
    } else {
        std::stable_sort(cand.begin(), cand.end(),
                         [&](int32_t a, int32_t b) { return scores[a] > scores[b]; });
    }
    nms_greedy(hits, cand, nms_threshold, keep);
}

// MTM's NMS on a hit list in ANY order (mtm_find_matches_image_nms): what nms_boxes selects from the list in the order
// mtm_find_matches returns, without producing that order first - one radix sort by the transformed score, and only runs of
// equal scores (exact copies at 1.0) are put into the order they would arrive in (mtm_nms_core.h: nms_earlier).
void nms_select(const mtm_hit* hits, int64_t n, int ascending, float score_threshold, float nms_threshold,
                std::vector<int32_t>& keep, int64_t n_sure) {
    std::vector<ScoreRec> rec;
    rec.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const float s = nms_score(hits[i], ascending);
        if (s > score_threshold) rec.push_back(ScoreRec{~float_order(s), (uint32_t)i});      // (false for NaN)
    }
    if (rec.size() >= 64) radix_sort<ScoreRec, 4>(rec);
    else std::sort(rec.begin(), rec.end(), [](const ScoreRec& a, const ScoreRec& b) { return a.key < b.key; });
    for (size_t a = 0; a < rec.size();) {
        size_t b = a + 1;
        while (b < rec.size() && rec[b].key == rec[a].key) ++b;
        if (b - a > 1)
            std::sort(rec.begin() + (long)a, rec.begin() + (long)b,
                      [&](const ScoreRec& p, const ScoreRec& q) { return nms_earlier(hits[p.idx], hits[q.idx], ascending); });
        a = b;
    }
    std::vector<int32_t> cand(rec.size());
    for (size_t k = 0; k < rec.size(); ++k) cand[k] = (int32_t)rec[k].idx;
    nms_greedy(hits, cand, nms_threshold, keep, n_sure);
}

static void nms_greedy(const mtm_hit* hits, const std::vector<int32_t>& cand, float nms_threshold, std::vector<int32_t>& keep,
                       int64_t n_sure) {
    keep.clear();

    // Same greedy decisions as OpenCV's NMSFast_ (a candidate is kept iff its overlap with EVERY kept
    // box is <= nms_threshold), but a candidate is only compared with the kept boxes that can touch
    // it: disjoint boxes have overlap 0 <= nms_threshold.  Kept boxes are hashed by the grid cell of
    // their top-left corner, cell = largest box side, so 3x3 cells cover every possible partner.
    // O(n) instead of O(n^2) for the thousands of hits a multi-GPU gather produces.
    long long cell = 1;
    bool regular = nms_threshold >= 0.0f;
    for (int32_t i : cand) {
        if (hits[i].w <= 0 || hits[i].h <= 0) regular = false;
        cell = std::max<long long>(cell, std::max(hits[i].w, hits[i].h));
    }
    if (!regular || cand.size() < 64) {          // degenerate boxes / tiny lists: plain double loop
        for (int32_t idx : cand) {
            bool ok = true;
            for (size_t k = 0; k < keep.size() && ok; ++k)
                ok = rect_overlap(hits[idx], hits[keep[k]]) <= nms_threshold;
            if (ok) keep.push_back(idx);
        }
        return;
    }
    auto fdiv = [](long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    // dense grid of singly linked lists (head per cell, next per box) over the candidates' extent
    long long cx0 = LLONG_MAX, cy0 = LLONG_MAX, cx1 = LLONG_MIN, cy1 = LLONG_MIN;
    for (int32_t i : cand) {
        const long long cx = fdiv(hits[i].x, cell), cy = fdiv(hits[i].y, cell);
        cx0 = std::min(cx0, cx); cx1 = std::max(cx1, cx);
        cy0 = std::min(cy0, cy); cy1 = std::max(cy1, cy);
    }
    const long long gw = cx1 - cx0 + 3, gh = cy1 - cy0 + 3;      // one empty ring around the extent
    if (gw * gh > (1ll << 24)) {                                  // absurdly sparse: plain double loop
        for (int32_t idx : cand) {
            bool ok = true;
            for (size_t k = 0; k < keep.size() && ok; ++k)
                ok = rect_overlap(hits[idx], hits[keep[k]]) <= nms_threshold;
            if (ok) keep.push_back(idx);
        }
        return;
    }
    // Lists are kept in insertion order (head = the cell's best box): a candidate of a dense cluster is almost always
    // suppressed by the cluster's top, which is then the first box it meets; the own cell is visited first.  The kept
    // boxes live in one compact array in the order they were kept (the lists link into it).
    //
    // The decision "overlap <= nms_threshold" is OpenCV's float expression 1.f - (float)(1.0 - inter / union), a
    // non-decreasing step function of r = inter / union: there is one r* with  overlap <= threshold  <=>  r <= r*.  It is
    // found by bisection on the expression itself; a pair is then decided by inter vs r* x union - no division - unless it
    // falls within 1e-12 (relative) of the step, where the original expression decides.
    auto overlap_of = [](double r) { return 1.0f - (float)(1.0 - r); };
    double r_star = 2.0;                                  // threshold >= 1: nothing is ever suppressed
    if (overlap_of(1.0) > nms_threshold) {
        double lo = 0.0, hi = 1.0;                        // overlap_of(lo) <= threshold < overlap_of(hi)
        for (int it = 0; it < 100 && hi - lo > 0.0; ++it) {
            const double mid = lo + 0.5 * (hi - lo);
            if (mid <= lo || mid >= hi) break;
            if (overlap_of(mid) <= nms_threshold) lo = mid;
            else hi = mid;
        }
        r_star = lo;
    }
    const double r_lo = r_star * (1.0 - 1e-12), r_hi = r_star * (1.0 + 1e-12);
    struct Kept { int x, y, x2, y2; double area; int32_t next; };
    std::vector<Kept> kb;
    kb.reserve(cand.size());
    std::vector<int32_t> head((size_t)(gw * gh), -1), tail((size_t)(gw * gh), -1);
    static const int kOrder[9][2] = {{0, 0}, {0, -1}, {0, 1}, {-1, 0}, {1, 0}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
    const bool cell_pow2 = (cell & (cell - 1)) == 0;
    int cell_shift = 0;
    while ((1ll << cell_shift) < cell) ++cell_shift;
    for (int32_t idx : cand) {
        const mtm_hit& b = hits[idx];
        const long long cx = (cell_pow2 && b.x >= 0 ? (long long)(b.x >> cell_shift) : fdiv(b.x, cell)) - cx0 + 1;
        const long long cy = (cell_pow2 && b.y >= 0 ? (long long)(b.y >> cell_shift) : fdiv(b.y, cell)) - cy0 + 1;
        const int bx2 = b.x + b.w, by2 = b.y + b.h;
        const double barea = (double)((long long)b.w * b.h);
        bool ok = true;
        for (int o = 0; o < 9 && ok && idx >= n_sure; ++o)       // (idx < n_sure: kept for certain, straight into the grid)
            for (int32_t k = head[(size_t)((cy + kOrder[o][0]) * gw + cx + kOrder[o][1])]; k >= 0; k = kb[(size_t)k].next) {
                const Kept& q = kb[(size_t)k];
                const int iw = std::min(bx2, q.x2) - std::max(b.x, q.x);
                if (iw <= 0) continue;
                const int ih = std::min(by2, q.y2) - std::max(b.y, q.y);
                if (ih <= 0) continue;                               // disjoint: overlap 0 <= threshold
                const double inter = (double)((long long)iw * ih), uni = barea + q.area - inter;
                if (inter <= r_lo * uni) continue;
                if (inter >= r_hi * uni || !(rect_overlap(b, hits[keep[(size_t)k]]) <= nms_threshold)) {
                    ok = false;
                    break;
                }
            }
        if (ok) {
            const int32_t slot = (int32_t)kb.size();              // == keep.size(): kb[i] is the box of keep[i]
            keep.push_back(idx);
            kb.push_back(Kept{b.x, b.y, bx2, by2, barea, -1});
            const size_t cellidx = (size_t)(cy * gw + cx);
            if (tail[cellidx] >= 0) kb[(size_t)tail[cellidx]].next = slot;
            else head[cellidx] = slot;
            tail[cellidx] = slot;
        }
    }
}

// ---- the host plan of a tracking call (mtm_track.hip)
int plan_tracks(const std::vector<BlobTempl>& tl, int rows, int cols, int chans, int dtype, const mtm_box_unit* start,
                int n_tracks, int margin, bool reacq, const int32_t* set_off, const int32_t* set_idx, const char* who,
                TrackPlan& P) {
    P = TrackPlan{};
    const bool sets = set_off != nullptr;
    if (sets && set_off[0] != 0) {
        set_error(std::string(who) + ": set_off[0] must be 0");
        return MTM_E_INVALID;
    }
    P.set_off.assign(1, 0);
    for (int k = 0; k < n_tracks; ++k) {
        const mtm_box_unit& s = start[k];
        auto fail = [&](const char* what) {
            set_error(std::string(who) + ": track " + std::to_string(k) + what);
            return MTM_E_INVALID;
        };
        const auto listed = [&](int j) { return j >= 0 && j < (int)tl.size(); };
        const long long n_set = sets ? (long long)set_off[k + 1] - set_off[k] : 1;
        if (n_set < 1) return fail(n_set == 0 ? ": empty set" : ": set_off is not ascending");
        const int32_t* js = sets ? set_idx + set_off[k] : &s.templ_idx;
        if (s.templ_idx != js[0]) return fail(": start's template is not the first of its set");
        // (a plain track's index is checked ahead of its box, a set's behind it: the order each entry point reports in)
        if (!sets && !listed(s.templ_idx)) return fail(": template index out of range");
        if (s.y0 < 0 || s.x0 < 0 || s.rows < 1 || s.cols < 1 || s.rows > rows - s.y0 || s.cols > cols - s.x0)
            return fail(": box outside the frame");
        for (long long i = 0; i < n_set; ++i) {
            if (!listed(js[i])) return fail(": template index out of range");
            const BlobTempl& v = tl[(size_t)js[i]];
            if (v.dtype != dtype || v.chans != chans)
                return fail(": template and frames differ in pixel type or channel count");
            if (v.rows != tl[(size_t)js[0]].rows || v.cols != tl[(size_t)js[0]].cols)
                return fail(": the templates of a set must be of one shape");
        }
        const BlobTempl& t = tl[(size_t)s.templ_idx];
        if (t.rows > s.rows || t.cols > s.cols) return fail(": template larger than the box");
        if (dtype == MTM_U16 && (long long)t.rows * t.cols > (1ll << 21))
            return fail(": uint16 template of more than 2^21 pixels");
        const long long wh = rows - t.rows + 1, ww = cols - t.cols + 1;         // the whole-frame map
        if (reacq) {
            if (wh * ww >= (1ll << 32)) return fail(": whole-frame map of 2^32 outputs or more");
            P.tiles_max = std::max(P.tiles_max, (unsigned long long)((wh + kTrackTile - 1) / kTrackTile) *
                                                    (unsigned long long)((ww + kTrackTile - 1) / kTrackTile));
            P.groups_max = std::max(P.groups_max, (unsigned long long)((n_set + kTrackNV - 1) / kTrackNV));
        }
        const int u0 = (int)P.units.size(), u1 = u0 + (int)n_set;
        const int oh = s.rows - t.rows + 1, ow = s.cols - t.cols + 1;
        for (long long i = 0; i < n_set; ++i) P.units.push_back(TrackUnit{js[i], s.y0, s.x0, oh, ow});
        P.set_off.push_back(u1);
        P.templ_bytes.push_back((size_t)t.rows * t.cols * (t.dtype == MTM_U16 ? 2 : t.chans));
        // the tiles cover every map the track can have during the call: the frame-0 map, or one of at most 2 margin + 1
        // outputs per side (a box is the hit widened by the margin), neither larger than the whole-frame map
        const long long side = 2ll * margin + 1;
        const int th = (int)std::min<long long>(std::max<long long>(oh, side), wh);
        const int tw = (int)std::min<long long>(std::max<long long>(ow, side), ww);
        for (int g0 = u0; g0 < u1; g0 += kTrackNV)
            for (int ty = 0; ty < th; ty += kTrackTile)
                for (int tx = 0; tx < tw; tx += kTrackTile)
                    P.tiles.push_back(TrackTile{g0, std::min(kTrackNV, u1 - g0), ty, tx});
    }
    P.n_units = P.units.size();
    return MTM_OK;
}

// ---- the host plan of a block-matching call (mtm_blocks.hip)
int plan_blocks(int rows, int cols, int chans, int dtype, const mtm_block* blocks, int n_blocks, int margin,
                long long budget_bytes, const char* who, BlockPlan& P, bool with_tiles, bool masked) {
    P = BlockPlan{};
    P.units.reserve((size_t)n_blocks);
    P.toff.reserve((size_t)n_blocks);
    P.clip.reserve(2 * (size_t)n_blocks);
    BlockChunk cur{0, 0, 0, 0, 0};
    for (int k = 0; k < n_blocks; ++k) {
        const mtm_block& b = blocks[k];
        auto fail = [&](const char* what) {
            set_error(std::string(who) + ": block " + std::to_string(k) + what);
            return MTM_E_INVALID;
        };
        if (b.w < 1 || b.h < 1) return fail(": empty block");
        if (b.x < 0 || b.y < 0 || b.w > cols - b.x || b.h > rows - b.y) return fail(": block outside the reference");
        const long long area = (long long)b.w * b.h;
        // (uint16: correlations of up to 2^21 pixels stay below 2^53, exact in float64 as the exhaustive kernels need)
        if (dtype == MTM_U16 && area > (1ll << 21)) return fail(": uint16 block of more than 2^21 pixels");
        if (area >= (1ll << 31)) return fail(": block of 2^31 pixels or more");       // (the gather kernel's pixel index)
        // the search box (MTM.blocks.search_box) and the block's map over it
        const long long x0 = std::max(0ll, (long long)b.x - margin), y0 = std::max(0ll, (long long)b.y - margin);
        const long long x1 = std::min((long long)cols, (long long)b.x + b.w + margin);
        const long long y1 = std::min((long long)rows, (long long)b.y + b.h + margin);
        const long long oh = y1 - y0 - b.h + 1, ow = x1 - x0 - b.w + 1;
        if (oh * ow >= (1ll << 32)) return fail(": map of 2^32 outputs or more");
        // (masked: the planes of T M, then as many of the mask)
        const size_t bytes = (size_t)area * (size_t)(dtype == MTM_U16 ? 2 : chans) * (masked ? 2u : 1u);
        if (k > cur.b0 && (long long)(cur.bytes + bytes) > budget_bytes) {
            cur.b1 = k;
            cur.t1 = P.tiles.size();
            P.chunks.push_back(cur);
            cur = BlockChunk{k, k, P.tiles.size(), P.tiles.size(), 0};
        }
        P.units.push_back(TrackUnit{k, (int)y0, (int)x0, (int)oh, (int)ow});
        P.toff.push_back((long long)cur.bytes);
        P.clip.push_back((int32_t)((long long)margin - (b.x - x0)));
        P.clip.push_back((int32_t)((long long)margin - (b.y - y0)));
        cur.bytes += bytes;
        P.max_bytes = std::max(P.max_bytes, cur.bytes);
        for (int ty = 0; with_tiles && ty < (int)oh; ty += kTrackTile)
            for (int tx = 0; tx < (int)ow; tx += kTrackTile) P.tiles.push_back(TrackTile{k, 1, ty, tx});
    }
    if (n_blocks > 0) {
        cur.b1 = n_blocks;
        cur.t1 = P.tiles.size();
        P.chunks.push_back(cur);
    }
    return MTM_OK;
}

// ---- the fixed tile table and the passes of a call whose boxes the device computes (mtm_blocks.hip)
int fix_block_tiles(BlockPlan& P, int rows, int cols, const mtm_block* blocks, int margin, const char* who) {
    const long long side = 2ll * margin + 1;
    const size_t n = P.units.size();
    // block k's grid covers the largest map a moved block can have: 2 margin + 1 outputs per side, or the whole image's
    auto span_h = [&](size_t k) { return std::min(side, (long long)rows - blocks[k].h + 1); };
    auto span_w = [&](size_t k) { return std::min(side, (long long)cols - blocks[k].w + 1); };
    unsigned long long total = 0;
    for (size_t k = 0; k < n; ++k) {
        const long long oh = span_h(k), ow = span_w(k);
        if (oh * ow >= (1ll << 32)) {
            set_error(std::string(who) + ": block " + std::to_string(k) + ": map of 2^32 outputs or more");
            return MTM_E_INVALID;
        }
        total += (unsigned long long)((oh + kTrackTile - 1) / kTrackTile) * (unsigned long long)((ow + kTrackTile - 1) / kTrackTile);
    }
    if (total >= (1ull << 31)) {
        set_error(std::string(who) + ": " + std::to_string(n) + " blocks at margin " + std::to_string(margin) +
                  " need 2^31 tiles or more");
        return MTM_E_INVALID;
    }
    P.tiles.clear();
    P.tiles.reserve((size_t)total);
    for (BlockChunk& C : P.chunks) {
        C.t0 = P.tiles.size();
        for (int k = C.b0; k < C.b1; ++k) {
            const int th = (int)span_h((size_t)k), tw = (int)span_w((size_t)k);
            for (int ty = 0; ty < th; ty += kTrackTile)
                for (int tx = 0; tx < tw; tx += kTrackTile) P.tiles.push_back(TrackTile{k, 1, ty, tx});
        }
        C.t1 = P.tiles.size();
    }
    return MTM_OK;
}

int plan_block_passes(int rows, int cols, int chans, int dtype, const mtm_block_pass* passes, int n_passes,
                      long long budget_bytes, const char* who, std::vector<BlockPassPlan>& plans) {
    plans.clear();
    plans.resize((size_t)n_passes);
    for (int p = 0; p < n_passes; ++p) {
        const mtm_block_pass& a = passes[p];
        BlockPassPlan& Q = plans[(size_t)p];
        const std::string pw = std::string(who) + ": pass " + std::to_string(p);
        if (a.bw < 1 || a.bh < 1 || a.sx < 1 || a.sy < 1 || a.margin < 0) {
            set_error(pw + ": block and step must be >= 1 and the margin >= 0");
            return MTM_E_INVALID;
        }
        Q.grid = block_grid_of(a, rows, cols);
        Q.margin = a.margin;
        const long long n = (long long)Q.grid.nx * Q.grid.ny;
        if (n < 1) {
            set_error(pw + ": no " + std::to_string(a.bw) + " x " + std::to_string(a.bh) + " block fits the images (empty grid)");
            return MTM_E_INVALID;
        }
        if (n > INT_MAX) {
            set_error(pw + ": grid of 2^31 blocks or more");
            return MTM_E_INVALID;
        }
        Q.blocks.reserve((size_t)n);
        for (int iy = 0; iy < Q.grid.ny; ++iy)
            for (int ix = 0; ix < Q.grid.nx; ++ix) Q.blocks.push_back(mtm_block{ix * a.sx, iy * a.sy, a.bw, a.bh});
        int rc = plan_blocks(rows, cols, chans, dtype, Q.blocks.data(), (int)n, a.margin, budget_bytes, pw.c_str(), Q.plan, false);
        if (rc == MTM_OK) rc = fix_block_tiles(Q.plan, rows, cols, Q.blocks.data(), a.margin, pw.c_str());
        if (rc != MTM_OK) return rc;
    }
    return MTM_OK;
}

// ---- the frame chunks of a block-matching call over a frame stack (mtm_blocks.hip)
std::vector<StackChunk> plan_blocks_stack(int n_frames, int frames_per_chunk, int mode) {
    std::vector<StackChunk> chunks;
    const int per = std::max(2, frames_per_chunk) - 1;         // new frames of a chunk, behind its carried frame
    for (int f0 = 1; f0 < n_frames; f0 += per)
        chunks.push_back(StackChunk{f0, std::min(per, n_frames - f0), mode == MTM_BLOCKS_REF_FIRST ? 0 : f0 - 1, f0 - 1});
    return chunks;
}

}  // namespace mtm

extern "C" {

const char* mtm_last_error(void) { return mtm::g_last_error.c_str(); }

int mtm_abi_version(void) { return MTM_ABI_VERSION; }

int mtm_debug_tail_split(int h, int w, double thr) { return mtm::tail_split_rule(h, w, thr); }

int mtm_debug_templ_stats(const void* px, int rows, int cols, int chans, int dtype, int method, double* out7) {
    if (!px || !out7 || rows < 1 || cols < 1 || chans < 1 || chans > 4 || method < MTM_TM_SQDIFF || method > MTM_TM_CCOEFF_NORMED ||
        (dtype != MTM_U8 && dtype != MTM_U16 && dtype != MTM_F32)) {
        mtm::set_error("mtm_debug_templ_stats: bad arguments");
        return MTM_E_INVALID;
    }
    const size_t plane = (size_t)rows * cols;
    std::vector<double> planar(plane * (size_t)chans);
    for (size_t p = 0; p < plane; ++p)
        for (int c = 0; c < chans; ++c) {
            const size_t i = p * (size_t)chans + (size_t)c;
            double v;
            if (dtype == MTM_U8) {
                v = (double)static_cast<const uint8_t*>(px)[i];
            } else if (dtype == MTM_U16) {
                uint16_t u;
                std::memcpy(&u, static_cast<const uint8_t*>(px) + 2 * i, sizeof(u));
                v = (double)u;
            } else {
                float f;
                std::memcpy(&f, static_cast<const uint8_t*>(px) + 4 * i, sizeof(f));
                v = (double)f;
            }
            planar[(size_t)c * plane + p] = v;
        }
    const mtm::TemplStats st = mtm::compute_templ_stats(planar.data(), nullptr, rows, cols, chans, method, dtype != MTM_F32);
    for (int c = 0; c < 4; ++c) out7[c] = st.mean[c];
    out7[4] = st.templ_norm;
    out7[5] = st.templ_sum2;
    out7[6] = (double)st.all_ones;
    return MTM_OK;
}

int mtm_debug_plan_blocks(int rows, int cols, int chans, int dtype, const mtm_block* blocks, int n_blocks, int margin,
                          int64_t budget_bytes, int32_t* tiles, int64_t tile_cap, int64_t* n_tiles, int32_t* chunk_of,
                          int64_t* toff, int32_t* maps) {
    if (rows < 1 || cols < 1 || n_blocks < 0 || (n_blocks > 0 && !blocks) || margin < 0 || tile_cap < 0 ||
        !((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        mtm::set_error("mtm_debug_plan_blocks: bad arguments");
        return MTM_E_INVALID;
    }
    mtm::BlockPlan P;
    const int rc = mtm::plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, budget_bytes, "mtm_debug_plan_blocks", P);
    if (rc != MTM_OK) return rc;
    if (n_tiles) *n_tiles = (int64_t)P.tiles.size();
    for (size_t i = 0; tiles && i < P.tiles.size() && (int64_t)i < tile_cap; ++i) {
        tiles[3 * i] = P.tiles[i].u0;
        tiles[3 * i + 1] = P.tiles[i].ty0;
        tiles[3 * i + 2] = P.tiles[i].tx0;
    }
    for (size_t ci = 0; chunk_of && ci < P.chunks.size(); ++ci)
        for (int k = P.chunks[ci].b0; k < P.chunks[ci].b1; ++k) chunk_of[k] = (int32_t)ci;
    for (int k = 0; k < n_blocks; ++k) {
        if (toff) toff[k] = P.toff[(size_t)k];
        if (maps) {
            const mtm::TrackUnit& u = P.units[(size_t)k];
            maps[4 * k] = u.x0;
            maps[4 * k + 1] = u.y0;
            maps[4 * k + 2] = u.ow;
            maps[4 * k + 3] = u.oh;
        }
    }
    return MTM_OK;
}

int mtm_debug_plan_blocks_stack(int n_frames, int frames_per_chunk, int mode, int32_t* chunks, int64_t chunk_cap,
                                int64_t* n_chunks, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                                int n_blocks, int margin, int32_t* clip) {
    if (n_frames < 2 || frames_per_chunk < 2 || (mode != MTM_BLOCKS_REF_PREVIOUS && mode != MTM_BLOCKS_REF_FIRST) ||
        chunk_cap < 0 || n_blocks < 0 || margin < 0 || (n_blocks > 0 && !blocks)) {
        mtm::set_error("mtm_debug_plan_blocks_stack: bad arguments");
        return MTM_E_INVALID;
    }
    const std::vector<mtm::StackChunk> C = mtm::plan_blocks_stack(n_frames, frames_per_chunk, mode);
    if (n_chunks) *n_chunks = (int64_t)C.size();
    for (size_t i = 0; chunks && i < C.size() && (int64_t)i < chunk_cap; ++i) {
        chunks[4 * i] = C[i].f0;
        chunks[4 * i + 1] = C[i].nf;
        chunks[4 * i + 2] = C[i].carried;
        chunks[4 * i + 3] = C[i].p0;
    }
    if (n_blocks > 0 && clip) {
        if (rows < 1 || cols < 1 || !((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
            mtm::set_error("mtm_debug_plan_blocks_stack: bad arguments");
            return MTM_E_INVALID;
        }
        mtm::BlockPlan P;
        const int rc = mtm::plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 1ll << 62,
                                        "mtm_debug_plan_blocks_stack", P);
        if (rc != MTM_OK) return rc;
        std::copy(P.clip.begin(), P.clip.end(), clip);
    }
    return MTM_OK;
}

int mtm_debug_plan_blocks_passes(int rows, int cols, int chans, int dtype, const mtm_block_pass* passes, int n_passes,
                                 int64_t budget_bytes, int64_t* counts, int32_t* tiles, int64_t tile_cap, int64_t* n_tiles,
                                 int32_t* chunk_of, const mtm_hit* coarse, int at_pass, int32_t* pred, int32_t* maps) {
    if (rows < 1 || cols < 1 || n_passes < 1 || !passes || tile_cap < 0 ||
        (coarse && (at_pass < 1 || at_pass >= n_passes)) ||
        !((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        mtm::set_error("mtm_debug_plan_blocks_passes: bad arguments");
        return MTM_E_INVALID;
    }
    std::vector<mtm::BlockPassPlan> Q;
    const int rc = mtm::plan_block_passes(rows, cols, chans, dtype, passes, n_passes, budget_bytes,
                                          "mtm_debug_plan_blocks_passes", Q);
    if (rc != MTM_OK) return rc;
    int64_t nt = 0, base = 0;
    for (int p = 0; p < n_passes; ++p) {
        const mtm::BlockPlan& P = Q[(size_t)p].plan;
        if (counts) counts[p] = (int64_t)P.units.size();
        for (size_t i = 0; i < P.tiles.size(); ++i, ++nt)
            if (tiles && nt < tile_cap) {
                tiles[4 * nt] = p;
                tiles[4 * nt + 1] = P.tiles[i].u0;
                tiles[4 * nt + 2] = P.tiles[i].ty0;
                tiles[4 * nt + 3] = P.tiles[i].tx0;
            }
        for (size_t ci = 0; chunk_of && ci < P.chunks.size(); ++ci)
            for (int k = P.chunks[ci].b0; k < P.chunks[ci].b1; ++k) chunk_of[base + k] = (int32_t)ci;
        base += (int64_t)P.units.size();
    }
    if (n_tiles) *n_tiles = nt;
    if (coarse) {
        const mtm::BlockPassPlan& F = Q[(size_t)at_pass];
        const mtm::BlockGrid& G = Q[(size_t)at_pass - 1].grid;
        for (size_t k = 0; k < F.blocks.size(); ++k) {
            long long dx, dy;
            mtm::blocks_predict_inl(G, coarse, F.blocks[k], &dx, &dy);
            const mtm::BlockUnitBox u = mtm::blocks_unit_at_inl(F.blocks[k], dx, dy, F.margin, rows, cols);
            if (pred) {
                pred[2 * k] = (int32_t)dx;
                pred[2 * k + 1] = (int32_t)dy;
            }
            if (maps) {
                maps[4 * k] = u.x0;
                maps[4 * k + 1] = u.y0;
                maps[4 * k + 2] = u.ow;
                maps[4 * k + 3] = u.oh;
            }
        }
    }
    return MTM_OK;
}

int mtm_nms(const mtm_hit* hits, int64_t n, double score_threshold, int ascending,
            int64_t n_object, double max_overlap, int32_t* keep, int64_t* n_keep) {
    if (n < 0 || (n > 0 && (hits == nullptr || keep == nullptr)) || n_keep == nullptr) {
        mtm::set_error("mtm_nms: bad arguments");
        return MTM_E_INVALID;
    }
    std::vector<float> scores((size_t)n);
    // MTM/NMS.py:73-75: scores are np.float32, so 1-score is a float32 subtraction; the threshold
    // is a python float, transformed in double and narrowed by the cv2 binding.
    for (int64_t i = 0; i < n; ++i) scores[i] = ascending ? (1.0f - hits[i].score) : hits[i].score;
    const float thr = (float)(ascending ? (1.0 - score_threshold) : score_threshold);
    std::vector<int32_t> kept;
    mtm::nms_boxes(hits, n, scores.data(), thr, (float)max_overlap, kept);
    int64_t m = (int64_t)kept.size();
    if (n_object >= 0 && m > n_object) m = n_object;   // MTM/NMS.py:81-82
    for (int64_t i = 0; i < m; ++i) keep[i] = kept[(size_t)i];
    *n_keep = m;
    return MTM_OK;
}

int mtm_nms_segments(const mtm_hit* hits, const int64_t* seg_counts, int64_t n_seg, double score_threshold, int ascending,
                     double max_overlap, int32_t* keep, int64_t* keep_counts) {
    if (n_seg < 0 || (n_seg > 0 && (seg_counts == nullptr || keep_counts == nullptr))) {
        mtm::set_error("mtm_nms_segments: bad arguments");
        return MTM_E_INVALID;
    }
    int64_t total = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        if (seg_counts[s] < 0) {
            mtm::set_error("mtm_nms_segments: negative segment length");
            return MTM_E_INVALID;
        }
        total += seg_counts[s];
    }
    if (total > 0 && (hits == nullptr || keep == nullptr)) {
        mtm::set_error("mtm_nms_segments: bad arguments");
        return MTM_E_INVALID;
    }
    // as mtm_nms: float32 scores (1 - score for the difference methods), the threshold transformed in double and narrowed
    const float thr = (float)(ascending ? (1.0 - score_threshold) : score_threshold);
    std::vector<float> scores;
    std::vector<int32_t> kept;
    int64_t off = 0, n_keep = 0;
    for (int64_t s = 0; s < n_seg; ++s) {
        const int64_t n = seg_counts[s];
        const mtm_hit* h = hits + off;
        if (n <= 1) {                                   // MTM/NMS.py: a list of one hit is returned as it is
            for (int64_t i = 0; i < n; ++i) keep[n_keep++] = (int32_t)(off + i);
            keep_counts[s] = n;
        } else {
            scores.resize((size_t)n);
            for (int64_t i = 0; i < n; ++i) scores[(size_t)i] = ascending ? (1.0f - h[i].score) : h[i].score;
            mtm::nms_boxes(h, n, scores.data(), thr, (float)max_overlap, kept);
            for (int32_t k : kept) keep[n_keep++] = (int32_t)(off + k);
            keep_counts[s] = (int64_t)kept.size();
        }
        off += n;
    }
    return MTM_OK;
}

}  // extern "C"
