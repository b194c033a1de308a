// Sanitizer driver for the host-only C++ of libmtm_hip.so (no GPU, no HIP): mtm_host.cpp (NMS, 1-D peaks, hit
// sorting, extremum-key decoding, result hand-over, template statistics, the plan of a tracking call) and mtm_group.cpp
// (worker threads, generation counter, LPT shards, host merge) are
// compiled as they are, with -fsanitize=address,undefined and again with -fsanitize=thread; the per-device context
// API the group drives (mtm_ctx_create, mtm_set_templates, mtm_find_matches_image, ...) is replaced by a fake that
// returns deterministic hits - so the group's threading protocol runs thousands of jobs under the sanitizers.
// Built and run by tests/test_native_sanitizers_cpu.py.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../multitemplatematching-python_amd/csrc/mtm_blocks_validate.h"
#include "../../multitemplatematching-python_amd/csrc/mtm_internal.h"
#include "../../multitemplatematching-python_amd/csrc/mtm_nms_core.h"
#include "../../multitemplatematching-python_amd/csrc/mtm_peak_sizing.h"
#include "../../multitemplatematching-python_amd/csrc/mtm_stats_route.h"

using namespace mtm;

// ---- fake per-device contexts (what mtm_context / _placement / _api .hip provide in the real library)
struct mtm_ctx {
    int device = 0;
    std::vector<mtm_templ> templs;
    int method = 0;
    std::vector<mtm_hit> last;
    int64_t opt = 0;
};
static std::atomic<int> g_live_ctx{0};

extern "C" {
int mtm_ctx_create(mtm_ctx** out, int device_id) {
    if (device_id < 0) {
        set_error("fake: no such device");
        return MTM_E_NO_DEVICE;
    }
    *out = new mtm_ctx();
    (*out)->device = device_id;
    ++g_live_ctx;
    return MTM_OK;
}
void mtm_ctx_destroy(mtm_ctx* c) {
    if (c) --g_live_ctx;
    delete c;
}
int mtm_set_option(mtm_ctx* c, int, int64_t v) {
    c->opt = v;
    return MTM_OK;
}
int mtm_set_templates(mtm_ctx* c, const mtm_templ* t, int n, int method) {
    c->templs.assign(t, t + n);
    c->method = method;
    return MTM_OK;
}
// every template yields (rows % 7) hits whose coordinates encode (device-independent) facts about it; a template with
// cols == 13 makes the call fail (error propagation through the worker)
int mtm_find_matches_image(mtm_ctx* c, const void* px, int rows, int cols, int, int, int64_t, int, double thr, mtm_hit* out,
                           int64_t cap, int64_t* n_out) {
    c->last.clear();
    for (size_t i = 0; i < c->templs.size(); ++i) {
        const mtm_templ& t = c->templs[i];
        if (t.cols == 13) {
            set_error("fake: template refused");
            return MTM_E_INVALID;
        }
        for (int k = 0; k < t.rows % 7; ++k) {
            mtm_hit h;
            h.templ_idx = (int)i;
            h.x = t.cols * 100 + k;
            h.y = rows - t.rows + (px ? 1 : 0);
            h.w = t.cols;
            h.h = t.rows;
            h.score = (float)thr + (float)k * 0.001f + (float)cols * 1e-6f;
            c->last.push_back(h);
        }
    }
    *n_out = (int64_t)c->last.size();
    if ((int64_t)c->last.size() > cap) {
        set_error("fake: capacity");
        return MTM_E_OVERFLOW;
    }
    if (!c->last.empty()) std::memcpy(out, c->last.data(), sizeof(mtm_hit) * c->last.size());
    return MTM_OK;
}
// page-locked memory of the group's shared image staging: plain heap here
void* mtm_host_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
void mtm_host_free(void* p) { std::free(p); }
// the in-process communicator calls: rank i = context i; the "all-gather" concatenates the lists in rank order
static std::atomic<int> g_comm_calls{0};
static std::atomic<bool> g_comm_fail{false};
int mtm_comm_init_all(mtm_ctx* const* ctxs, int n) {
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < i; ++k)
            if (ctxs[i]->device == ctxs[k]->device) {
                set_error("fake: device listed twice");
                return MTM_E_COMM;
            }
    return MTM_OK;
}
int mtm_comm_count(mtm_ctx*) { return 1; }
int mtm_comm_allgather_hits_all(mtm_ctx* const*, int n, const mtm_hit* const* local, const int64_t* n_local, mtm_hit* out,
                                int64_t cap, int64_t* counts, int64_t* n_out) {
    ++g_comm_calls;
    if (g_comm_fail.load()) {
        set_error("fake: the collective timed out");
        return MTM_E_COMM;
    }
    int64_t o = 0;
    for (int r = 0; r < n; ++r) {
        counts[r] = n_local[r];
        if (o + n_local[r] > cap) return MTM_E_OVERFLOW;
        if (n_local[r]) std::memcpy(out + o, local[r], sizeof(mtm_hit) * (size_t)n_local[r]);
        o += n_local[r];
    }
    *n_out = o;
    return MTM_OK;
}
int mtm_last_hits(mtm_ctx* c, mtm_hit* out, int64_t cap, int64_t* n_out) {
    *n_out = (int64_t)c->last.size();
    if ((int64_t)c->last.size() > cap) return MTM_E_OVERFLOW;
    if (!c->last.empty()) std::memcpy(out, c->last.data(), sizeof(mtm_hit) * c->last.size());
    return MTM_OK;
}
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #cond, __LINE__); \
            std::exit(2);                                                        \
        }                                                                        \
    } while (0)

static void test_group(std::mt19937& rng) {
    for (int nd : {1, 2, 3, 8}) {
        std::vector<int> devs(nd);
        for (int i = 0; i < nd; ++i) devs[i] = i % 3;
        mtm_group* g = nullptr;
        CHECK(mtm_group_create(&g, devs.data(), nd) == MTM_OK);
        CHECK(mtm_group_size(g) == nd && mtm_group_ctx(g, nd) == nullptr && mtm_group_ctx(g, 0) != nullptr);
        CHECK(mtm_group_set_option(g, 3, 77) == MTM_OK);
        // in-process communicators: one rank per device - refused (host merge kept) when a device is listed twice
        const bool unique_devs = nd <= 3;
        CHECK(mtm_group_set_exchange(g, MTM_GROUP_EXCHANGE_RCCL) == MTM_E_STATE);
        CHECK(mtm_group_comm_init(g) == (unique_devs ? MTM_OK : MTM_E_COMM));
        CHECK(mtm_group_comm_ranks(g) == (unique_devs ? 1 : 0));
        const int calls0 = g_comm_calls.load();
        static const uint8_t pixel = 0;
        for (int job = 0; job < 400; ++job) {
            const int n = (int)(rng() % 70);
            std::vector<mtm_templ> t((size_t)n);
            long long expect = 0;
            bool refuse = false;
            for (int i = 0; i < n; ++i) {
                std::memset(&t[i], 0, sizeof(mtm_templ));
                t[i].px = &pixel;
                t[i].rows = 1 + (int)(rng() % 40);
                t[i].cols = 1 + (int)(rng() % 40);
                if (job % 50 == 49 && i == n / 2) t[i].cols = 13;
                refuse = refuse || t[i].cols == 13;
                t[i].chans = 1;
                expect += t[i].rows % 7;
            }
            std::vector<int32_t> dev((size_t)std::max(n, 1));
            CHECK(mtm_group_shards(g, t.data(), n, 5, 500, 600, dev.data()) == MTM_OK);
            for (int i = 0; i < n; ++i) CHECK(dev[i] >= 0 && dev[i] < nd);
            const int64_t cap = job % 7 == 0 ? 3 : 4096;            // small capacity: the overflow protocol
            if (unique_devs) CHECK(mtm_group_set_exchange(g, job % 3 != 2 ? MTM_GROUP_EXCHANGE_RCCL : MTM_GROUP_EXCHANGE_HOST) == MTM_OK);
            std::vector<mtm_hit> out((size_t)cap);
            int64_t got = -1;
            int rc = mtm_group_find_matches(g, t.data(), n, 5, &pixel, 500, 600, 1, MTM_U8, 600, 0, 0.5, out.data(), cap, &got);
            if (refuse) {
                CHECK(rc == MTM_E_INVALID && std::string(mtm_last_error()).find("template refused") != std::string::npos);
                continue;
            }
            if (expect > cap) {
                CHECK(rc == MTM_E_OVERFLOW && got == expect);
                out.resize((size_t)got);
                rc = mtm_group_last_hits(g, out.data(), got, &got);
            }
            CHECK(rc == MTM_OK && got == expect);
            CHECK(mtm_group_exchange_used(g) == (unique_devs && job % 3 != 2 ? MTM_GROUP_EXCHANGE_RCCL : MTM_GROUP_EXCHANGE_HOST));
            // merged in template order, global indices, each template's own hits in the order its device produced them
            int prev = -1, k = 0;
            for (int64_t i = 0; i < got; ++i) {
                const mtm_hit& h = out[(size_t)i];
                CHECK(h.templ_idx >= prev && h.templ_idx < n);
                k = h.templ_idx == prev ? k + 1 : 0;
                prev = h.templ_idx;
                CHECK(h.w == t[(size_t)h.templ_idx].cols && h.h == t[(size_t)h.templ_idx].rows && h.x == h.w * 100 + k);
            }
        }
        CHECK(unique_devs ? g_comm_calls.load() > calls0 : g_comm_calls.load() == calls0);
        // mtm_group_find_matches_nms == mtm_nms over mtm_group_find_matches' list (overlapping boxes: the fake's hits of one
        // template sit one pixel apart), for both exchanges, finite N_object and an overflowing capacity
        for (int job = 0; job < 60; ++job) {
            const int n = 1 + (int)(rng() % 24);
            std::vector<mtm_templ> t((size_t)n);
            for (int i = 0; i < n; ++i) {
                std::memset(&t[i], 0, sizeof(mtm_templ));
                t[i].px = &pixel;
                t[i].rows = 1 + (int)(rng() % 40);
                t[i].cols = 14 + (int)(rng() % 3);          // few distinct widths: boxes of different templates coincide
                t[i].chans = 1;
            }
            if (unique_devs) CHECK(mtm_group_set_exchange(g, job & 1 ? MTM_GROUP_EXCHANGE_RCCL : MTM_GROUP_EXCHANGE_HOST) == MTM_OK);
            const int method = job % 3 == 0 ? 1 : 5;
            const double thr = 0.5, ov = (job % 4) * 0.25;
            const int64_t nobj = job % 5 == 0 ? 2 : -1;
            std::vector<mtm_hit> all(4096), fused(4096);
            int64_t n_all = -1, n_fused = -1;
            CHECK(mtm_group_find_matches(g, t.data(), n, method, &pixel, 500, 600, 1, MTM_U8, 600, 0, thr, all.data(), 4096, &n_all) == MTM_OK);
            const int64_t cap = job % 7 == 0 ? 1 : 4096;
            int rc = mtm_group_find_matches_nms(g, t.data(), n, method, &pixel, 500, 600, 1, MTM_U8, 600, thr, ov, nobj, fused.data(), cap, &n_fused);
            if (rc == MTM_E_OVERFLOW) {
                CHECK(n_fused > cap);
                rc = mtm_group_last_hits(g, fused.data(), 4096, &n_fused);
            }
            CHECK(rc == MTM_OK);
            std::vector<int32_t> keep((size_t)std::max<int64_t>(n_all, 1));
            int64_t nk = 0;
            if (n_all > 1) {
                CHECK(mtm_nms(all.data(), n_all, thr, method == 1, nobj, ov, keep.data(), &nk) == MTM_OK);
            } else {                                            // MTM/NMS.py:53-55: a list of one hit is returned as it is
                nk = n_all;
                keep[0] = 0;
                if (nobj >= 0 && nk > nobj) nk = nobj;
            }
            CHECK(nk == n_fused);
            for (int64_t i = 0; i < nk; ++i) CHECK(std::memcmp(&all[(size_t)keep[(size_t)i]], &fused[(size_t)i], sizeof(mtm_hit)) == 0);
        }
        // a failing collective costs the exchange, not the search: the lists are merged on the host, now and afterwards
        if (unique_devs) {
            CHECK(mtm_group_set_exchange(g, MTM_GROUP_EXCHANGE_RCCL) == MTM_OK);
            g_comm_fail.store(true);
            std::vector<mtm_templ> t(3);
            for (int i = 0; i < 3; ++i) {
                std::memset(&t[i], 0, sizeof(mtm_templ));
                t[i].px = &pixel;
                t[i].rows = 5 + i;
                t[i].cols = 20;
                t[i].chans = 1;
            }
            std::vector<mtm_hit> out(4096);
            int64_t got = -1;
            CHECK(mtm_group_find_matches(g, t.data(), 3, 5, &pixel, 500, 600, 1, MTM_U8, 600, 0, 0.5, out.data(), 4096, &got) == MTM_OK);
            CHECK(got == 5 + 6 + 0 && mtm_group_exchange_used(g) == MTM_GROUP_EXCHANGE_HOST);
            g_comm_fail.store(false);
            CHECK(mtm_group_set_exchange(g, MTM_GROUP_EXCHANGE_RCCL) == MTM_E_STATE);      // until mtm_group_comm_init runs again
            CHECK(mtm_group_find_matches(g, t.data(), 3, 5, &pixel, 500, 600, 1, MTM_U8, 600, 0, 0.5, out.data(), 4096, &got) == MTM_OK && got == 11);
            CHECK(mtm_group_comm_init(g) == MTM_OK);
        }
        // an image of a megabyte and more goes through the group's shared page-locked staging buffer: every worker copies
        // its slice of the rows (strided and contiguous sources), waits for the others, searches from the buffer
        if (nd > 1) {
            const int rows = 1030, cols = 1100;
            for (int64_t stride : {(int64_t)cols, (int64_t)cols + 52}) {
                std::vector<uint8_t> img((size_t)rows * (size_t)stride, 7);
                for (int job = 0; job < 40; ++job) {
                    const int n = 1 + (int)(rng() % 12);
                    std::vector<mtm_templ> t((size_t)n);
                    long long expect = 0;
                    for (int i = 0; i < n; ++i) {
                        std::memset(&t[i], 0, sizeof(mtm_templ));
                        t[i].px = img.data();
                        t[i].rows = 1 + (int)(rng() % 40);
                        t[i].cols = 14 + (int)(rng() % 30);
                        expect += t[i].rows % 7;
                    }
                    std::vector<mtm_hit> out(4096);
                    int64_t got = -1;
                    CHECK(mtm_group_find_matches(g, t.data(), n, 5, img.data(), rows, cols, 1, MTM_U8, stride, 0, 0.5, out.data(), 4096,
                                                 &got) == MTM_OK && got == expect);
                }
            }
        }
        mtm_group_destroy(g);
        CHECK(g_live_ctx.load() == 0);
    }
    mtm_group* bad = nullptr;
    const int neg = -1;
    CHECK(mtm_group_create(&bad, &neg, 1) == MTM_E_NO_DEVICE && bad == nullptr && g_live_ctx.load() == 0);
}

static void test_host(std::mt19937& rng) {
    std::uniform_real_distribution<float> uf(0.f, 1.f);
    for (int rep = 0; rep < 300; ++rep) {
        const int n = (int)(rng() % 600);
        std::vector<mtm_hit> hits((size_t)n);
        for (auto& h : hits) {
            h.templ_idx = (int)(rng() % 5);
            h.x = (int)(rng() % 900);
            h.y = (int)(rng() % 700);
            h.w = 1 + (int)(rng() % 90);
            h.h = 1 + (int)(rng() % 90);
            h.score = rep % 11 == 0 ? 0.5f : uf(rng);               // all-equal scores: the stable-sort paths
            if (rep % 17 == 0 && (rng() % 9) == 0) h.score = NAN;
        }
        std::vector<int32_t> keep((size_t)std::max(n, 1));
        int64_t nk = -1;
        CHECK(mtm_nms(hits.data(), n, uf(rng), rep & 1, rep % 5 == 0 ? 3 : -1, uf(rng), keep.data(), &nk) == MTM_OK);
        CHECK(nk >= 0 && nk <= n);
        for (int64_t i = 0; i < nk; ++i) CHECK(keep[(size_t)i] >= 0 && keep[(size_t)i] < n);
        std::vector<mtm_hit> s = hits;
        sort_hits(s, (rep & 1) != 0);
        CHECK(s.size() == hits.size());
        for (size_t i = 1; i < s.size(); ++i) CHECK(s[i - 1].templ_idx <= s[i].templ_idx);
        // 1-D peaks on lines with plateaus and NaNs at the ends
        const int len = 1 + (int)(rng() % 300);
        std::vector<float> line((size_t)len);
        for (auto& v : line) v = (float)(rng() % 7) * 0.1f;
        const std::vector<int> pk = find_peaks_1d(line.data(), len, 1, 0.25f, (rep & 2) != 0);
        for (int p : pk) CHECK(p > 0 && p < len - 1);
        // line_map_peaks: the 1x1 rule and find_peaks_1d restated, in both orientations and both modes
        for (int orient = 0; orient < 2; ++orient) {
            const bool mode_min = (rep & 4) != 0;
            const float thr = mode_min ? 0.35f : 0.25f;
            const int oh = orient ? len : 1, ow = orient ? 1 : len;
            std::vector<int> expect;
            if (len == 1) {
                if ((mode_min ? -line[0] : line[0]) >= (mode_min ? -thr : thr)) expect.push_back(0);
            } else {
                expect = find_peaks_1d(line.data(), len, 1, mode_min ? -thr : thr, mode_min);
            }
            std::vector<mtm_hit> recs(1);
            recs[0].templ_idx = -1;
            line_map_peaks(line.data(), oh, ow, thr, mode_min, 3, 7, 9, recs);
            CHECK(recs.size() == 1 + expect.size() && recs[0].templ_idx == -1);
            for (size_t i = 0; i < expect.size(); ++i) {
                const mtm_hit& r = recs[1 + i];
                CHECK(r.templ_idx == 3 && r.w == 7 && r.h == 9 && r.x == (orient ? 0 : expect[i]) &&
                      r.y == (orient ? expect[i] : 0) && std::memcmp(&r.score, &line[(size_t)expect[i]], 4) == 0);
            }
        }
        // extremum keys: both encodings round-trip through a host restatement of mf_float_order (-0 -> +0)
        {
            auto float_order = [](float v) {
                if (v == 0.0f) v = 0.0f;
                uint32_t b;
                std::memcpy(&b, &v, 4);
                return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
            };
            const float specials[] = {-0.0f, 0.0f, INFINITY, -INFINITY, 1e-40f, -3.5f};
            const bool mode_min = (rep & 1) != 0;
            const int ow = 1 + (int)(rng() % 500), oh = 1 + (int)(rng() % 500);
            const uint32_t idx = (uint32_t)(rng() % ((uint32_t)ow * (uint32_t)oh));
            const float v = rep % 3 == 0 ? specials[rep / 3 % 6] : (uf(rng) - 0.5f) * 1e3f;
            const float vn = v + 0.0f;
            // (a) extremum_kernel: the max key over the score, the min key over the complemented order
            const uint32_t oa = mode_min ? ~float_order(v) : float_order(v);
            const unsigned long long ka = ((unsigned long long)oa << 32) | (0xFFFFFFFFull - idx);
            mtm_hit a = decode_extremum_key(ka, mode_min, 2, ow, 5, 6);
            CHECK(a.templ_idx == 2 && a.w == 5 && a.h == 6 && a.x == (int)(idx % ow) && a.y == (int)(idx / ow) &&
                  std::memcmp(&a.score, &vn, 4) == 0);
            CHECK(order_to_float(float_order(v)) == v && std::signbit(order_to_float(float_order(v))) == std::signbit(vn));
            a = decode_extremum_key(0ull, mode_min, 2, ow, 5, 6);
            CHECK(a.x == 0 && a.y == 0 && a.score != a.score);
            // (b) the window kernels: the key over the quality
            const unsigned long long kb = ((unsigned long long)float_order(mode_min ? -v : v) << 32) | (0xFFFFFFFFull - idx);
            mtm_hit b = decode_quality_key(kb, mode_min, 4, ow, 5, 6);
            CHECK(b.templ_idx == 4 && b.x == (int)(idx % ow) && b.y == (int)(idx / ow) && std::memcmp(&b.score, &vn, 4) == 0);
            b = decode_quality_key(0ull, mode_min, 4, ow, 5, 6);
            CHECK(b.x == (int)(0xFFFFFFFFu % (uint32_t)ow) && b.y == (int)(0xFFFFFFFFu / (uint32_t)ow) && b.score != b.score);
        }
        // publish_hits / copy_out_hits below, at and above the number of hits
        {
            const int64_t cap = n == 0 ? (int64_t)(rng() % 2) : (int64_t)n - 1 + (int64_t)(rng() % 3);
            std::vector<mtm_hit> res = hits, last(3), out((size_t)std::max<int64_t>(cap, 1));
            int64_t n_out = -1;
            const int rc = publish_hits(res, last, out.data(), cap, &n_out, "sanitize: too small");
            CHECK(n_out == n && last.size() == hits.size() && res.size() == 3);
            CHECK(last.empty() || std::memcmp(last.data(), hits.data(), sizeof(mtm_hit) * hits.size()) == 0);
            if (n > cap) {
                CHECK(rc == MTM_E_OVERFLOW && std::strcmp(mtm_last_error(), "sanitize: too small") == 0);
            } else {
                CHECK(rc == MTM_OK && (n == 0 || std::memcmp(out.data(), hits.data(), sizeof(mtm_hit) * (size_t)n) == 0));
            }
            std::vector<mtm_hit> all((size_t)std::max(n, 1));
            CHECK(copy_out_hits(last, all.data(), n, &n_out, "unused") == MTM_OK && n_out == n);
        }
        // template constants from pixels and from sums agree in size and do not read out of bounds
        const int th = 1 + (int)(rng() % 20), tw = 1 + (int)(rng() % 20), tc = 1 + (int)(rng() % 3);
        std::vector<double> px((size_t)th * tw * tc), mk((size_t)th * tw * tc);
        for (auto& v : px) v = (double)(rng() % 256);
        for (auto& v : mk) v = (double)(rng() % 2);
        for (int method = 0; method < 6; ++method) {
            const TemplStats a = compute_templ_stats(px.data(), nullptr, th, tw, tc, method, true);
            const TemplStats b = compute_templ_stats(px.data(), mk.data(), th, tw, tc, method, true);
            CHECK(a.inv_area > 0.0 && b.templ2_mask2_sum >= 0.0);
        }
    }
    // the device's NMS is built from two decisions (mtm_nms_core.h): "a precedes b" and "a suppresses b".  Greedy NMS written
    // with them, over hit lists in the order mtm_find_matches returns (sort_hits), must select what mtm_nms selects - ties in
    // the transformed score (few distinct scores, several templates), maxima and minima methods, every overlap threshold
    for (int rep = 0; rep < 200; ++rep) {
        const int n = 2 + (int)(rng() % 400), asc = rep & 1;
        std::vector<mtm_hit> hits((size_t)n);
        for (auto& h : hits) {
            h.templ_idx = (int)(rng() % 4);
            h.w = 20 + 10 * (h.templ_idx & 1);
            h.h = 24;
            h.x = (int)(rng() % 160);
            h.y = (int)(rng() % 120);
            h.score = rep % 3 == 0 ? 0.25f * (float)(rng() % 5) : uf(rng);
        }
        // (a pixel is listed once per template)
        std::sort(hits.begin(), hits.end(), [](const mtm_hit& a, const mtm_hit& b) {
            return std::tie(a.templ_idx, a.y, a.x) < std::tie(b.templ_idx, b.y, b.x); });
        hits.erase(std::unique(hits.begin(), hits.end(), [](const mtm_hit& a, const mtm_hit& b) {
            return a.templ_idx == b.templ_idx && a.y == b.y && a.x == b.x; }), hits.end());
        sort_hits(hits, asc != 0);
        const double thr = 0.1 * (double)(rng() % 8), ov = 0.1 * (double)(rng() % 11);
        std::vector<int32_t> keep(hits.size());
        int64_t nk = 0;
        CHECK(mtm_nms(hits.data(), (int64_t)hits.size(), thr, asc, -1, ov, keep.data(), &nk) == MTM_OK);
        std::vector<int> order;
        const float thr_s = (float)(asc ? 1.0 - thr : thr);
        for (int i = 0; i < (int)hits.size(); ++i)
            if (nms_score(hits[(size_t)i], asc) > thr_s) order.push_back(i);
        std::sort(order.begin(), order.end(), [&](int a, int b) { return nms_earlier(hits[(size_t)a], hits[(size_t)b], asc); });
        std::vector<int> kept;
        for (int i : order) {
            bool ok = true;
            for (int k : kept) ok = ok && nms_rect_overlap(hits[(size_t)i], hits[(size_t)k]) <= (float)ov;
            if (ok) kept.push_back(i);
        }
        CHECK((int64_t)kept.size() == nk);
        for (size_t i = 0; i < kept.size(); ++i) CHECK(kept[i] == keep[i]);
        // nms_select (mtm_find_matches_image_nms): the same hits in the same order from the list in ANY order
        std::vector<mtm_hit> shuffled = hits;
        std::shuffle(shuffled.begin(), shuffled.end(), rng);
        std::vector<int32_t> sel;
        nms_select(shuffled.data(), (int64_t)shuffled.size(), asc, thr_s, (float)ov, sel);
        CHECK((int64_t)sel.size() == nk);
        for (size_t i = 0; i < sel.size(); ++i)
            CHECK(std::memcmp(&shuffled[(size_t)sel[i]], &hits[(size_t)keep[i]], sizeof(mtm_hit)) == 0);
        // ... and what the device does first (mtm_k_nms.hip.h): "champions" - candidates no earlier candidate overlaps
        // beyond the limit - are kept for certain, what a champion overlaps beyond the limit is dropped; the selection from
        // [champions | undecided rest], champions untested, is the same again
        std::vector<mtm_hit> champs, rest;
        std::vector<char> is_champ(hits.size(), 0), doomed(hits.size(), 0);
        for (int i : order) {
            bool c = true;
            for (int k : order) {
                if (k == i) break;                              // `order` is sorted: everything before i is earlier
                if (nms_rect_overlap(hits[(size_t)i], hits[(size_t)k]) > (float)ov) { c = false; break; }
            }
            is_champ[(size_t)i] = c;
        }
        for (int i : order)
            for (int k : order)
                if (is_champ[(size_t)k] && k != i && nms_rect_overlap(hits[(size_t)i], hits[(size_t)k]) > (float)ov) doomed[(size_t)i] = 1;
        for (int i : order) {
            if (is_champ[(size_t)i]) champs.push_back(hits[(size_t)i]);
            else if (!doomed[(size_t)i]) rest.push_back(hits[(size_t)i]);
        }
        if (ov >= 0.0) {
            std::vector<mtm_hit> pruned = champs;
            std::shuffle(rest.begin(), rest.end(), rng);
            pruned.insert(pruned.end(), rest.begin(), rest.end());
            nms_select(pruned.data(), (int64_t)pruned.size(), asc, thr_s, (float)ov, sel, (int64_t)champs.size());
            CHECK((int64_t)sel.size() == nk);
            for (size_t i = 0; i < sel.size(); ++i)
                CHECK(std::memcmp(&pruned[(size_t)sel[i]], &hits[(size_t)keep[i]], sizeof(mtm_hit)) == 0);
        }
    }
    // byte-run sums (the SSE2 pass over fresh template bytes): exact at every length and alignment, incl. all-255 runs
    // long enough to wrap a 32-bit lane if the block length were wrong
    std::vector<uint8_t> bytes((size_t)(16 * 8192 * 3 + 77));
    for (int rep = 0; rep < 40; ++rep) {
        for (auto& v : bytes) v = rep == 0 ? 255 : (uint8_t)(rng() & 255);
        const size_t off = rep == 0 ? 0 : rng() % 33, n = rep < 2 ? bytes.size() - off : rng() % 5000;
        unsigned long long s = 7, q = 9, rs = 7, rq = 9;
        u8_run_sums(bytes.data() + off, n, &s, &q);
        for (size_t i = 0; i < n; ++i) {
            rs += bytes[off + i];
            rq += (unsigned long long)bytes[off + i] * bytes[off + i];
        }
        CHECK(s == rs && q == rq);
    }
    int64_t nk = 0;
    CHECK(mtm_nms(nullptr, 5, 0.5, 0, -1, 0.5, nullptr, &nk) == MTM_E_INVALID && std::strlen(mtm_last_error()) > 0);
}

// ---- the grid of the device's NMS (mtm_nms_core.h: nms_grid; the cell rule as nms_cell_of, mtm_k_nms.hip.h, applies it) ----
// Boxes inside the image with sides <= max_side: any two that intersect are filed at most one cell apart in each axis (the
// 3 x 3 neighbourhood holds every partner), and every index the kernels form - cell_cnt[c + dy * gw - 1] and
// cell_cnt[c + dy * gw + 2], dy = -1 .. 1 - lies in [0, gw * gh] (cell_cnt has gw * gh + 1 words).
static void test_nms_grid(std::mt19937& rng) {
    const auto cell_xy = [](const NmsGrid& g, const mtm_hit& h, int* cx, int* cy) {
        *cx = std::min(std::max(h.x / g.cell, 0), g.gw - 3) + 1;
        *cy = std::min(std::max(h.y / g.cell, 0), g.gh - 3) + 1;
    };
    CHECK(nms_grid(300, 640, 0).cell == 32 && nms_grid(300, 640, 32).gw == 23 && nms_grid(300, 640, 32).gh == 12);
    CHECK(nms_grid(300, 640, 48).cell == 48 && nms_grid(300, 640, 48).gw == 16 && nms_grid(300, 640, 48).gh == 9);
    for (int rep = 0; rep < 400; ++rep) {
        const int max_side = rep % 7 == 0 ? 1 + (int)(rng() % 31) : 1 + (int)(rng() % 300);
        // (images narrower than a cell, sides at and next to multiples of the cell)
        int rows = 1 + (int)(rng() % 2000), cols = 1 + (int)(rng() % 2000);
        const int cell0 = std::max(32, max_side);
        if (rep % 5 == 1) cols = cell0 * (1 + (int)(rng() % 6)) + (int)(rng() % 3) - 1;
        if (rep % 5 == 2) rows = cell0 * (1 + (int)(rng() % 6)) + (int)(rng() % 3) - 1;
        const NmsGrid g = nms_grid(rows, cols, max_side);
        CHECK(g.cell == cell0 && g.gw == cols / g.cell + 3 && g.gh == rows / g.cell + 3);
        std::vector<mtm_hit> hits(64);
        for (size_t i = 0; i < hits.size(); ++i) {
            mtm_hit& h = hits[i];
            h.w = 1 + (int)(rng() % (unsigned)std::min(max_side, cols));
            h.h = 1 + (int)(rng() % (unsigned)std::min(max_side, rows));
            if (i % 4 == 0) h.w = std::min(max_side, cols);
            if (i % 8 == 0) h.h = std::min(max_side, rows);
            // around one place (so that pairs intersect), or at the image's edges
            const int ax = (int)(rng() % (unsigned)cols), ay = (int)(rng() % (unsigned)rows);
            h.x = i < 40 ? (int)(hits[0].x * (i > 0) + (i ? (int)(rng() % (unsigned)(2 * g.cell)) - g.cell : ax)) : (i % 2 ? 0 : cols);
            h.y = i < 40 ? (int)(hits[0].y * (i > 0) + (i ? (int)(rng() % (unsigned)(2 * g.cell)) - g.cell : ay)) : (i % 3 ? 0 : rows);
            h.x = std::min(std::max(h.x, 0), cols - h.w);
            h.y = std::min(std::max(h.y, 0), rows - h.h);
            h.templ_idx = 0;
            h.score = 1.0f;
        }
        int pairs = 0;
        for (const mtm_hit& a : hits) {
            int ax, ay;
            cell_xy(g, a, &ax, &ay);
            CHECK(ax >= 1 && ax <= g.gw - 2 && ay >= 1 && ay <= g.gh - 2);
            const int c = ay * g.gw + ax;
            for (int dy = -1; dy <= 1; ++dy)
                CHECK(c + dy * g.gw - 1 >= 0 && c + dy * g.gw + 2 <= g.gw * g.gh);
            for (const mtm_hit& b : hits) {
                if (nms_rect_overlap(a, b) <= 0.0f) continue;
                int bx, by;
                cell_xy(g, b, &bx, &by);
                CHECK(std::abs(ax - bx) <= 1 && std::abs(ay - by) <= 1);
                ++pairs;
            }
        }
        CHECK(pairs > (int)hits.size());        // (more than every box with itself)
    }
}

// ---- the sizing rules of the peak pass (mtm_peak_sizing.h), one check per rule --------------------------------------------
static void test_peak_sizing(std::mt19937& rng) {
    CHECK(map_pitch_of(1) == 4 && map_pitch_of(4) == 4 && map_pitch_of(5) == 8 && map_pitch_of(513) == 516);
    CHECK(peak_grid_dims(130, 513, 33, kPkRows).x == 3 && peak_grid_dims(130, 513, 33, kPkRows).y == 2 &&
          peak_grid_dims(130, 513, 33, kPkRows).z == 33 && peak_grid_dims(130, 513, 33, kPkSparseRows).y == 5);
    CHECK(peak_list_cap(2048, 4) == 256 && peak_list_cap(1 << 20, 4) == (1 << 17) && verify_blocks(1) == 1 && verify_blocks(257) == 2);
    CHECK(cand_hash_slots(1) == 1024 && cand_hash_slots(512) == 1024 && cand_hash_slots(513) == 2048);
    CHECK(extremum_blocks() == 256 && extremum_batch_blocks(1) == 1 && extremum_batch_blocks(4097) == 2);
    for (int rep = 0; rep < 2000; ++rep) {
        // the grid covers every pixel of the largest map: the last strip holds its last row and column, no strip is empty
        const int max_oh = 1 + (int)(rng() % (rep % 3 ? 300u : 65535u)), max_ow = 1 + (int)(rng() % (rep % 3 ? 1100u : 65535u));
        const int n_maps = 1 + (int)(rng() % 4096u);
        for (int strip_rows : {kPkRows, kPkSparseRows}) {
            const PeakGrid g = peak_grid_dims(max_oh, max_ow, n_maps, strip_rows);
            CHECK((long long)g.x * kPkCols >= max_ow && (long long)(g.x - 1) * kPkCols < max_ow);
            CHECK((long long)g.y * 4 * strip_rows >= max_oh && (long long)(g.y - 1) * 4 * strip_rows < max_oh);
            CHECK(g.z == (unsigned)n_maps && g.y <= 65535u && g.z <= 65535u);
        }
        // the lists: within 64 MB all together, or at the floor of 256 records; never more than an eighth of the capacity
        // unless at the floor
        const unsigned long long hit_cap = rep % 4 == 0 ? 1 + rng() % 4096u : 1 + (((unsigned long long)rng() << 8) % (1ull << 26));
        const unsigned long long n_lists = 1 + rng() % (rep % 5 == 0 ? 4096u : 200u);
        const unsigned long long cap_t = peak_list_cap(hit_cap, n_lists);
        CHECK(cap_t >= 256 && (cap_t == 256 || (cap_t * n_lists * sizeof(mtm_hit) <= (64ull << 20) && cap_t <= hit_cap / 8)));
        CHECK(cap_t == 256 || cap_t == hit_cap / 8 || cap_t == (64ull << 20) / sizeof(mtm_hit) / n_lists);
        // the verifiers: one thread per record of a candidate list of min(hit_cap, 4096 * 256) records
        const long long hc = (long long)hit_cap, cand_cap = std::min<long long>(hc, 4096ll * 256);
        CHECK((long long)verify_blocks(hc) * 256 >= cand_cap && verify_blocks(hc) <= 4096u && verify_blocks(hc) >= 1u);
        CHECK(((long long)verify_blocks(hc) - 1) * 256 < hc);
        // the table: a power of two, at least 1024 slots and twice the list; the keys are what is cleared, the values follow
        const size_t hsz = cand_hash_slots(cand_cap);
        CHECK((hsz & (hsz - 1)) == 0 && hsz >= 1024 && hsz >= 2 * (size_t)cand_cap && (hsz == 1024 || hsz / 2 < 2 * (size_t)cand_cap));
        const unsigned mask = (unsigned)(hsz - 1);
        CHECK(cand_hash_key_bytes(mask) == hsz * 8 && cand_hash_bytes(mask) == hsz * 12);
        // the extremum launches: at least one work-group, at most 256, one pixel per thread until then
        const long long px = 1 + (long long)(rng() % (rep % 2 ? 5000u : 4000000u));
        const int nb = extremum_batch_blocks(px);
        CHECK(nb >= 1 && nb <= 256 && (nb == 256 || (long long)nb * 4096 >= px));
    }
}

// ---- which kernel chain makes a class's window statistics (mtm_stats_route.h): every boundary of the rule, and for the route
// it names the preconditions of that route's kernels (mtm_k_stats.hip.h), restated here in integer arithmetic
static bool route_kernels_fit(int route, int dtype, int chans, int h, int w, int cols) {
    const unsigned long long area = (unsigned long long)w * (unsigned long long)h, two32 = 1ull << 32;
    const int owg = (1024 + 1 - w) & ~15;       // stats_u8_owg: output columns of a 1024-column strip
    const bool strip_ok = w <= 768 && owg >= 256 && owg % 16 == 0 && owg + w - 1 <= 1024;
    switch (route) {
    case kStatsRouteU8:      // uint32 prefixes of I and I^2 over a strip: every window sum below 2^32
        return dtype == MTM_U8 && chans == 1 && strip_ok && area * 255ull * 255ull < two32;
    case kStatsRouteU8MC:    // ... the squares of all three channels in one prefix
        return dtype == MTM_U8 && chans == 3 && strip_ok && 3ull * area * 255ull * 255ull < two32;
    case kStatsRouteU16:     // ... of I only (the squares are uint64)
        return dtype == MTM_U16 && chans == 1 && strip_ok && area * 65535ull < two32;
    case kStatsRouteU8TwoPass:       // two uint32 prefix rows of cols + 1 words in 64 KB of dynamic LDS; uint32 row sums of I^2
        return dtype == MTM_U8 && 2ull * 4ull * (unsigned long long)(cols + 1) <= 65536ull && (unsigned long long)w * 65025ull < two32;
    case kStatsRouteU8TwoPassWide:
        return dtype == MTM_U8 && (unsigned long long)w * 65025ull < two32;
    case kStatsRouteF64Lds: {       // 256 * 16 + w floats of a row, one pad word per 16, in 64 KB
        const long long n = 256 * 16 + w, words = n + n / 16 + 2;
        return w <= 1024 && 4 * words <= 65536;
    }
    case kStatsRouteF64:
        return true;
    default:
        return false;
    }
}

static void test_stats_route() {
    std::vector<int> ws = {1, 2, 16, 64, 65, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 4096, 16384};
    const int cols_set[] = {8190, 8191, 8192, 16384};
    const double limits[] = {4294967295.0 / 65025.0, 4294967295.0 / (3.0 * 65025.0), 4294967295.0 / 65535.0};
    int seen[kStatsRouteCount] = {0};
    for (int dtype : {MTM_U8, MTM_F32, MTM_U16})
        for (int chans = 1; chans <= 4; ++chans)
            for (int fuse = 0; fuse <= 1; ++fuse)
                for (int w : ws) {
                    std::vector<int> hs = {1, 2, 8, 255, 256, 257, 16384};
                    for (double lim : limits) {         // the three area limits: one below, at, one above
                        const int h_at = (int)std::min(16384.0, std::floor(lim / w));
                        for (int d = -1; d <= 1; ++d)
                            if (h_at + d >= 1 && h_at + d <= 16384) hs.push_back(h_at + d);
                    }
                    for (int h : hs)
                        for (int cols : cols_set) {
                            if (cols < w) continue;
                            const StatsRoute r = stats_route(dtype, chans, h, w, cols, fuse != 0);
                            seen[r]++;
                            CHECK(route_kernels_fit(r, dtype, chans, h, w, cols));
                            CHECK(stats_route_refusal(r, dtype, chans, h, w, cols) == nullptr);
                            // a fused kernel is chosen wherever it fits and the option is on; never with the option off
                            const int fused = dtype == MTM_U8 && chans == 1 ? kStatsRouteU8 : dtype == MTM_U8 && chans == 3 ? kStatsRouteU8MC
                                            : dtype == MTM_U16 && chans == 1 ? kStatsRouteU16 : -1;
                            const bool fits = fused >= 0 && route_kernels_fit(fused, dtype, chans, h, w, cols);
                            CHECK((r == fused) == (fits && fuse != 0));
                            if (r != fused) {
                                if (dtype == MTM_U8) CHECK(r == (cols <= 8191 ? kStatsRouteU8TwoPass : kStatsRouteU8TwoPassWide));
                                else CHECK(r == (w <= 1024 ? kStatsRouteF64Lds : kStatsRouteF64));
                            }
                            // a forced route (the test-support entry) is admitted only where its kernels fit
                            for (int f = 0; f < kStatsRouteCount; ++f)
                                if (stats_route_refusal(f, dtype, chans, h, w, cols) == nullptr)
                                    CHECK(route_kernels_fit(f, dtype, chans, h, w, cols));
                        }
                }
    for (int r = 0; r < kStatsRouteCount; ++r) CHECK(seen[r] > 0);
    CHECK(stats_route_refusal(kStatsRouteCount, MTM_U8, 1, 8, 8, 64) != nullptr && stats_route_refusal(-1, MTM_U8, 1, 8, 8, 64) != nullptr);
    // the boundaries by name
    CHECK(stats_route(MTM_U8, 1, 86, 768, 900, true) == kStatsRouteU8 && stats_route(MTM_U8, 1, 87, 768, 900, true) == kStatsRouteU8TwoPass);
    CHECK(stats_route(MTM_U8, 1, 8, 769, 900, true) == kStatsRouteU8TwoPass && stats_route(MTM_U8, 1, 8, 8, 900, false) == kStatsRouteU8TwoPass);
    CHECK(stats_route(MTM_U8, 3, 28, 768, 900, true) == kStatsRouteU8MC && stats_route(MTM_U8, 3, 29, 768, 900, true) == kStatsRouteU8TwoPass);
    CHECK(stats_route(MTM_U8, 3, 86, 256, 900, true) == kStatsRouteU8MC && stats_route(MTM_U8, 3, 87, 256, 900, true) == kStatsRouteU8TwoPass);
    CHECK(stats_route(MTM_U8, 2, 8, 8, 8191, true) == kStatsRouteU8TwoPass && stats_route(MTM_U8, 2, 8, 8, 8192, true) == kStatsRouteU8TwoPassWide);
    CHECK(stats_route(MTM_U16, 1, 256, 256, 900, true) == kStatsRouteU16 && stats_route(MTM_U16, 1, 255, 257, 900, true) == kStatsRouteU16);
    CHECK(stats_route(MTM_U16, 1, 256, 257, 900, true) == kStatsRouteF64Lds && stats_route(MTM_U16, 1, 8, 8, 900, false) == kStatsRouteF64Lds);
    CHECK(stats_route(MTM_F32, 1, 8, 1024, 2000, true) == kStatsRouteF64Lds && stats_route(MTM_F32, 1, 8, 1025, 2000, true) == kStatsRouteF64);
}

// ---- what a class's score kernel reads of the window statistics (stat_wants, mtm_stats_route.h), against what the consumers
// need, stated per consumer: the masked float64 / naive / dot4 kernels and TM_CCORR off the matrix cores read no plane; the
// numerator needs the window sums for the centred methods, the sum of squares for the two SQDIFF ones and plain TM_CCORR; the
// matrix-core epilogues undo their operands' bias with the window sums whatever the method; a masked class on the int8 cores
// takes its sum2 from the sum I^2 M pass and normalises there; the reciprocal plane is the row-multiplexed epilogue's; the
// block records are the single-channel hits-only screens'
static void test_stat_wants() {
    const int methods[] = {MTM_TM_SQDIFF, MTM_TM_SQDIFF_NORMED, MTM_TM_CCORR, MTM_TM_CCORR_NORMED, MTM_TM_CCOEFF, MTM_TM_CCOEFF_NORMED};
    const int kernels[] = {MTM_KERNEL_AUTO, MTM_KERNEL_NAIVE, MTM_KERNEL_DOT4, MTM_KERNEL_MFMA, MTM_KERNEL_MFMA16, MTM_KERNEL_MFMA_F32};
    long long n = 0, n_none = 0, n_blk = 0, n_rsq = 0;
    for (int method : methods)
        for (int kernel : kernels)
            for (int masked = 0; masked <= 1; ++masked)
                for (int mask_rm = 0; mask_rm <= 1; ++mask_rm)
                    for (int r2 : {0, 1, 2})
                        for (int rm_R : {0, 2, 16})
                            for (int chans = 1; chans <= 4; ++chans)
                                for (int dtype : {MTM_U8, MTM_F32, MTM_U16}) {
                                    const StatWants s = stat_wants(method, kernel, masked != 0, mask_rm != 0, r2, rm_R, chans, dtype);
                                    ++n;
                                    const bool cores = kernel == MTM_KERNEL_MFMA || kernel == MTM_KERNEL_MFMA16 || kernel == MTM_KERNEL_MFMA_F32;
                                    const bool mm = masked && kernel == MTM_KERNEL_MFMA;
                                    const bool normed_method = method == MTM_TM_SQDIFF_NORMED || method == MTM_TM_CCORR_NORMED || method == MTM_TM_CCOEFF_NORMED;
                                    const bool ccoeff = method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED;
                                    CHECK(s.masked_mfma == mm);
                                    CHECK(s.none == ((masked && kernel != MTM_KERNEL_MFMA) || (method == MTM_TM_CCORR && !cores)));
                                    CHECK(s.num_type == ((mm || method == MTM_TM_CCORR_NORMED) ? 0 : ccoeff ? 1 : 2));
                                    CHECK(s.normed == (normed_method && !mm));
                                    CHECK(s.want_t == (s.num_type == 1 || cores));
                                    if (mm) CHECK(!s.want_sum2);
                                    else if (s.num_type == 2 || (s.normed && s.num_type != 1) || !cores) CHECK(s.want_sum2);
                                    // ... and off where nothing reads the plane: a centred method on the matrix cores (the
                                    // numerator takes the window sums, the norm comes from the sqrt plane)
                                    else CHECK(!s.want_sum2);
                                    if (s.rsq) CHECK(rm_R > 0 && s.normed);
                                    if (s.blk) CHECK(chans == 1);
                                    if (s.blk && mm) CHECK(method == MTM_TM_CCORR_NORMED && rm_R > 0);
                                    // the mask's row-multiplexed pack chooses the kernel of the sum I^2 M pass, nothing here
                                    const StatWants t = stat_wants(method, kernel, masked != 0, mask_rm == 0, r2, rm_R, chans, dtype);
                                    CHECK(s.none == t.none && s.masked_mfma == t.masked_mfma && s.num_type == t.num_type && s.normed == t.normed &&
                                          s.want_t == t.want_t && s.want_sum2 == t.want_sum2 && s.rsq == t.rsq && s.blk == t.blk);
                                    n_none += s.none, n_blk += s.blk, n_rsq += s.rsq;
                                }
    CHECK(n == 6 * 6 * 2 * 2 * 3 * 3 * 4 * 3 && n_none > 0 && n_none < n && n_blk > 0 && n_rsq > 0);
}

// ---- the host-only pieces of fm_end (mtm_api.hip; its peak pass: mtm_peaks.hip): the 3x3 test of the candidate list, the trivial-map rule, the ladder

// one case of verify_candidates_3x3 against brute force over the maps: `maps[t]` the scores of an oh[t] x ow[t] map, the list
// every pixel whose quality exceeds thr_q, shuffled; the scratch vectors come from the caller as they are
static void verify_case(const std::vector<int>& oh, const std::vector<int>& ow, const std::vector<std::vector<float>>& maps,
                        bool mode_min, float thr_q, float padv, std::mt19937& rng, std::vector<unsigned long long>& hk,
                        std::vector<int>& hv) {
    const int nt = (int)maps.size();
    auto q = [&](int t, int y, int x) { return mode_min ? -maps[(size_t)t][(size_t)y * ow[(size_t)t] + x] : maps[(size_t)t][(size_t)y * ow[(size_t)t] + x]; };
    std::vector<mtm_hit> list;
    std::vector<std::tuple<int, int, int>> expect;
    std::vector<int> expect_n((size_t)nt, 0);
    for (int t = 0; t < nt; ++t)
        for (int y = 0; y < oh[(size_t)t]; ++y)
            for (int x = 0; x < ow[(size_t)t]; ++x) {
                const float v = q(t, y, x);
                if (!(v > thr_q)) continue;
                mtm_hit h{t, x, y, 7 + t, 9 + t, maps[(size_t)t][(size_t)y * ow[(size_t)t] + x]};
                list.push_back(h);
                bool peak = true;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (!dy && !dx) continue;
                        const int yy = y + dy, xx = x + dx;
                        const bool inside = yy >= 0 && yy < oh[(size_t)t] && xx >= 0 && xx < ow[(size_t)t];
                        peak = peak && v >= (inside ? q(t, yy, xx) : padv);
                    }
                if (peak) {
                    expect.emplace_back(t, y, x);
                    ++expect_n[(size_t)t];
                }
            }
    std::shuffle(list.begin(), list.end(), rng);
    mtm_hit sentinel{};
    sentinel.templ_idx = -7;
    std::vector<mtm_hit> hits(1, sentinel);         // (hits are appended)
    std::vector<int> tflags((size_t)nt, 0);
    verify_candidates_3x3(list.data(), list.size(), MapDims{oh.data(), ow.data(), sizeof(int)}, mode_min, thr_q, padv, hk, hv, hits,
                          tflags.data());
    CHECK(hits[0].templ_idx == -7 && hits.size() == 1 + expect.size());
    std::vector<std::tuple<int, int, int>> got;
    for (size_t i = 1; i < hits.size(); ++i) {
        const mtm_hit& h = hits[i];
        CHECK(h.templ_idx >= 0 && h.templ_idx < nt && h.w == 7 + h.templ_idx && h.h == 9 + h.templ_idx);
        CHECK(std::memcmp(&h.score, &maps[(size_t)h.templ_idx][(size_t)h.y * ow[(size_t)h.templ_idx] + h.x], 4) == 0);
        got.emplace_back(h.templ_idx, h.y, h.x);
    }
    std::sort(got.begin(), got.end());
    CHECK(got == expect);                           // (expect was built in (t, y, x) order)
    for (int t = 0; t < nt; ++t) CHECK(tflags[(size_t)t] == expect_n[(size_t)t]);
}

static void test_verify_candidates(std::mt19937& rng) {
    std::vector<unsigned long long> hk;             // one pair of scratch vectors through every case, never cleared here
    std::vector<int> hv;
    for (int rep = 0; rep < 400; ++rep) {
        const int nt = 1 + (int)(rng() % 3);
        std::vector<int> oh((size_t)nt), ow((size_t)nt);
        std::vector<std::vector<float>> maps((size_t)nt);
        for (int t = 0; t < nt; ++t) {
            oh[(size_t)t] = 1 + (int)(rng() % 12);
            ow[(size_t)t] = 1 + (int)(rng() % 12);
            maps[(size_t)t].resize((size_t)oh[(size_t)t] * ow[(size_t)t]);
            for (float& v : maps[(size_t)t]) v = 0.25f * (float)(rng() % 5);          // five levels: plateaus and ties
        }
        const bool mode_min = (rep & 1) != 0;
        const float thr = 0.25f * (float)(rng() % 5) + (rng() % 3 == 0 ? -0.3f : 0.1f);
        verify_case(oh, ow, maps, mode_min, mode_min ? -thr : thr, (rep & 2) ? 0.0f : -INFINITY, rng, hk, hv);
    }
    // NaN: a NaN candidate is never a hit and never beats a neighbour (the rule of peaks_kernel: fmaxf ignores it), and it
    // keeps the template's count below oh * ow - the map is not trivial
    for (float padv : {0.0f, -INFINITY})
        for (int mode_min = 0; mode_min < 2; ++mode_min) {
            const int oh = 3, ow = 4;
            const float s = mode_min ? -1.0f : 1.0f;
            std::vector<mtm_hit> list;
            for (int y = 0; y < oh; ++y)
                for (int x = 0; x < ow; ++x) list.push_back(mtm_hit{0, x, y, 2, 2, s * 0.75f});
            list[5].score = NAN;                     // (1, 1): every other pixel has it as a neighbour or lies beside one that has
            list[0].score = s * 0.875f;              // (0, 0) beats (0, 1) and (1, 0); its NaN neighbour does not beat it
            std::shuffle(list.begin(), list.end(), rng);
            std::vector<mtm_hit> hits;
            int flag = 0;
            verify_candidates_3x3(list.data(), list.size(), MapDims{&oh, &ow, sizeof(int)}, mode_min != 0, 0.5f, padv, hk, hv, hits, &flag);
            CHECK((int)hits.size() == oh * ow - 3 && flag == oh * ow - 3 && !fused_count_trivial(flag, oh, ow));
            for (const mtm_hit& h : hits) CHECK(h.score == h.score && !(h.x == 1 && h.y == 0) && !(h.x == 0 && h.y == 1));
        }
    for (float padv : {0.0f, -INFINITY}) {
        // the empty list
        std::vector<mtm_hit> hits;
        int flag = 0;
        const int one = 5;
        verify_candidates_3x3(nullptr, 0, MapDims{&one, &one, sizeof(int)}, false, 0.5f, padv, hk, hv, hits, &flag);
        CHECK(hits.empty() && flag == 0);
        // an all-equal map above the threshold: every pixel is returned, and the fused trivial predicate says "drop"
        for (int oh : {1, 4, 12})
            for (int ow : {1, 7}) {
                std::vector<std::vector<float>> flat(1, std::vector<float>((size_t)oh * ow, 0.75f));
                verify_case({oh}, {ow}, flat, false, 0.5f, padv, rng, hk, hv);
                std::vector<mtm_hit> list;
                for (int y = 0; y < oh; ++y)
                    for (int x = 0; x < ow; ++x) list.push_back(mtm_hit{0, x, y, 3, 3, 0.75f});
                hits.clear();
                flag = 0;
                verify_candidates_3x3(list.data(), list.size(), MapDims{&oh, &ow, sizeof(int)}, false, 0.5f, padv, hk, hv, hits, &flag);
                CHECK((int)hits.size() == oh * ow && flag == oh * ow && fused_count_trivial(flag, oh, ow));
                CHECK(!fused_count_trivial(flag - 1, oh, ow));
            }
        // a hit at each corner (quality above the constant border's 0)
        {
            const int oh = 5, ow = 6;
            std::vector<std::vector<float>> m(1, std::vector<float>((size_t)oh * ow, 0.25f));
            for (int y : {0, oh - 1})
                for (int x : {0, ow - 1}) m[0][(size_t)y * ow + x] = 1.0f;
            verify_case({oh}, {ow}, m, false, 0.5f, padv, rng, hk, hv);
            hits.clear();
            flag = 0;
            const mtm_hit corners[4] = {{0, 0, 0, 2, 2, 1.0f}, {0, ow - 1, 0, 2, 2, 1.0f}, {0, 0, oh - 1, 2, 2, 1.0f}, {0, ow - 1, oh - 1, 2, 2, 1.0f}};
            verify_candidates_3x3(corners, 4, MapDims{&oh, &ow, sizeof(int)}, false, 0.5f, padv, hk, hv, hits, &flag);
            CHECK(hits.size() == 4 && flag == 4);
        }
        // one duplicated record: its first copy is what the neighbours see.  A = (1, 1) listed with 0.5, then again with 0.9;
        // B = (2, 1) with 0.7 is a hit only against the first
        {
            const int oh = 3, ow = 4;
            const mtm_hit list[3] = {{0, 1, 1, 2, 2, 0.5f}, {0, 2, 1, 2, 2, 0.7f}, {0, 1, 1, 2, 2, 0.9f}};
            hits.clear();
            flag = 0;
            verify_candidates_3x3(list, 3, MapDims{&oh, &ow, sizeof(int)}, false, 0.25f, -INFINITY, hk, hv, hits, &flag);
            bool b_hit = false, first_a_hit = false;
            for (const mtm_hit& h : hits) {
                b_hit = b_hit || (h.x == 2 && h.y == 1);
                first_a_hit = first_a_hit || (h.x == 1 && h.score == 0.5f);
            }
            CHECK(b_hit && !first_a_hit && flag == (int)hits.size());
        }
    }
    // the scans' flag word: bytes 0 / 1 / 2 zero or not, against the expression as fm_end had it; the top byte is not looked at
    for (unsigned b0 : {0u, 1u, 0x80u})
        for (unsigned b1 : {0u, 1u, 0xFFu})
            for (unsigned b2 : {0u, 2u, 0x40u})
                for (unsigned b3 : {0u, 0x7Fu}) {
                    const unsigned f = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
                    CHECK(scan_flags_trivial(f) == ((f & 0xFFu) == 0 && !((f & 0xFF00u) != 0 && (f & 0xFF0000u) != 0)));
                    CHECK(scan_flags_trivial(f) == (b0 == 0 && !(b1 != 0 && b2 != 0)));
                }
}

// Every sequence of outcomes the device can report from `R` on: rig_wide only in pp_mode and from the refined global extremum
// (an output that is not finite), cands_overflow only while fused,
// hits_overflow only when not fused (a verified list is no longer than the candidate list, whose capacity never exceeds
// hit_cap) and never right after the single list of a non-flagged full scan was grown (same maps, room for every peak).
// Pass `attempt` is about to run: it must lie within `cap`; no step but a grown list is taken twice (`seen`).
static void walk_ladder(const mtmi::CallRoute& R, int attempt, unsigned seen, bool list_holds_all, int cap, int* longest) {
    CHECK(attempt < cap);
    CHECK(!(R.refine && R.f32_exact));
    const bool local = R.mode == MTM_PEAKS_LOCAL;
    for (int rig = 0; rig <= ((local ? R.pp_mode : (R.refine && R.ext)) ? 1 : 0); ++rig)
        for (int co = 0; co <= ((local ? R.fused : (R.refine && R.ext)) ? 1 : 0); ++co)
            for (int ho = 0; ho <= (local && !R.fused && !list_holds_all ? 1 : 0); ++ho) {
                const LadderStep step = ladder_next(R, PassOutcome{rig != 0, co != 0, ho != 0}, attempt);
                if (step == LadderStep::Done) {
                    *longest = std::max(*longest, attempt + 1);
                    continue;
                }
                CHECK(rig || co || ho);
                const bool grow = step == LadderStep::GrowList || step == LadderStep::GrowListLeaveSegments;
                const unsigned bit = 1u << (unsigned)step;
                CHECK(grow || !(seen & bit));
                mtmi::CallRoute next = R;
                ladder_apply(next, step);
                walk_ladder(next, attempt + 1, seen | bit, step == LadderStep::GrowList && !R.fused && !R.sparse, cap, longest);
            }
}

static void test_ladder() {
    std::vector<mtmi::CallRoute> starts;
    mtmi::CallRoute base;
    base.n = 3;
    base.cand_cap = 16;
    for (int ho = 0; ho < 2; ++ho) {
        mtmi::CallRoute r = base;               // integer candidates
        r.fused = true;
        r.hits_only = ho != 0;
        starts.push_back(r);
        for (int np : {1, 3})
            for (int raw = 0; raw < 2; ++raw) {
                mtmi::CallRoute f = r;          // float32 refinement from kernel candidates
                f.refine = true;
                f.bf16_np = np;
                f.raw_rig = raw != 0;
                starts.push_back(f);
            }
    }
    for (int np : {1, 3}) {
        mtmi::CallRoute r = base;               // float32 refinement from a map scan, as fm_end enters its loop
        r.refine = r.refine_scan = r.pp_mode = r.fused = true;
        r.bf16_np = np;
        starts.push_back(r);
        mtmi::CallRoute g = base;               // the refined global extremum
        g.mode = MTM_PEAKS_GLOBAL;
        g.refine = g.ext = g.hits_only = true;
        g.bf16_np = np;
        starts.push_back(g);
    }
    for (int skip = 0; skip < 2; ++skip) {
        mtmi::CallRoute r = base;               // flagged segments
        r.sparse = true;
        r.seg_skip_used = skip != 0;
        starts.push_back(r);
    }
    starts.push_back(base);                     // the plain full scan
    mtmi::CallRoute f64 = base;                 // ... on the float64 kernel's maps; the global extremum without a list
    f64.f32_exact = true;
    starts.push_back(f64);
    f64.mode = MTM_PEAKS_GLOBAL;
    starts.push_back(f64);
    int worst_local = 0, worst_global = 0;
    for (const mtmi::CallRoute& r : starts) {
        const bool local = r.mode == MTM_PEAKS_LOCAL;
        walk_ladder(r, 0, 0u, false, local ? 5 : 3, local ? &worst_local : &worst_global);
    }
    // one product -> three products -> map scan -> float64 kernel -> grown list; one product -> three products -> float64 kernel
    CHECK(worst_local == 5 && worst_global == 3);
    // a step's route: the flagged segments are left with complete maps asked for, the float64 kernel ends every refinement
    mtmi::CallRoute r = base;
    r.sparse = r.seg_skip_used = r.fused = true;
    ladder_apply(r, LadderStep::GrowListLeaveSegments);
    CHECK(!r.sparse && !r.seg_skip_used && !r.fused);
    r = base;
    r.refine = r.fused = r.hits_only = r.raw_rig = true;
    ladder_apply(r, LadderStep::Float64);
    CHECK(r.f32_exact && !r.refine && !r.fused && !r.hits_only && !r.raw_rig && !r.pp_mode && !r.ext);
}

// ---- the host plan of a tracking call (plan_tracks, mtm_host.cpp): the tile tables against brute force, every error path
static int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// What plan_tracks must have laid out for valid tracks: units in set order, groups that partition each set, per group a
// row-major grid of distinct 16-aligned tiles that holds the frame-0 map and the next_box map of every possible hit.
static void check_plan(const TrackPlan& P, const std::vector<BlobTempl>& tl, int rows, int cols,
                       const std::vector<mtm_box_unit>& start, const std::vector<int32_t>& off, const std::vector<int32_t>& idx,
                       int margin, bool reacq) {
    const int n = (int)start.size();
    CHECK(P.n_units == idx.size() && P.units.size() == idx.size() && P.set_off.size() == off.size());
    CHECK(std::equal(off.begin(), off.end(), P.set_off.begin()));
    CHECK((int)P.templ_bytes.size() == n);
    size_t at = 0;              // the next tile of the table
    unsigned long long tiles_max = 0, groups_max = 0;
    for (int k = 0; k < n; ++k) {
        const mtm_box_unit& s = start[(size_t)k];
        const BlobTempl& t = tl[(size_t)s.templ_idx];
        const int h = t.rows, w = t.cols, oh0 = s.rows - h + 1, ow0 = s.cols - w + 1;
        CHECK(P.templ_bytes[(size_t)k] == (size_t)h * w * (t.dtype == MTM_U16 ? 2 : t.chans));
        for (int u = off[(size_t)k]; u < off[(size_t)k + 1]; ++u) {
            const TrackUnit& U = P.units[(size_t)u];
            CHECK(U.t == idx[(size_t)u] && U.y0 == s.y0 && U.x0 == s.x0 && U.oh == oh0 && U.ow == ow0);
        }
        // the largest map of the call, by brute force: frame 0's, and MTM.tracking.next_box around every hit of the frame
        int need_h = oh0, need_w = ow0;
        for (int y = 0; y <= rows - h; ++y)
            need_h = std::max(need_h, std::min(rows, y + h + margin) - std::max(0, y - margin) - h + 1);
        for (int x = 0; x <= cols - w; ++x)
            need_w = std::max(need_w, std::min(cols, x + w + margin) - std::max(0, x - margin) - w + 1);
        const int ty_n = cdiv(need_h, 16), tx_n = cdiv(need_w, 16);
        int u_next = off[(size_t)k];
        while (u_next < off[(size_t)k + 1]) {           // one group: its tiles are a ty_n x tx_n grid, row-major
            CHECK(at < P.tiles.size());
            const int u0 = P.tiles[at].u0, nv = P.tiles[at].nv;
            CHECK(u0 == u_next && nv >= 1 && nv <= kTrackNV && nv == std::min(kTrackNV, off[(size_t)k + 1] - u0));
            for (int ty = 0; ty < ty_n; ++ty)
                for (int tx = 0; tx < tx_n; ++tx, ++at) {
                    CHECK(at < P.tiles.size());
                    const TrackTile& K = P.tiles[at];
                    CHECK(K.u0 == u0 && K.nv == nv && K.ty0 == 16 * ty && K.tx0 == 16 * tx);
                }
            u_next += nv;
        }
        CHECK(u_next == off[(size_t)k + 1]);
        tiles_max = std::max(tiles_max,
                             (unsigned long long)cdiv(rows - h + 1, 16) * (unsigned long long)cdiv(cols - w + 1, 16));
        groups_max = std::max(groups_max, (unsigned long long)cdiv(off[(size_t)k + 1] - off[(size_t)k], kTrackNV));
    }
    CHECK(at == P.tiles.size());
    CHECK(P.tiles_max == (reacq ? tiles_max : 0ull) && P.groups_max == (reacq ? groups_max : 0ull));
}

static void test_track_plan() {
    const int rows = 40, cols = 50;
    const int shapes[4][2] = {{1, 1}, {7, 9}, {17, 33}, {40, 50}};
    const int set_sizes[5] = {1, 2, 4, 5, 9};
    const int kinds[3][2] = {{MTM_U8, 1}, {MTM_U8, 3}, {MTM_U16, 1}};
    for (const auto& kind : kinds) {
        // nine templates of every shape in the kind, then one of another kind
        std::vector<BlobTempl> tl;
        for (const auto& sh : shapes)
            for (int v = 0; v < 9; ++v) tl.push_back(BlobTempl{sh[0], sh[1], kind[1], kind[0], nullptr});
        tl.push_back(BlobTempl{7, 9, kind[1] == 3 ? 1 : 3, MTM_U8, nullptr});
        for (int margin : {0, 1, 3, 8, 60})
            for (int reacq = 0; reacq < 2; ++reacq) {
                std::vector<mtm_box_unit> start;
                std::vector<int32_t> off(1, 0), idx;
                int ns = 0;
                for (int si = 0; si < 4; ++si) {
                    const int h = shapes[si][0], w = shapes[si][1];
                    const int bh = std::min(rows, h + 5), bw = std::min(cols, w + 6);
                    // the four corners, a box equal to the template, the whole frame
                    const int boxes[6][4] = {{0, 0, bh, bw}, {0, cols - bw, bh, bw}, {rows - bh, 0, bh, bw},
                                             {rows - bh, cols - bw, bh, bw}, {(rows - h) / 2, (cols - w) / 2, h, w},
                                             {0, 0, rows, cols}};
                    for (const auto& b : boxes) {
                        const int n_set = set_sizes[ns++ % 5];
                        for (int v = 0; v < n_set; ++v) idx.push_back(9 * si + (v * 4 + ns) % 9);   // (with repeats)
                        start.push_back(mtm_box_unit{idx[(size_t)off.back()], b[0], b[1], b[2], b[3]});
                        off.push_back((int32_t)idx.size());
                    }
                }
                const int n = (int)start.size();
                TrackPlan P;
                CHECK(plan_tracks(tl, rows, cols, kind[1], kind[0], start.data(), n, margin, reacq != 0, off.data(), idx.data(),
                                  "mtm_track_boxes_sets", P) == MTM_OK);
                check_plan(P, tl, rows, cols, start, off, idx, margin, reacq != 0);
                // without sets: what singleton sets give
                std::vector<int32_t> off1((size_t)n + 1), idx1((size_t)n);
                for (int k = 0; k <= n; ++k) off1[(size_t)k] = k;
                for (int k = 0; k < n; ++k) idx1[(size_t)k] = start[(size_t)k].templ_idx;
                TrackPlan A, B;
                CHECK(plan_tracks(tl, rows, cols, kind[1], kind[0], start.data(), n, margin, reacq != 0, nullptr, nullptr,
                                  "mtm_track_boxes", A) == MTM_OK);
                CHECK(plan_tracks(tl, rows, cols, kind[1], kind[0], start.data(), n, margin, reacq != 0, off1.data(),
                                  idx1.data(), "mtm_track_boxes_sets", B) == MTM_OK);
                check_plan(A, tl, rows, cols, start, off1, idx1, margin, reacq != 0);
                CHECK(A.units.size() == B.units.size() && A.tiles.size() == B.tiles.size() && A.set_off == B.set_off &&
                      A.templ_bytes == B.templ_bytes && A.tiles_max == B.tiles_max && A.groups_max == B.groups_max);
                CHECK(std::memcmp(A.units.data(), B.units.data(), sizeof(TrackUnit) * A.units.size()) == 0);
                CHECK(std::memcmp(A.tiles.data(), B.tiles.data(), sizeof(TrackTile) * A.tiles.size()) == 0);
            }
    }
    // ---- every error path: the code and the message of the entry points
    std::vector<BlobTempl> tl = {{7, 9, 1, MTM_U8, nullptr},  {7, 9, 1, MTM_U8, nullptr},  {5, 9, 1, MTM_U8, nullptr},
                                 {7, 9, 3, MTM_U8, nullptr},  {7, 9, 1, MTM_U16, nullptr}, {2048, 1025, 1, MTM_U16, nullptr},
                                 {2048, 1024, 1, MTM_U16, nullptr}, {1, 1, 1, MTM_U8, nullptr}};
    struct Bad {
        int rows, cols, dtype;
        std::vector<mtm_box_unit> start;
        std::vector<int32_t> off, idx;      // (off empty: without sets)
        bool reacq;
        std::string msg;
    };
    const mtm_box_unit ok = {0, 2, 3, 12, 14};
    const std::vector<Bad> bad = {
        {40, 50, MTM_U8, {ok, {8, 2, 3, 12, 14}}, {}, {}, false, "mtm_track_boxes: track 1: template index out of range"},
        {40, 50, MTM_U8, {ok, {-1, 2, 3, 12, 14}}, {}, {}, false, "mtm_track_boxes: track 1: template index out of range"},
        {40, 50, MTM_U8, {ok, ok}, {0, 1, 3}, {0, 0, 8}, false, "mtm_track_boxes_sets: track 1: template index out of range"},
        {40, 50, MTM_U8, {{0, 30, 3, 12, 14}}, {}, {}, false, "mtm_track_boxes: track 0: box outside the frame"},
        {40, 50, MTM_U8, {{0, 2, 40, 12, 14}}, {0, 1}, {0}, false, "mtm_track_boxes_sets: track 0: box outside the frame"},
        {40, 50, MTM_U8, {{0, -1, 3, 12, 14}}, {}, {}, false, "mtm_track_boxes: track 0: box outside the frame"},
        {40, 50, MTM_U8, {{0, 2, 3, 0, 14}}, {}, {}, false, "mtm_track_boxes: track 0: box outside the frame"},
        // (both an index out of range and a box outside: a plain track reports the index, a set the box)
        {40, 50, MTM_U8, {{8, 30, 3, 12, 14}}, {}, {}, false, "mtm_track_boxes: track 0: template index out of range"},
        {40, 50, MTM_U8, {{8, 30, 3, 12, 14}}, {0, 1}, {8}, false, "mtm_track_boxes_sets: track 0: box outside the frame"},
        {40, 50, MTM_U8, {{3, 2, 3, 12, 14}}, {}, {}, false,
         "mtm_track_boxes_nbhd: track 0: template and frames differ in pixel type or channel count"},
        {40, 50, MTM_U8, {{4, 2, 3, 12, 14}}, {}, {}, false,
         "mtm_track_boxes_nbhd: track 0: template and frames differ in pixel type or channel count"},
        {40, 50, MTM_U8, {ok}, {0, 2}, {0, 3}, false,
         "mtm_track_boxes_sets: track 0: template and frames differ in pixel type or channel count"},
        {40, 50, MTM_U8, {{0, 2, 3, 6, 14}}, {}, {}, false, "mtm_track_boxes_adapt: track 0: template larger than the box"},
        {40, 50, MTM_U8, {{0, 2, 3, 12, 8}}, {0, 2}, {0, 1}, false,
         "mtm_track_boxes_sets: track 0: template larger than the box"},
        {2048, 1025, MTM_U16, {{5, 0, 0, 2048, 1025}}, {}, {}, false,
         "mtm_track_boxes: track 0: uint16 template of more than 2^21 pixels"},
        {2048, 1025, MTM_U16, {{5, 0, 0, 2048, 1025}}, {0, 1}, {5}, false,
         "mtm_track_boxes_sets: track 0: uint16 template of more than 2^21 pixels"},
        {65536, 65537, MTM_U8, {{7, 0, 0, 4, 4}}, {}, {}, true,
         "mtm_track_boxes_reacquire: track 0: whole-frame map of 2^32 outputs or more"},
        {65536, 65537, MTM_U8, {{7, 0, 0, 4, 4}}, {0, 1}, {7}, true,
         "mtm_track_boxes_sets: track 0: whole-frame map of 2^32 outputs or more"},
        {40, 50, MTM_U8, {ok}, {1, 2}, {0, 0}, false, "mtm_track_boxes_sets: set_off[0] must be 0"},
        {40, 50, MTM_U8, {ok, ok}, {0, 1, 1}, {0}, false, "mtm_track_boxes_sets: track 1: empty set"},
        {40, 50, MTM_U8, {ok, ok}, {0, 2, 1}, {0, 1}, false, "mtm_track_boxes_sets: track 1: set_off is not ascending"},
        {40, 50, MTM_U8, {ok}, {0, 2}, {1, 0}, false,
         "mtm_track_boxes_sets: track 0: start's template is not the first of its set"},
        {40, 50, MTM_U8, {ok}, {0, 3}, {0, 1, 2}, false,
         "mtm_track_boxes_sets: track 0: the templates of a set must be of one shape"},
        // two invalid tracks: the first is reported
        {40, 50, MTM_U8, {ok, {0, 2, 3, 6, 14}, {9, 2, 3, 12, 14}}, {}, {}, false,
         "mtm_track_boxes: track 1: template larger than the box"},
        {40, 50, MTM_U8, {ok, ok, ok}, {0, 1, 1, 0}, {0}, false, "mtm_track_boxes_sets: track 1: empty set"},
    };
    for (const Bad& b : bad) {
        const std::string who = b.msg.substr(0, b.msg.find(':'));
        TrackPlan P;
        set_error("");
        const int rc = plan_tracks(tl, b.rows, b.cols, 1, b.dtype, b.start.data(), (int)b.start.size(), 2, b.reacq,
                                   b.off.empty() ? nullptr : b.off.data(), b.idx.data(), who.c_str(), P);
        if (rc != MTM_E_INVALID || b.msg != mtm_last_error())
            std::fprintf(stderr, "plan_tracks: %d '%s', expected '%s'\n", rc, mtm_last_error(), b.msg.c_str());
        CHECK(rc == MTM_E_INVALID && b.msg == mtm_last_error());
    }
    // the last sizes that pass: a uint16 template of exactly 2^21 pixels, a whole-frame map of 2^32 - 2^16 outputs
    TrackPlan P;
    const mtm_box_unit big = {6, 0, 0, 2048, 1024}, dot = {7, 0, 0, 4, 4};
    CHECK(plan_tracks(tl, 2048, 1025, 1, MTM_U16, &big, 1, 0, false, nullptr, nullptr, "mtm_track_boxes", P) == MTM_OK);
    CHECK(P.tiles.size() == 1 && P.templ_bytes[0] == (size_t)2 << 21);
    CHECK(plan_tracks(tl, 65536, 65535, 1, MTM_U8, &dot, 1, 0, true, nullptr, nullptr, "mtm_track_boxes_reacquire", P) ==
          MTM_OK);
    CHECK(P.tiles_max == 4096ull * 4096ull && P.groups_max == 1 && P.tiles.size() == 1);
}

// ---- the keys' decoder shared by host and device (mtm_quality_key.h), against bit patterns and positions worked out by hand
static uint32_t f32_bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    return b;
}

static void test_quality_key() {
    // order word of a quality (sign bit set for v >= +0, all bits complemented below) -> the score's bits for the
    // maxima methods and for the difference methods (the quality negated, then + 0.0f: never -0)
    struct Q {
        uint32_t order, score_max, score_min;
    };
    const Q qs[] = {
        {0xBFC00000u, 0x3FC00000u, 0xBFC00000u},    // quality 1.5
        {0x403FFFFFu, 0xBFC00000u, 0x3FC00000u},    // quality -1.5
        {0xFF800000u, 0x7F800000u, 0xFF800000u},    // quality +inf
        {0x80000000u, 0x00000000u, 0x00000000u},    // quality +0: the score of a difference method is -(+0) + 0 = +0
        {0x7FFFFFFFu, 0x00000000u, 0x00000000u},    // quality -0 (no kernel stores it): +0 all the same
    };
    // a zero key reads index 2^32 - 1: column and row of it in a map `ow` wide (the row as the int it is cast to)
    struct W {
        int ow, zero_col, zero_row;
    };
    const W ws[] = {{1, 0, -1}, {7, 3, 613566756}, {65535, 0, 65537}};
    const int y0 = 11, x0 = 23;
    for (int mode_min = 0; mode_min < 2; ++mode_min)
        for (const W& wd : ws) {
            const int ow = wd.ow;
            // the first output, the end of row 0, the start of row 1, the last output of a 3-row map
            const int at[4][2] = {{0, 0}, {0, ow - 1}, {1, 0}, {2, ow - 1}};
            for (const auto& rc : at)
                for (const Q& q : qs) {
                    const uint32_t idx = (uint32_t)rc[0] * (uint32_t)ow + (uint32_t)rc[1];
                    const unsigned long long key = ((unsigned long long)q.order << 32) | (0xFFFFFFFFull - idx);
                    CHECK(key_index(key) == idx);
                    const mtm_hit r = quality_key_record(key, mode_min, 4, y0, x0, ow, 5, 6);
                    CHECK(r.templ_idx == 4 && r.w == 5 && r.h == 6 && r.x == x0 + rc[1] && r.y == y0 + rc[0]);
                    CHECK(f32_bits(r.score) == (mode_min ? q.score_min : q.score_max));
                    // the host's entry is the header at origin (0, 0)
                    const mtm_hit d = decode_quality_key(key, mode_min != 0, 4, ow, 5, 6);
                    const mtm_hit z = quality_key_record(key, mode_min, 4, 0, 0, ow, 5, 6);
                    CHECK(std::memcmp(&d, &z, sizeof(mtm_hit)) == 0 && d.x == rc[1] && d.y == rc[0] &&
                          f32_bits(d.score) == f32_bits(r.score));
                }
            const mtm_hit r = quality_key_record(0ull, mode_min, 4, y0, x0, ow, 5, 6);
            CHECK(r.templ_idx == 4 && r.w == 5 && r.h == 6 && r.x == x0 + wd.zero_col && r.y == y0 + wd.zero_row);
            CHECK(f32_bits(r.score) == 0x7FC00000u);        // the quiet NaN
            const mtm_hit d = decode_quality_key(0ull, mode_min != 0, 4, ow, 5, 6);
            CHECK(d.x == wd.zero_col && d.y == wd.zero_row && f32_bits(d.score) == 0x7FC00000u);
        }
    CHECK(f32_bits(key_order_float(0xBFC00000u)) == 0x3FC00000u && f32_bits(order_to_float(0x403FFFFFu)) == 0xBFC00000u);
}

// ---- the record that steers the next pass (blocks_steer_record_inl, mtm_blocks_validate.h), threshold 2, epsilon 0.5
static void test_steer_record() {
    const double threshold = 2.0, e4 = 4.0 * 0.5;
    // 3 x 3 blocks at stride (8, 6), every block displaced by (3, 2), the centre by (5, 2): the centre's neighbours are
    // uniform (median 3, residuals 0), so 2 |2 * 5 - 6| = 8 > 2 * (0 + 2) flags it; every other block sees at most one 5
    // among at least three values, median 3, and its own residual is 0
    {
        const int nx = 3, ny = 3, sx = 8, sy = 6;
        mtm_hit recs[9];
        for (int k = 0; k < 9; ++k) recs[k] = mtm_hit{k, (k % 3) * sx + 3, (k / 3) * sy + 2, 16, 12, 0.5f + (float)k};
        recs[4].x = 1 * sx + 5;
        for (int k = 0; k < 9; ++k) {
            mtm_hit s;
            std::memset(&s, 0xEE, sizeof s);
            const bool ok = blocks_steer_record_inl(recs, nx, ny, sx, sy, k, threshold, e4, &s);
            mtm_hit expect = recs[k];
            if (k == 4) {
                expect.x = 1 * sx + 3;          // = 11: block position + the neighbours' median
                expect.y = 1 * sy + 2;          // = 8
            }
            CHECK(ok == (k != 4));
            CHECK(s.templ_idx == expect.templ_idx && s.x == expect.x && s.y == expect.y && s.w == expect.w && s.h == expect.h &&
                  f32_bits(s.score) == f32_bits(expect.score));
        }
    }
    // 1 x 4: no block has three neighbours - all valid, whatever they found
    {
        const int nx = 4, ny = 1, sx = 5, sy = 5;
        const mtm_hit recs[4] = {{0, 40, 9, 4, 4, 1.0f}, {1, -30, 0, 4, 4, 2.0f}, {2, 10, -7, 4, 4, 3.0f}, {3, 15, 100, 4, 4, 4.0f}};
        for (int k = 0; k < 4; ++k) {
            mtm_hit s;
            std::memset(&s, 0xEE, sizeof s);
            CHECK(blocks_steer_record_inl(recs, nx, ny, sx, sy, k, threshold, e4, &s));
            CHECK(std::memcmp(&s, &recs[k], sizeof(mtm_hit)) == 0);
        }
    }
}

int main() {
    std::mt19937 rng(12345);
    test_quality_key();
    test_steer_record();
    test_verify_candidates(rng);
    test_ladder();
    test_track_plan();
    test_nms_grid(rng);
    test_peak_sizing(rng);
    test_stats_route();
    test_stat_wants();
    test_host(rng);
    test_group(rng);
    // two groups driven from two caller threads at once (each group is single-caller; the library must not share state)
    std::thread a([] { std::mt19937 r(1); test_group(r); }), b([] { std::mt19937 r(2); test_host(r); });
    a.join();
    b.join();
    std::puts("sanitize_host: ok");
    return 0;
}
