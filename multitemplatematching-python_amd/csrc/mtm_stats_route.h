// Which kernel chain produces a size class's window statistics (stats_route) and which planes and records the class's score
// kernel reads (stat_wants), each written once: launch_stats (mtm_stats.hip) asks both and switches on the route,
// class_reads_f32 / the banded-upload rule (mtm_launch.hip) / choose_tiling (mtm_placement.hip) ask the route, the
// test-support entries mtm_debug_window_stats and mtm_debug_window_stats_route (mtm_stats.hip) admit their arguments with
// it, and the host checks (tests/native/sanitize_host.cpp) walk every boundary.  Plain C++: no HIP type, no context.
#pragma once
#include "../../include/mtm_hip.h"

namespace mtm {

// the numbers of mtm_debug_window_stats_route's `route` argument and info[0] (include/mtm_hip.h: MTM_STATS_ROUTE_*)
enum StatsRoute {
    kStatsRouteU8 = 0,        // stats_u8_kernel: uint8, 1 channel
    kStatsRouteU8MC = 1,      // stats_u8_mc_kernel<3>: uint8, 3 channels
    kStatsRouteU16 = 2,       // stats_u16_kernel: uint16, 1 channel, over the two biased byte planes
    kStatsRouteU8TwoPass = 3,       // hsum_u8_kernel + vsum_stats_kernel<uint32_t, unsigned long long>: every other uint8 class
    kStatsRouteU8TwoPassWide = 4,   // hsum_kernel<uint32_t> on the float32 plane + the same vsum: ... of images too wide for that
    kStatsRouteF64Lds = 5,    // hsum_lds_kernel + vsum_stats_kernel<double, double>: everything else
    kStatsRouteF64 = 6,       // hsum_kernel<double> + the same vsum: ... with a window too wide for the LDS row
    kStatsRouteCount = 7
};

// what the kernels are built for
constexpr int kStatsFusedMaxW = 768;        // fused kernels: a strip of 1024 image columns holds >= 256 output columns
constexpr int kStatsHsumU8MaxCols = 8191;   // hsum_u8_kernel: two uint32 prefix rows of cols + 1 words in 64 KB of LDS
constexpr int kStatsHsumLdsMaxW = 1024;     // hsum_lds_kernel: 256 * 16 + w floats (and their padding) in LDS
constexpr double kStatsU32Range = 4294967296.0;
// the units the launches' row ranges are counted in (the banded runners of mtm_launch.hip cut their bands on them)
#ifndef MTM_STAT_BAND4
#define MTM_STAT_BAND4 8
#endif
constexpr int kStatBand4 = MTM_STAT_BAND4;    // fused statistics kernels: output rows per row unit (the unit of [sb0, sb1) ranges)
#ifndef MTM_VSUM_BAND
#define MTM_VSUM_BAND 32
#endif
constexpr int kVsumBand = MTM_VSUM_BAND;      // vsum_stats_kernel: output rows per band (a band restarts its column sums)

// a fused kernel's uint32 prefix sums hold every window sum it forms: chans * w * h * 255^2 (uint8: the squares of all
// channels in one prefix) or w * h * 65535 (uint16: the sums; the squares are uint64) stays below 2^32
inline bool stats_fused_fits(int dtype, int chans, int h, int w) {
    if (w > kStatsFusedMaxW) return false;
    return (double)chans * w * h * (dtype == MTM_U16 ? 65535.0 : 65025.0) < kStatsU32Range;
}

inline StatsRoute stats_route(int dtype, int chans, int h, int w, int cols, bool fuse_stats) {
    if (dtype == MTM_U8) {
        if (fuse_stats && chans == 1 && stats_fused_fits(dtype, 1, h, w)) return kStatsRouteU8;
        if (fuse_stats && chans == 3 && stats_fused_fits(dtype, 3, h, w)) return kStatsRouteU8MC;
        return cols <= kStatsHsumU8MaxCols ? kStatsRouteU8TwoPass : kStatsRouteU8TwoPassWide;
    }
    if (dtype == MTM_U16 && fuse_stats && chans == 1 && stats_fused_fits(dtype, 1, h, w)) return kStatsRouteU16;
    return w <= kStatsHsumLdsMaxW ? kStatsRouteF64Lds : kStatsRouteF64;
}

// May `route` run on such a class at all (a forced route of the test-support entry)?  nullptr: yes; else what it is not
// built for.  stats_route's own answer always passes.
inline const char* stats_route_refusal(int route, int dtype, int chans, int h, int w, int cols) {
    switch (route) {
    case kStatsRouteU8:
        return dtype == MTM_U8 && chans == 1 && stats_fused_fits(dtype, 1, h, w) ? nullptr
               : "the fused kernel takes uint8, 1 channel, w <= 768 and w h 255^2 < 2^32";
    case kStatsRouteU8MC:
        return dtype == MTM_U8 && chans == 3 && stats_fused_fits(dtype, 3, h, w) ? nullptr
               : "the fused RGB kernel takes uint8, 3 channels, w <= 768 and 3 w h 255^2 < 2^32";
    case kStatsRouteU16:
        return dtype == MTM_U16 && chans == 1 && stats_fused_fits(dtype, 1, h, w) ? nullptr
               : "the fused uint16 kernel takes uint16, 1 channel, w <= 768 and w h 65535 < 2^32";
    case kStatsRouteU8TwoPass:
        if (dtype != MTM_U8) return "the uint8 two-pass kernels take uint8 images";
        return cols <= kStatsHsumU8MaxCols ? nullptr : "hsum_u8_kernel takes cols <= 8191";
    case kStatsRouteU8TwoPassWide:
        // (uint32 row sums of the float32 plane: exact whatever the width; w * 255^2 < 2^32 holds for every w <= 16384)
        return dtype == MTM_U8 ? nullptr : "the uint8 two-pass kernels take uint8 images";
    case kStatsRouteF64Lds:
        return w <= kStatsHsumLdsMaxW ? nullptr : "hsum_lds_kernel takes w <= 1024";
    case kStatsRouteF64:
        return nullptr;
    default:
        return "no such route";
    }
}

// What the score kernel of a size class reads of the window statistics - a function of the call's method and the class's
// placement, nothing else: launch_stats sizes, carves and fills exactly this.  (The tail boxes' records are not here:
// tail_split_for needs the call's route.)
struct StatWants {
    bool none = false;          // the class's kernel reads no statistics at all: no launch
    bool masked_mfma = false;   // masked class on the int8 matrix cores: window sums only, sum2 from the sum I^2 M pass
    int num_type = 0;           // what the numerator needs: 0 nothing, 1 the window sums per channel, 2 the sum of squares
    bool normed = false;        // the sqrt plane
    bool want_t = false;        // the window sums are written
    bool want_sum2 = false;     // ... the sum of squares, by the fused uint8 kernel (every other chain writes it anyway)
    bool rsq = false;           // the reciprocal of the sqrt plane (fused uint8 kernel)
    bool blk = false;           // the records per 16-column block (fused uint8 and uint16 kernels): the hits-only screens
};
// `mask_rm`: the masked class has its row-multiplexed mask pack (SizeClass::mask_rm_off >= 0) - that chooses the kernel of
// the sum I^2 M pass, not what is wanted of this one: no field depends on it (the host checks hold that)
inline StatWants stat_wants(int method, int kernel, bool masked, bool mask_rm, int r2, int rm_R, int chans, int dtype) {
    (void)mask_rm;
    StatWants s;
    const bool want_t_always = kernel == MTM_KERNEL_MFMA || kernel == MTM_KERNEL_MFMA16 || kernel == MTM_KERNEL_MFMA_F32;
    s.masked_mfma = masked && kernel == MTM_KERNEL_MFMA;
    s.none = (masked && !s.masked_mfma) || (method == MTM_TM_CCORR && !want_t_always);
    s.num_type = s.masked_mfma ? 0
               : (method == MTM_TM_CCORR_NORMED) ? 0
               : (method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED) ? 1 : 2;
    s.normed = !s.masked_mfma && (method == MTM_TM_SQDIFF_NORMED || method == MTM_TM_CCORR_NORMED ||
                                  method == MTM_TM_CCOEFF_NORMED);
    s.want_t = s.num_type == 1 || want_t_always;
    // (masked classes on the matrix cores: the sum2 plane is written by the sum I^2 M pass, not by the statistics launch)
    s.want_sum2 = !s.masked_mfma && (s.num_type == 2 || (s.normed && s.num_type != 1) || !want_t_always);
    s.rsq = rm_R > 0 && s.normed;
    // statistic ranges per 16-pixel column block: the hits-only screens of the multi-row and row-multiplexed tilings
    // (uint8), of the uint16 kernel
    if (dtype == MTM_U16)
        s.blk = chans == 1 && s.normed && kernel == MTM_KERNEL_MFMA16;
    else if (dtype == MTM_U8)
        s.blk = chans == 1 && ((r2 > 0 && s.normed) ||
                               (rm_R > 0 && (s.normed || (s.masked_mfma && method == MTM_TM_CCORR_NORMED))));
    return s;
}

}  // namespace mtm
