// The second correlation peak of a block's map (mtm_match_blocks_second, mtm_match_blocks_passes_second),
// as inline functions for the host (mtm_debug_second_peaks without a context) and the device (blocks_second_kernel,
// mtm_k_blocks.hip.h): a single source for which cells the first peak excludes and for the key a cell competes with, so that
// the second peak a test computes on the host is the one the kernel finds.  The cells are ordered as the first peak's key
// orders them (win_merge_key: order(quality) << 32 | ~row-major index, quality = score, or -score for the difference
// methods): larger quality first, -0 equal to +0, ties to the smaller index.
#pragma once
#include <cstdint>

#include "mtm_quality_key.h"

namespace mtm {

// Cell (y, x) lies inside the exclusion window of radius r >= 0 around the first peak (py, px): Chebyshev distance <= r.
MTM_HOST_DEVICE inline bool second_excluded(int y, int x, int py, int px, int r) {
    const long long dy = (long long)y - py, dx = (long long)x - px;
    const long long ay = dy < 0 ? -dy : dy, ax = dx < 0 ? -dx : dx;
    return (ay > ax ? ay : ax) <= (long long)r;
}

// The key of the cell at row-major index idx holding score s: what win_merge_key forms for it.  A NaN cell takes no part
// (key 0, below every cell's key): the calls' maps hold none, a constructed plane uses it for "no score here".
MTM_HOST_DEVICE inline unsigned long long second_cell_key(float s, int mode_min, uint32_t idx) {
    if (s != s) return 0ull;
    return ((unsigned long long)key_float_order(mode_min ? -s : s) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

// The largest key among the cells of the oh x ow map `m` (row-major, contiguous) outside the exclusion of radius r around
// the cell `first` reads (key_index), or - first == 0, no first peak - among all of them: the second peak's key, or the
// first one's.  0: no such cell.  The host's loop; blocks_second_kernel walks the same cells with the same two functions.
MTM_HOST_DEVICE inline unsigned long long second_scan_inl(const float* m, int oh, int ow, unsigned long long first, int mode_min,
                                                          int r) {
    const uint32_t at = key_index(first);
    const int py = (int)(at / (uint32_t)ow), px = (int)(at % (uint32_t)ow);
    unsigned long long best = 0ull;
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            if (first != 0ull && second_excluded(y, x, py, px, r)) continue;
            const uint32_t idx = (uint32_t)y * (uint32_t)ow + (uint32_t)x;
            const unsigned long long key = second_cell_key(m[idx], mode_min, idx);
            best = key > best ? key : best;
        }
    return best;
}

// The record of a second key for block `templ_idx` (a w x h box) whose map, ow outputs wide, starts at pixel (x0, y0):
// quality_key_record's, or - key == 0, no cell outside the exclusion - position (-1, -1) and the quiet NaN.
MTM_HOST_DEVICE inline mtm_hit second_key_record(unsigned long long key, int mode_min, int templ_idx, int y0, int x0, int ow,
                                                 int w, int h) {
    if (key != 0ull) return quality_key_record(key, mode_min, templ_idx, y0, x0, ow, w, h);
    mtm_hit r;
    r.templ_idx = templ_idx;
    r.x = -1;
    r.y = -1;
    r.w = w;
    r.h = h;
    r.score = __builtin_nanf("");
    return r;
}

}  // namespace mtm
