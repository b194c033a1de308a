// Sub-pixel steering of the deformed passes of a block-matching call (mtm_match_blocks_passes_steered with steer = 1,
// mtm_debug_steer_q8): the displacement that steers pass p + 1 comes from pass p's fitted position in Q8
// (1/256 pixel) and is filtered by a 3 x 3 binomial kernel over the grid.  Inline functions for the host
// (mtm_debug_steer_q8 without a context) and the device (blocks_steer_q8_kernel, blocks_smooth_q8_kernel, mtm_k_blocks.hip.h) -
// a single source for the rule.  (MTM.subpixel.fit_offsets, MTM.blocks.to_q8 and smooth_displacements state it in numpy.)
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/mtm_hip.h"
#include "mtm_blocks_deform.h"
#include "mtm_templ_stats.h"       // MTM_HOST_DEVICE

namespace mtm {

// subpixel.fit_offsets along one axis, with exactly its operations: the three float32 scores (neighbour at -1, centre,
// neighbour at +1) widened to double and negated for a minimum; 0.5 (a - c) / d with d = (a - 2 b) + c when all three are
// finite, the centre is their maximum and d < 0, else 0.0.  IEEE float64 throughout (the build contracts nothing): the
// division is a division.
MTM_HOST_DEVICE inline double steer_fit_inl(float fa, float fb, float fc, int mode_min) {
    double a = (double)fa, b = (double)fb, c = (double)fc;
    if (mode_min) {
        a = -a;
        b = -b;
        c = -c;
    }
    const double d = (a - 2.0 * b) + c;
    const bool ok = std::isfinite(a) && std::isfinite(b) && std::isfinite(c) && b >= a && b >= c && d < 0.0;
    return ok ? 0.5 * (a - c) / d : 0.0;
}

// A position in Q8: floor(256 P + 0.5) of P = pos + o, the float64 a refined call returns (|P| far below 2^31).
MTM_HOST_DEVICE inline long long steer_q8_inl(int pos, double o) {
    const double P = (double)pos + o;
    return (long long)std::floor(256.0 * P + 0.5);
}

// The steering displacement (Q8) of record k of a pass over a grid of nx columns at stride (sx, sy): the record `r` - its
// position the one found in the searched image plus the rounded field (px, py) = pred[2 k], pred[2 k + 1] -, its 3 x 3
// neighbourhood nb[9] (row-major, the found position at the centre): D8 = Q - 256 b + c.  An outlier of the median test
// (valid != nullptr and valid[k] == 0) takes 256 times the displacement of its validated record steer[k].
MTM_HOST_DEVICE inline void steer_d8_inl(const mtm_hit* recs, const float* nbhd, const int32_t* pred, const uint8_t* valid,
                                         const mtm_hit* steer, int nx, int sx, int sy, int mode_min, int k, int32_t* dx8,
                                         int32_t* dy8) {
    const long long bx = (long long)(k % nx) * sx, by = (long long)(k / nx) * sy;
    if (valid && !valid[k]) {
        *dx8 = (int32_t)(256 * ((long long)steer[k].x - bx));
        *dy8 = (int32_t)(256 * ((long long)steer[k].y - by));
        return;
    }
    const float* nb = nbhd + 9 * (size_t)k;
    const long long cx = pred[2 * (size_t)k], cy = pred[2 * (size_t)k + 1];
    const int xw = (int)(recs[k].x - deform_round_inl(cx)), yw = (int)(recs[k].y - deform_round_inl(cy));
    const long long qx = steer_q8_inl(xw, steer_fit_inl(nb[3], nb[4], nb[5], mode_min));
    const long long qy = steer_q8_inl(yw, steer_fit_inl(nb[1], nb[4], nb[7], mode_min));
    *dx8 = (int32_t)(qx - 256 * bx + cx);
    *dy8 = (int32_t)(qy - 256 * by + cy);
}

// The predictor filter at node (j, i) of an ny x nx grid of (dx, dy) pairs d: the 3 x 3 binomial kernel (1 2 1) x (1 2 1)
// over clamped indices, in int64, (sum + 8) >> 4 with an arithmetic shift.  Reads d only: the result goes elsewhere.
MTM_HOST_DEVICE inline void steer_smooth_inl(const int32_t* d, int nx, int ny, int i, int j, int32_t* sx8, int32_t* sy8) {
    long long ax = 0, ay = 0;
    for (int v = -1; v <= 1; ++v) {
        const int jj = j + v < 0 ? 0 : (j + v > ny - 1 ? ny - 1 : j + v);
        for (int u = -1; u <= 1; ++u) {
            const int ii = i + u < 0 ? 0 : (i + u > nx - 1 ? nx - 1 : i + u);
            const int w = (2 - (u < 0 ? -u : u)) * (2 - (v < 0 ? -v : v));
            const int32_t* p = d + 2 * ((long long)jj * nx + ii);
            ax += (long long)w * p[0];
            ay += (long long)w * p[1];
        }
    }
    *sx8 = (int32_t)((ax + 8) >> 4);
    *sy8 = (int32_t)((ay + 8) >> 4);
}

}  // namespace mtm
