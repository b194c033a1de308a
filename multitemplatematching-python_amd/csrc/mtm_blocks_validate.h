// The outlier test a pass's records go through before they steer the next pass (mtm_match_blocks_passes_validated,
// mtm_debug_validate_blocks): the normalised median test of Westerweel & Scarano over the displacements of a
// block's 3 x 3 grid neighbourhood, as one inline function for the host (mtm_debug_validate_blocks without a context) and
// the device (blocks_validate_kernel, mtm_k_blocks.hip.h) - a single source for the rule, so that the flags a test computes on
// the host are the flags the kernel writes.  (MTM.blocks.validate states the same rule in numpy.)  Integers, and one
// rounded float64 addition and one rounded float64 multiplication per component: no product is fused into a sum on
// either side (the device calls the _rn intrinsics, the library is built with -ffp-contract=off).
// No array below is indexed at run time: the eight neighbour values live in an array whose every index is a constant
// once the loops are unrolled, sorted by a fixed network and picked by select chains, so the kernel needs no scratch.
#pragma once
#include <cstdint>

#include "../../include/mtm_hip.h"
#include "mtm_templ_stats.h"       // MTM_HOST_DEVICE

namespace mtm {

// An absent neighbour: sorts behind every value (displacements and residuals of int32 positions stay below 2^35).
constexpr long long kValidatePad = INT64_MAX;

MTM_HOST_DEVICE inline void validate_cx(long long& a, long long& b) {
    const long long lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// v[0 .. 7] in ascending order: the 19 compare-exchanges of the optimal 8-input network, six layers.
MTM_HOST_DEVICE inline void validate_sort8(long long (&v)[8]) {
    validate_cx(v[0], v[2]); validate_cx(v[1], v[3]); validate_cx(v[4], v[6]); validate_cx(v[5], v[7]);
    validate_cx(v[0], v[4]); validate_cx(v[1], v[5]); validate_cx(v[2], v[6]); validate_cx(v[3], v[7]);
    validate_cx(v[0], v[1]); validate_cx(v[2], v[3]); validate_cx(v[4], v[5]); validate_cx(v[6], v[7]);
    validate_cx(v[2], v[4]); validate_cx(v[3], v[5]);
    validate_cx(v[1], v[4]); validate_cx(v[3], v[6]);
    validate_cx(v[1], v[2]); validate_cx(v[3], v[4]); validate_cx(v[5], v[6]);
}

// The doubled median of the n values of v that are not padding, 3 <= n <= 8 (v is sorted in place): s[(n - 1) / 2] +
// s[n / 2], both picked by a chain of selects on n over the constant indices 1 .. 4.
MTM_HOST_DEVICE inline long long validate_dmed8(long long (&v)[8], int n) {
    validate_sort8(v);
    const long long lo = n <= 4 ? v[1] : (n <= 6 ? v[2] : v[3]);
    const long long hi = n <= 3 ? v[1] : (n <= 5 ? v[2] : (n <= 7 ? v[3] : v[4]));
    return lo + hi;
}

// One component: u0 the centre's value, u the neighbours' (kValidatePad where there is none), n >= 3 of them present.
// *m2 = the doubled median of the neighbours; returns whether the centre is an outlier:
// (double)(2 |2 u0 - m2|) > threshold * ((double)rm4 + e4), rm4 the doubled median of the residuals |2 u_i - m2|.
MTM_HOST_DEVICE inline bool validate_component_inl(long long u0, const long long (&u)[8], int n, double threshold, double e4,
                                                   long long* m2) {
    long long s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = u[j];
    const long long med2 = validate_dmed8(s, n);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool pad = u[j] == kValidatePad;
        const long long d = 2 * (pad ? 0 : u[j]) - med2;
        s[j] = pad ? kValidatePad : (d < 0 ? -d : d);
    }
    const long long rm4 = validate_dmed8(s, n);
    const long long d0 = 2 * u0 - med2;
    const double lhs = (double)(2 * (d0 < 0 ? -d0 : d0));
#if defined(__HIP_DEVICE_COMPILE__)
    const double rhs = __dmul_rn(threshold, __dadd_rn((double)rm4, e4));
#else
    const double sum = (double)rm4 + e4;
    const double rhs = threshold * sum;
#endif
    *m2 = med2;
    return lhs > rhs;
}

// Block (iy, ix) of an nx x ny grid of blocks at stride (sx, sy) - block (iy, ix) at (ix sx, iy sy), its record
// recs[iy nx + ix] -: whether its displacement (record position - block position) passes the test against those of the
// blocks of its 3 x 3 neighbourhood that exist (fewer than three: valid), and in (*dx, *dy) the displacement that steers
// the next pass - its own, or for an outlier the neighbours' median per component, rounded half towards +infinity.
// Only raw records are read: the result depends on no order of evaluation.
MTM_HOST_DEVICE inline bool blocks_validate_inl(const mtm_hit* recs, int nx, int ny, int sx, int sy, int ix, int iy,
                                                double threshold, double e4, long long* dx, long long* dy) {
    const mtm_hit& c = recs[(long long)iy * nx + ix];
    const long long x0 = (long long)c.x - (long long)ix * sx, y0 = (long long)c.y - (long long)iy * sy;
    *dx = x0;
    *dy = y0;
    long long ux[8], uy[8];
    int n = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int q = j < 4 ? j : j + 1;            // (the 3 x 3 cells in row-major order without the centre)
        const int jx = ix + q % 3 - 1, jy = iy + q / 3 - 1;
        const bool in = jx >= 0 && jx < nx && jy >= 0 && jy < ny;
        const long long at = in ? (long long)jy * nx + jx : (long long)iy * nx + ix;       // (absent: a read in bounds)
        const mtm_hit& r = recs[at];
        ux[j] = in ? (long long)r.x - (long long)jx * sx : kValidatePad;
        uy[j] = in ? (long long)r.y - (long long)jy * sy : kValidatePad;
        n += in ? 1 : 0;
    }
    if (n < 3) return true;
    long long m2x, m2y;
    const bool ox = validate_component_inl(x0, ux, n, threshold, e4, &m2x);
    const bool oy = validate_component_inl(y0, uy, n, threshold, e4, &m2y);
    if (!(ox || oy)) return true;
    *dx = (m2x + 1) >> 1;
    *dy = (m2y + 1) >> 1;
    return false;
}

// Block k = iy nx + ix of the same grid: whether it passes (blocks_validate_inl), and in *steer the record that steers
// the next pass - recs[k], or for an outlier recs[k] moved to block position + the neighbours' median.  What
// blocks_validate_kernel writes per lane and mtm_debug_validate_blocks computes without a context.
MTM_HOST_DEVICE inline bool blocks_steer_record_inl(const mtm_hit* recs, int nx, int ny, int sx, int sy, int k, double threshold,
                                                    double e4, mtm_hit* steer) {
    const int ix = k % nx, iy = k / nx;
    long long dx, dy;
    const bool ok = blocks_validate_inl(recs, nx, ny, sx, sy, ix, iy, threshold, e4, &dx, &dy);
    mtm_hit r = recs[k];
    if (!ok) {
        r.x = (int)((long long)ix * sx + dx);
        r.y = (int)((long long)iy * sy + dy);
    }
    *steer = r;
    return ok;
}

}  // namespace mtm
