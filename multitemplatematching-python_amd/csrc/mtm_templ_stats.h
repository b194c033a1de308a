// The template constants of OpenCV's common_matchTemplate from a template's per-channel sums, as one inline function
// for the host (mtm_set_templates, mtm_host.cpp) and the device (track_adopt_kernel, mtm_track.hip): a single source for
// the operation order, so that a template whose statistics are recomputed on the device carries the constants
// mtm_set_templates would give it, bit for bit.  (The library is built with -ffp-contract=off: no product below is fused
// into a sum on either side.)
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/mtm_hip.h"

#if defined(__HIP__)
#define MTM_HOST_DEVICE __host__ __device__
#else
#define MTM_HOST_DEVICE
#endif

namespace mtm {

// cv::meanStdDev + the template constants of OpenCV's common_matchTemplate, in the same
// operation order as oracle/mtm_oracle.py::match_template (so that both sides round alike).
struct TemplStats {
    double mean[4] = {0, 0, 0, 0};   // templMean per channel (zeroed when numType != 1)
    double templ_norm = 0;           // sqrt(templNorm) / sqrt(invArea)
    double templ_sum2 = 0;           // templSum2 / invArea
    double inv_area = 0;
    int all_ones = 0;                // TM_CCOEFF_NORMED with a constant template: map == 1
    double templ2_mask2_sum = 0;     // masked path: sum((T*M)^2)
    double centred_sum2 = 0;         // sum over channels of sum (T - channel mean)^2, whatever the method (error bound of the
                                     // refined raw-sum extremum of float32 classes, mtm_bf16.hip.h)
};

// From the per-channel sums (sum v, sum v^2) - or, masked, from sum (v*m)^2 alone: what a reduction over a template
// delivers (exact integers for uint8 and uint16 pixels).
MTM_HOST_DEVICE inline TemplStats templ_stats_from_sums_inl(const double* sum, const double* sumsq, double templ2_mask2_sum,
                                                            bool masked, int rows, int cols, int chans, int method) {
    TemplStats st;
    const double n = (double)rows * (double)cols;
    st.inv_area = 1.0 / ((double)rows * (double)cols);
    if (masked) {
        st.templ2_mask2_sum = templ2_mask2_sum;
        return st;
    }
    double mean[4] = {0, 0, 0, 0}, sdv[4] = {0, 0, 0, 0};
    for (int c = 0; c < chans && c < 4; ++c) {
        mean[c] = sum[c] / n;
        const double var = sumsq[c] / n - mean[c] * mean[c];
        const double var0 = var < 0.0 ? 0.0 : var;          // (std::max(var, 0.0))
        sdv[c] = sqrt(var0);
        st.centred_sum2 += var0 * n + 1e-15 * sumsq[c];     // (+ the cancellation in sumsq / n - mean^2)
    }
    if (method == MTM_TM_CCORR) return st;
    const int num_type = (method == MTM_TM_CCORR || method == MTM_TM_CCORR_NORMED) ? 0
                       : (method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED) ? 1 : 2;
    for (int c = 0; c < 4; ++c) st.mean[c] = mean[c];
    if (method != MTM_TM_CCOEFF) {
        double templ_norm = 0.0;
        for (int c = 0; c < chans && c < 4; ++c) templ_norm += sdv[c] * sdv[c];
        if (templ_norm < DBL_EPSILON && method == MTM_TM_CCOEFF_NORMED) {
            st.all_ones = 1;
            return st;
        }
        double msum = 0.0;
        for (int c = 0; c < chans && c < 4; ++c) msum += mean[c] * mean[c];
        double templ_sum2 = templ_norm + msum;
        if (num_type != 1) {
            for (int c = 0; c < 4; ++c) st.mean[c] = 0.0;
            templ_norm = templ_sum2;
        }
        templ_sum2 /= st.inv_area;
        templ_norm = sqrt(templ_norm);
        templ_norm /= sqrt(st.inv_area);
        st.templ_norm = templ_norm;
        st.templ_sum2 = templ_sum2;
    }
    return st;
}

}  // namespace mtm
