// The float64 normalisations of the MFMA score kernel's epilogues (mtm_mfma.hip.h): what turns an exact integer
// correlation and the window statistics into one float32 score, per matching method.  Part of mtm_mfma.hip.h.
#pragma once
#include "mtm_device_util.hip.h"
#include "mtm_mfma_params.h"

namespace mtm {

// finish_unmasked on values already in registers (same arithmetic, same order).  METHOD >= 0 fixes
// the matching method at compile time: the per-output code is then branch-free apart from the
// data-dependent normalisation cases (the runtime-method version spends most of its time in
// wave-uniform scalar branches).
template <int METHOD>
__device__ __forceinline__ float finish_vals(int method_rt, double corr, const double (&t)[kMaxChans], double sum2,
                                             double sq, const MfTemplConst& T, int chans) {
    const int method = METHOD >= 0 ? METHOD : method_rt;
    if (T.all_ones) return 1.0f;
    if (method == MTM_TM_CCORR) return (float)corr;
    const int num_type = (method == MTM_TM_CCORR_NORMED) ? 0
                       : (method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED) ? 1 : 2;
    const bool normed = (method == MTM_TM_SQDIFF_NORMED) || (method == MTM_TM_CCORR_NORMED) ||
                        (method == MTM_TM_CCOEFF_NORMED);
    double num = corr;
    if (num_type == 1) {
#pragma unroll
        for (int c = 0; c < kMaxChans; ++c)
            if (c < chans) num -= t[c] * T.mean[c];
    } else if (num_type == 2) {
        num = sum2 - 2.0 * num + T.templ_sum2;
        num = fmax(num, 0.0);
    }
    if (normed) {
        const double tt = sq * T.templ_norm;
        const double an = fabs(num);
        const double other = (method == MTM_TM_SQDIFF_NORMED) ? 1.0 : 0.0;
        const double sat = (an < tt * 1.125) ? ((num > 0.0) ? 1.0 : -1.0) : other;
        num = (an < tt) ? num / tt : sat;
    }
    return (float)num;
}

// Lean single-channel epilogue with the method fixed at compile time.  Same quantities and the same
// case analysis as finish_unmasked / OpenCV's common_matchTemplate; the exact integer correlation is
// rebuilt from the biased MFMA accumulator (a32 + 128*S1 + K, all exact in float64).  EXACT_DIV keeps
// the IEEE division num / t (bit-identical to the other kernels and to the oracle); otherwise the
// quotient is num * (1/sq) * (1/templ_norm) with both reciprocals correctly rounded: <= 2 ulp(double)
// from the exact quotient, i.e. the float32 result differs in the last bit for ~1e-8 of the pixels.
template <int METHOD, bool EXACT_DIV>
__device__ __forceinline__ float finish_lean(int a32, double s1, double p1, double sum2, double sq, double rsq,
                                             const MfTemplConst& T) {
    constexpr bool normed = METHOD == MTM_TM_SQDIFF_NORMED || METHOD == MTM_TM_CCORR_NORMED ||
                            METHOD == MTM_TM_CCOEFF_NORMED;
    const double corr = (double)a32 + (p1 + T.mfma_k);
    double num = corr;
    if (METHOD == MTM_TM_CCOEFF || METHOD == MTM_TM_CCOEFF_NORMED) num = corr - s1 * T.mean[0];
    if (METHOD == MTM_TM_SQDIFF || METHOD == MTM_TM_SQDIFF_NORMED) num = fmax(sum2 - 2.0 * corr + T.templ_sum2, 0.0);
    if (!normed) return (float)num;
    const double tt = sq * T.templ_norm;
    const double an = fabs(num);
    const float qf = EXACT_DIV ? (float)(num / tt) : (float)(num * (rsq * T.rtempl_norm));
    const float satf = (num > 0.0) ? 1.0f : -1.0f;
    const float other = (METHOD == MTM_TM_SQDIFF_NORMED) ? 1.0f : 0.0f;
    return (an < tt) ? qf : ((an < tt * 1.125) ? satf : other);
}

// (quotient_as_float: mtm_device_util.hip.h)
// finish_lean with the quotient computed unconditionally (the empty asm keeps the compiler from
// sinking it into a divergent branch): straight-line code, the four pixels of a lane interleave.
// Same operations in the same order as finish_lean: bit-identical results.
// DEFER (IEEE-division builds, one channel): the quotient is quotient_as_float's reciprocal product and *redo says whether
// it sits next to a float32 rounding boundary - the caller repeats those through the division behind ONE wave-uniform
// branch for the lane's four pixels (as a per-lane `if` the compiler turned the division into a select and computed both).
template <int METHOD, bool EXACT_DIV, int CH = 1, bool DEFER = false>
__device__ __forceinline__ float finish_fast(int a32, const double (&s1)[CH], double p1, double sum2, double sq,
                                             double rsq, const MfTemplConst& T, bool* redo = nullptr, bool* sat = nullptr) {
    constexpr bool normed = METHOD == MTM_TM_SQDIFF_NORMED || METHOD == MTM_TM_CCORR_NORMED ||
                            METHOD == MTM_TM_CCOEFF_NORMED;
    if constexpr (!EXACT_DIV && (METHOD == MTM_TM_CCORR_NORMED || METHOD == MTM_TM_CCOEFF_NORMED)) {
        // Default (reciprocal) mode of the two north-star methods: 5-6 float64 operations per output.
        //   num = a32 + K + 128 S1 [- mean S1]  as one fma on the biased accumulator,
        //   q   = num * (1/sq) * (1/templ_norm)   (both reciprocals correctly rounded; 0 for a flat
        //         window or a constant template, which yields the 0 OpenCV returns for t == 0),
        //   |q| < 1 -> q,  |q| < 1.125 -> +-1,  else 0: the case analysis of common_matchTemplate
        //   evaluated on the float32 quotient (it only differs from the float64 comparison when q is
        //   within one float64 rounding of 1.125; at 1 both give +-1.0f).
        double num = (double)a32 + T.mfma_k;
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) num = fma(s1[cc], METHOD == MTM_TM_CCOEFF_NORMED ? T.m128[cc] : 128.0, num);
        const float qf = (float)(num * (rsq * T.rtempl_norm));
        const float aq = fabsf(qf);
        const float sat = (aq < 1.125f) ? copysignf(1.0f, qf) : 0.0f;
        return (aq < 1.0f) ? qf : sat;
    }
    const double corr = (double)a32 + (p1 + T.mfma_k);
    double num = corr;
    if (METHOD == MTM_TM_CCOEFF || METHOD == MTM_TM_CCOEFF_NORMED) {
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) num -= s1[cc] * T.mean[cc];      // same order as finish_unmasked
    }
    if (METHOD == MTM_TM_SQDIFF || METHOD == MTM_TM_SQDIFF_NORMED) num = fmax(sum2 - 2.0 * corr + T.templ_sum2, 0.0);
    if (!normed) return (float)num;
    const double tt = sq * T.templ_norm;
    // (IEEE-division builds of the normalised methods defer; three channels with the function's general form - 16-44 B more
    // scratch in eight of those instantiations, RGB map-mode kernel 2.83 -> 2.68 ms at 4K x 32)
    float qf;
    if constexpr (EXACT_DIV && DEFER) {
        // |num| >= t (a flat window, a saturated quotient: the rules' constants, finish_saturated) is the caller's second
        // wave-uniform branch - the comparison with 1.125 t and the selects leave the common path as well
        const double q0 = num * (rsq * T.rtempl_norm);
        *redo = quotient_needs_division<(CH > 1)>(q0);   // (one channel: no tiny quotients from these operands, mtm_device_util.hip.h)
        *sat = !(fabs(num) < tt);
        return (float)q0;
    } else {
        qf = EXACT_DIV ? (float)(num / tt) : (float)(num * (rsq * T.rtempl_norm));
    }
    asm volatile("" : "+v"(qf));
    const double an = fabs(num);
    const float satf = (num > 0.0) ? 1.0f : -1.0f;
    const float other = (METHOD == MTM_TM_SQDIFF_NORMED) ? 1.0f : 0.0f;
    const float r2 = (an < tt * 1.125) ? satf : other;
    return (an < tt) ? qf : r2;
}

// What finish_fast returns where |num| >= t (same quantities, same order): +-1 below 1.125 t, else the rules' constant.
template <int METHOD, int CH = 1>
__device__ __forceinline__ float finish_saturated(int a32, const double (&s1)[CH], double p1, double sum2, double sq,
                                                  const MfTemplConst& T) {
    const double corr = (double)a32 + (p1 + T.mfma_k);
    double num = corr;
    if (METHOD == MTM_TM_CCOEFF || METHOD == MTM_TM_CCOEFF_NORMED) {
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) num -= s1[cc] * T.mean[cc];
    }
    if (METHOD == MTM_TM_SQDIFF || METHOD == MTM_TM_SQDIFF_NORMED) num = fmax(sum2 - 2.0 * corr + T.templ_sum2, 0.0);
    const double tt = sq * T.templ_norm;
    const float satf = (num > 0.0) ? 1.0f : -1.0f;
    const float other = (METHOD == MTM_TM_SQDIFF_NORMED) ? 1.0f : 0.0f;
    return (fabs(num) < tt * 1.125) ? satf : other;
}

// finish_lean with the method chosen at run time (one channel): `corr` is the exact correlation.
template <bool EXACT_DIV>
__device__ __forceinline__ float finish_rt(int method, double corr, double s1, double sum2, double sq, double rsq,
                                           const MfTemplConst& T) {
    const bool normed = method == MTM_TM_SQDIFF_NORMED || method == MTM_TM_CCORR_NORMED || method == MTM_TM_CCOEFF_NORMED;
    double num = corr;
    if (method == MTM_TM_CCOEFF || method == MTM_TM_CCOEFF_NORMED) num = corr - s1 * T.mean[0];
    if (method == MTM_TM_SQDIFF || method == MTM_TM_SQDIFF_NORMED) num = fmax(sum2 - 2.0 * corr + T.templ_sum2, 0.0);
    if (!normed) return (float)num;
    const double tt = sq * T.templ_norm;
    float qf = EXACT_DIV ? (float)(num / tt) : (float)(num * (rsq * T.rtempl_norm));
    asm volatile("" : "+v"(qf));
    const double an = fabs(num);
    const float satf = (num > 0.0) ? 1.0f : -1.0f;
    const float other = (method == MTM_TM_SQDIFF_NORMED) ? 1.0f : 0.0f;
    const float r2 = (an < tt * 1.125) ? satf : other;
    return (an < tt) ? qf : r2;
}

// Masked templates (OpenCV's matchTemplateMask, binary uint8 mask, reference MTM/__init__.py:78,:216):
// c1 = sum I*(T*M) comes from the MFMA accumulator exactly like an unmasked correlation (the packed
// template is T*M), c2 = sum I^2*M from the class's raw row-multiplexed pass (MfmaParams::sq_fused; MTM_ROW_MUX=0: the MASKSQ dot4 pass).  No guards, as in OpenCV: 0/0 is NaN.
// DEFER (IEEE builds, round 6): the float32 value of num / sqrt(tms c2) from num * (RN(1 / sqrt(c2)) * RN(1 / sqrt(tms))) - six
// roundings against the reference's three, <= 9 ulp(double) apart - with quotient_needs_division's general form; a quotient
// that is not finite (c2 == 0: inf or the 0 / 0 NaN of OpenCV) takes the reference sequence as well, so that even the NaN's bits
// are the division's.  *redo: the caller repeats those behind one wave-uniform branch (see finish_fast).
template <int METHOD, bool EXACT_DIV, bool DEFER = false>
__device__ __forceinline__ float finish_lean_masked(int a32, double p1, double c2, double rsqrt_c2,
                                                    const MfTemplConst& T, bool* redo = nullptr) {
    const double c1 = (double)a32 + (p1 + T.mfma_k);
    if (METHOD == MTM_TM_CCORR) return (float)c1;
    if (METHOD == MTM_TM_SQDIFF) return (float)(-2.0 * c1 + c2 + T.tms);
    const double num = (METHOD == MTM_TM_SQDIFF_NORMED) ? (-2.0 * c1 + c2 + T.tms) : c1;
    if constexpr (EXACT_DIV && DEFER) {
        const double q0 = num * (rsqrt_c2 * T.rsqrt_tms);
        const bool finite = ((uint32_t)__double2hiint(q0) & 0x7ff00000u) != 0x7ff00000u;
        *redo = quotient_needs_division<true>(q0) || !finite;
        return (float)q0;
    }
    return EXACT_DIV ? (float)(num / sqrt(T.tms * c2)) : (float)(num * (rsqrt_c2 * T.rsqrt_tms));
}

}  // namespace mtm
