// The K loops of the MFMA score kernel (part of mtm_mfma.hip.h, which says what the kernel computes): the K step on operands
// in registers (mfma_step*, the generated mtm_mfma_step_asm.inc), the operand macros of the three loops an instantiation
// chooses from, tile staging (mf_stage_tile), and two of the loops: packed K (mf_kloop_kp) and plain / row-multiplexed
// (mf_kloop_plain).  The two-row loop and its tail screen are in the kernel's body (mtm_mfma.hip.h says why).  What crosses
// from a K loop into the epilogue: the accumulators, and from the two-row loop the A operand of the chunk's last step
// (r2_prev, for the next chunk) and the tail screen's verdict (tail_out).
#pragma once
#include "mtm_device_util.hip.h"
#include "mtm_mfma_params.h"

namespace mtm {

// One K step: 16 phases x MB template groups, operands already in registers.
template <int MB>
__device__ __forceinline__ void mfma_step(v4i (&acc)[MB][16], const v4i qa, const v4i qb, const v4i (&a)[MB]) {
    const int W[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
    // phases with a whole-dword shift: no VALU work
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) {
        const v4i bv = {W[cq], W[cq + 1], W[cq + 2], W[cq + 3]};
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
            acc[mb][4 * cq] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mb], bv, acc[mb][4 * cq], 0, 0, 0);
    }
    // byte shifts 1..3: 7 v_alignbyte_b32 serve four phases each
#pragma unroll
    for (int cr = 1; cr < 4; ++cr) {
        int E[7];
#pragma unroll
        for (int m = 0; m < 7; ++m) E[m] = (int)__builtin_amdgcn_alignbyte((uint32_t)W[m + 1], (uint32_t)W[m], cr);
#pragma unroll
        for (int cq = 0; cq < 4; ++cq) {
            const v4i bv = {E[cq], E[cq + 1], E[cq + 2], E[cq + 3]};
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
                acc[mb][4 * cq + cr] =
                    __builtin_amdgcn_mfma_i32_16x16x64_i8(a[mb], bv, acc[mb][4 * cq + cr], 0, 0, 0);
        }
    }
}

#ifndef MTM_MFMA_NO_ASM
#include "mtm_mfma_step_asm.inc"
#else
__device__ __forceinline__ void mfma_step_one_set(v4i (&acc)[2][16], const v4i qa, const v4i qb, const v4i (&a)[2]) {
    mfma_step<2>(acc, qa, qb, a);
}
#endif
// The K step of two MFMA groups.  MTM_STEP_VARIANT (build-time experiment switch): 2 = the whole step as ONE asm
// statement with the odd-offset windows computed from the operand (default; 44 VALU), 1 = one statement with the odd-offset
// windows copied from the even ones (47 VALU), 0 = round 2's four statements.  Measured on one box, 4K x 32 templates,
// kernel per step banded / single launch (profiles/r04a/lib_ab.txt): 0: 0.6636 / 0.6262 ms at 1943 / 2036 MHz,
// 1: 0.6499 / 0.6131 at 1893 / 1982, 2: 0.6490 / 0.6116 at 1873 / 1967 - 6 % fewer cycles, 2.3 % less time (the chip
// clocks to its power budget); register-only step: 17.4 -> 16.2 cycles per MFMA (tools/ubench/step).
#ifndef MTM_STEP_VARIANT
#define MTM_STEP_VARIANT 2
#endif
__device__ __forceinline__ void mfma_step2(v4i (&acc)[2][16], const v4i qa, const v4i qb, const v4i (&a)[2]) {
#if defined(MTM_MFMA_NO_ASM) || MTM_STEP_VARIANT == 0
    mfma_step<2>(acc, qa, qb, a);
#elif MTM_STEP_VARIANT == 2
    mfma_step2_fused_b(acc, qa, qb, a);
#else
    mfma_step2_fused(acc, qa, qb, a);
#endif
}
// The K step of the row-multiplexed tilings: both groups, or - edge steps, see the generic K loop - only one of them
// (mode 1: group 0, 2: group 1).  One asm statement with three paths (tools/gen_mfma_step.py says why).
__device__ __forceinline__ void mfma_step2_rm(v4i (&acc)[2][16], const v4i qa, const v4i qb, const v4i (&a)[2], const int mode) {
#if defined(MTM_MFMA_NO_ASM) || MTM_STEP_VARIANT == 0
    if (mode == 0) {
        mfma_step<2>(acc, qa, qb, a);
    } else {
        v4i (&acc1)[1][16] = reinterpret_cast<v4i (&)[1][16]>(acc[mode - 1]);
        const v4i a1[1] = {a[mode - 1]};
        mfma_step<1>(acc1, qa, qb, a1);
    }
#else
    mfma_step2_edges(acc, qa, qb, a, mode);
#endif
}
// the K step of an instantiation: the uint16 kernel (three accumulator sets) takes the one-scratch-set form
template <int METHOD_, int MB>
__device__ __forceinline__ void mfma_kstep(v4i (&acc)[MB][16], const v4i qa, const v4i qb, const v4i (&a)[MB]) {
    if constexpr (METHOD_ == 7 && MB == 2) mfma_step_one_set(acc, qa, qb, a);       // kMfU16
    else if constexpr (MB == 2) mfma_step2(acc, qa, qb, a);
    else mfma_step<MB>(acc, qa, qb, a);
}

// ---- The operand macros of the three loops.  They work on the locals of the one loop that uses them (acc, p, lbase,
// loff, aptr, ...) and stay macros: a step assigns to up to nine of those, and the order of its statements around the
// sched_barriers is the software pipeline.  Undefined again at the end of mtm_mfma.hip.h.
//
// Two-row loop (in the kernel's body).  B operands alternate between two register sets (qx, qy / qx2, qy2).  A operands rotate
// through three (aA, aB, aC): a step's (ACUR, APREV -> ANEXT) are this image row's template row for the wave's first output
// row, the previous step's operand - the same template row for the second output row - and the one being requested.  Six
// steps bring the rotation back to phase 0:
//   (aA, aC -> aB) (aB, aA -> aC) (aC, aB -> aA) (aA, aC -> aB) (aB, aA -> aC) | (aC, aB -> aA)
// MTM_R2_FIVE is the first five; the sixth is written out where it is used (its B sets are the second pair).
#define MTM_R2_LOAD(QA, QB, A)                                              \
    QA = *reinterpret_cast<const v4i*>(lbase + loff);           \
    QB = *reinterpret_cast<const v4i*>(lbase + loff + 16);      \
    A = *reinterpret_cast<const v4i*>(aptr);
#define MTM_R2_STEP(QA, QB, ACUR, APREV, QA2, QB2, ANEXT)                   \
    {                                                           \
        aptr += 1024;                                           \
        loff += p.lds_pitch;                                    \
        MTM_R2_LOAD(QA2, QB2, ANEXT)                            \
        __builtin_amdgcn_sched_barrier(0);                      \
        const v4i ar_[2] = {ACUR, APREV};                       \
        mfma_step2(acc, QA, QB, ar_);                           \
        __builtin_amdgcn_sched_barrier(0);                      \
    }
#define MTM_R2_STEP_LAST(QA, QB, ACUR, APREV)                               \
    {                                                           \
        aptr += 1024;                                           \
        loff += p.lds_pitch;                                    \
        __builtin_amdgcn_sched_barrier(0);                      \
        const v4i ar_[2] = {ACUR, APREV};                       \
        mfma_step2(acc, QA, QB, ar_);                           \
        __builtin_amdgcn_sched_barrier(0);                      \
    }
#define MTM_R2_FIVE()                                                        \
    MTM_R2_STEP(qx, qy, aA, aC, qx2, qy2, aB)                   \
    MTM_R2_STEP(qx2, qy2, aB, aA, qx, qy, aC)                   \
    MTM_R2_STEP(qx, qy, aC, aB, qx2, qy2, aA)                   \
    MTM_R2_STEP(qx2, qy2, aA, aC, qx, qy, aB)                   \
    MTM_R2_STEP(qx, qy, aB, aA, qx2, qy2, aC)
// Packed-K loop (mf_kloop_kp): the stream advance of one step per lane group, and the operand request.
#define MTM_KP_ADVANCE()                                            \
    {                                                       \
        aptr += 1024;                                       \
        seg += dseg;                                        \
        const bool wrap_ = seg >= nseg;                     \
        seg -= wrap_ ? nseg : 0;                            \
        loff += adv + (wrap_ ? wrapfix : 0);                \
    }
#define MTM_KP_LOAD(QA, QB, A)                                                          \
    QA = *reinterpret_cast<const v4i*>(lbase + loff);                           \
    QB = *reinterpret_cast<const v4i*>(lbase + loff + 16);                      \
    _Pragma("unroll") for (int mb = 0; mb < Cfg::MB; ++mb)                           \
        A[mb] = *reinterpret_cast<const v4i*>(aptr + mb * p.group_bytes);
// Plain / row-multiplexed loop (mf_kloop_plain): the scalar bookkeeping of the next request (64-tap block nb_i, LDS offset
// loff), the operand request, and the step - which in the row-multiplexed tilings picks the one-group form at the edges.
#define MTM_MF_ADVANCE()                                            \
    {                                                       \
        MTM_MF_APTR_STEP                                    \
        const bool wrap_ = nb_i + 1 == p.nb;                \
        loff += wrap_ ? row_adv : 64;                       \
        nb_i = wrap_ ? 0 : nb_i + 1;                        \
    }
#define MTM_MF_APTR_STEP aptr += 1024;
#define MTM_MF_LOAD(QA, QB, A)                                                          \
    QA = *reinterpret_cast<const v4i*>(lbase + loff);                           \
    QB = *reinterpret_cast<const v4i*>(lbase + loff + 16);                      \
    _Pragma("unroll") for (int mb = 0; mb < Cfg::MB; ++mb)                           \
        A[mb] = *reinterpret_cast<const v4i*>(aptr + mb * p.group_bytes);
#define MTM_MF_LOAD_LOOP(QA, QB, A) MTM_MF_LOAD(QA, QB, A)
#define MTM_MF_STEP(QA, QB, A, K)                                                       \
    if constexpr (Cfg::kRmEdges) {                                                   \
        const int mode_ = srow < edge_lo ? 1 : srow >= edge_hi ? 2 : 0; \
        mfma_step2_rm(acc, QA, QB, A, __builtin_amdgcn_readfirstlane(mode_));   \
        const bool last_ = sblk + 1 == p.nb;                                    \
        srow += last_ ? 1 : 0;                                                  \
        sblk = last_ ? 0 : sblk + 1;                                            \
    } else {                                                                    \
        mfma_kstep<Cfg::METHOD, Cfg::MB>(acc, QA, QB, A);                                 \
    }

// ---- stage (ch + 3) rows of the int8 image plane by LDS-DMA: the tile is one linear
// array of 16-byte chunks [row][cpr]; wave-instruction k of the work-group fills chunks
// 64 k .. 64 k + 63 (LDS destination = wave-uniform base + lane * 16), each lane
// supplying the global address of its chunk.  No registers, no VALU conversion.
template <class Cfg>
__device__ __forceinline__ void mf_stage_tile(const MfmaParams& p, uint8_t* smem, const uint8_t* plane, const MfItem& it,
                                              int cy0, int ch, int tid_i, int wave, int lane) {
    __syncthreads();
    {
        typedef const __attribute__((address_space(1))) void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const int nchunk = (ch + (kMfRows - 1) * it.wave_rows) * p.cpr;
        int ci = tid_i;
        int r = (ci * p.cpr_magic) >> 16, d = ci - r * p.cpr;     // ci / cpr for ci < 256 (cpr <= 33), without a division
        const uint8_t* grow = plane + (size_t)(it.y0 + cy0) * p.pitch + it.x0;
        uint8_t* lbase_w = smem + wave * 1024;
        for (; ci - lane < nchunk; ci += 256) {
            if (ci < nchunk)
                __builtin_amdgcn_global_load_lds((gptr_t)(grow + (size_t)r * p.pitch + 16 * d), (lptr_t)lbase_w,
                                                 16, 0, 0);
            lbase_w += 4096;
            r += p.cpr_rstep;
            d += p.cpr_dstep;
            if (d >= p.cpr) {
                d -= p.cpr;
                ++r;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}

// ---- K loop over the segment stream (packed K, see MfmaParams): as below, but every lane group q walks
// its own (row, segment) position - five VALU instructions of bookkeeping per step instead of scalar ones
template <class Cfg>
__device__ __forceinline__ void mf_kloop_kp(const MfmaParams& p, v4i (&acc)[Cfg::MB][16], const uint8_t* smem, const MfItem& it,
                                            const uint8_t* apack_g, int cpk, int cy0, int ch, int wave, int j, int q) {
    const int nseg = p.kp_nseg;
    const uint8_t* aptr = apack_g + (Cfg::RM ? (size_t)cpk * p.rm_cstride : (size_t)cpk * p.kp_blocks * 1024) +
                          (size_t)((cy0 * nseg) >> 2) * 1024;           // cy0 is a multiple of 64
    const uint8_t* lbase = smem + wave * it.wave_rows * p.lds_pitch + j * 16;
    const int nsteps = (ch * nseg + 3) >> 2;
    const int drow = 4 / nseg, dseg = 4 - drow * nseg;                 // uniform: stream advance of one step
    const int adv = drow * p.lds_pitch + dseg * 16, wrapfix = p.lds_pitch - nseg * 16;
    int seg = q % nseg;                                                 // this lane group's segment of step 0
    int loff = (q / nseg) * p.lds_pitch + seg * 16;
    v4i qa0, qb0, qa1, qb1, a0[Cfg::MB], a1[Cfg::MB];
    if (mf_opaque_sgpr(p.hits_only)) __builtin_amdgcn_s_setprio(3);
    MTM_KP_LOAD(qa0, qb0, a0)            // step 0
    int ks = 0;
    for (; ks + 2 <= nsteps; ks += 2) {
        MTM_KP_ADVANCE()
        MTM_KP_LOAD(qa1, qb1, a1)
        __builtin_amdgcn_sched_barrier(0);
        mfma_kstep<Cfg::METHOD, Cfg::MB>(acc, qa0, qb0, a0);
        __builtin_amdgcn_sched_barrier(0);
        MTM_KP_ADVANCE()
        MTM_KP_LOAD(qa0, qb0, a0)
        __builtin_amdgcn_sched_barrier(0);
        mfma_kstep<Cfg::METHOD, Cfg::MB>(acc, qa1, qb1, a1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (ks < nsteps) {
        mfma_kstep<Cfg::METHOD, Cfg::MB>(acc, qa0, qb0, a0);
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_s_setprio(0);
}

// ---- K loop: template rows of this chunk x 64-tap blocks, software pipelined with two
// register sets: the operands of the next step (2 LDS chunks + MB packed template rows)
// are requested before the 16*MB MFMAs of the current step issue.  sched_barrier keeps
// the compiler from sinking the requests below the MFMAs.
template <class Cfg>
__device__ __forceinline__ void mf_kloop_plain(const MfmaParams& p, v4i (&acc)[Cfg::MB][16], const uint8_t* smem, const MfItem& it,
                                               const uint8_t* apack_g, int cpk, int cy0, int ch, int wave, int j, int q) {
    const uint8_t* aptr = apack_g + (Cfg::RM ? (size_t)cpk * p.rm_cstride + (size_t)cy0 * p.nb * 1024     // + ks * 1024
                                       : ((size_t)(cpk * p.h + cy0) * p.nb) * 1024);
    const uint8_t* lbase = smem + wave * it.wave_rows * p.lds_pitch + (j + q) * 16;
    const int nsteps = ch * p.nb;
    int nb_i = 0;                       // 64-tap block of the step last requested
    int loff = 0;                       // its LDS offset: dy * lds_pitch + b * 64
    const int row_adv = p.lds_pitch - (p.nb - 1) * 64;
    v4i qa0, qb0, qa1, qb1, a0[Cfg::MB], a1[Cfg::MB];
    // The loop body is branch-free: the bookkeeping of the next step is scalar selects, and the
    // requests run up to two steps past the end of the chunk (the pack arena has slack, LDS reads
    // past the tile stay inside the allocation; nothing of it is used).  Taken scalar branches
    // cost more than the loads they would save.
    // Row-multiplexed tilings (round 4): a wave's two MFMA groups are output rows [0, R) and [R, 2 R) of the same
    // templates, and image row s of the wave's h + 2 R - 1 holds template rows of group 0 only for s < h + R - 1 and
    // of group 1 only for s >= R - outside, the group's A operand is all zero.  Those edge steps run the
    // one-group step (16 MFMAs instead of 32): 2 R of the h + 2 R - 1 steps, i.e. for ONE template or mask
    // (R = 16, h = 64) 79 step-equivalents instead of 95.
    int srow = cy0, sblk = 0;                       // image row / 64-tap block of the step being executed
    const int edge_lo = Cfg::RM ? p.rm_R : 0, edge_hi = Cfg::RM ? p.h + p.rm_R - 1 : 0x7fffffff;
    // hits-only launches: the MFMA main loop outranks the (short) epilogue of the co-resident work-group
    // (-0.9 % kernel time; with the maps written the long epilogue is the one that must not starve: +1 %)
    if (mf_opaque_sgpr(p.hits_only)) __builtin_amdgcn_s_setprio(3);
    MTM_MF_LOAD(qa0, qb0, a0)            // step 0
    int ks = 0;
    for (; ks + 2 <= nsteps; ks += 2) {
        MTM_MF_ADVANCE()
        MTM_MF_LOAD_LOOP(qa1, qb1, a1)    // step ks + 1
        __builtin_amdgcn_sched_barrier(0);
        MTM_MF_STEP(qa0, qb0, a0, 0)
        __builtin_amdgcn_sched_barrier(0);
        MTM_MF_ADVANCE()
        MTM_MF_LOAD_LOOP(qa0, qb0, a0)    // step ks + 2 (one past the end in the last iteration)
        __builtin_amdgcn_sched_barrier(0);
        MTM_MF_STEP(qa1, qb1, a1, 1)
        __builtin_amdgcn_sched_barrier(0);
    }
    if (ks < nsteps) {                    // odd number of steps: the last one is already in set 0
        MTM_MF_STEP(qa0, qb0, a0, 0)
    }
    // the last MFMAs may have been issued from inline asm: give their results time to land
    // before compiler-generated code reads the accumulators (hipcc does not see asm MFMAs)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_s_setprio(0);
}

}  // namespace mtm
