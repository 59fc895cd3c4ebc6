#pragma once
// The selective-scan backward's recurrence, written once: the sequential kernel K2 (scan_bwd_impl.h) and the chunk-parallel
// kernel K2c (scan_bwd_chunked.h) call these functions and nothing else for the arithmetic of a step.  A lane holds its states
// as PAIRS (f32x2, packed fp32 instructions); every function below works on one pair or on the per-channel scalars of a step.
//
// One reverse step j of SURVEY.md A.1-bwd, per state n (a = exp(delta A), h_j = state after step j, h_{j-1} = before it,
// gy = g_out silu(z), carry = a_{j+1} lambda_{j+1} arriving from the step to the right):
//     y~     += C h_j                     the output before the gate (only the z gradient needs it)
//     lambda  = C gy + carry              dL/dh_j
//     dC      = h_j gy                    summed over the channels by the caller
//     carry   = a lambda                  leaves for step j-1
//     Gt      = carry h_{j-1}             = lambda a h_{j-1}
//     dlA    += A2 Gt                     the decay's part of ddelta (A2 = A log2 e; the LN2 comes back in step_outputs)
//     dA     += Gt delta
//     GB     += lambda B                  the input's part of ddelta and du
//     dB      = lambda delta u            summed over the channels by the caller
// and per channel, from the sums over its states:
//     ddelta  = (u GB + ln2 dlA) softplus'    du = delta GB + gy D    dz = g_out (y~ + D u) sigma(z) (1 + z (1 - sigma(z)))
//     dD     += gy u                          dbias += ddelta
//
// Form: the functions are inlined into loops that are unrolled only later, and where a by-value argument would read its array
// element (or, inside a lambda, its captured variable) ahead of the call, hipcc schedules and allocates K2 differently (the
// d_state 16 kernels then spill).  So inputs that callers pass from arrays travel as const references, the statements keep the
// order the terms are listed in, and callers evaluate a result before the address of the store that takes it.
// profiles/scan_bwd_one_recurrence.txt records which forms left K2's code as it was.
#include "dm_common.h"

namespace dm {

// make a value opaque to the optimiser (costs no instruction): stops it from keeping the exp() / B-row
// values of the recompute pass alive across the whole chunk just to save recomputing them
__device__ __forceinline__ float opaque(float x) {
    asm volatile("" : "+v"(x));
    return x;
}

// ---- the decay factors a = exp(delta A) ------------------------------------------------------------------------------------
// DM_FLAG_A_SHARED (ASH): one decay factor for all states of the channel, evaluated once per step by decay_shared
template <bool ASH>
__device__ __forceinline__ float decay_shared(f32x2 A2_0, float dl) {
    return ASH ? fast_exp2(A2_0.x * dl) : 0.f;
}
template <bool ASH>
__device__ __forceinline__ f32x2 decay_pair(f32x2 A2k, float dl, float a_shared) {
    if (ASH) return (f32x2){a_shared, a_shared};
    const f32x2 t = A2k * dl;
    return (f32x2){fast_exp2(t.x), fast_exp2(t.y)};
}

// DMODE (delta mode): 0 = delta + bias used as is, 1 = softplus(delta + bias) (DM_FLAG_DELTA_SOFTPLUS), 2 = delta already holds
// softplus(raw + bias) (DM_FLAG_DELTA_ACTIVATED: the producer of delta applied it once per element instead of every scan
// direction twice); the returned ddelta is the gradient of the RAW value in every mode: softplus'(x) = 1 - exp(-softplus(x)).
template <int DMODE>
__device__ __forceinline__ float activate_delta(float raw, float bias) {
    float x = raw;
    if (DMODE != 2) x += bias;
    if (DMODE == 1) x = softplus_f(x);
    return x;
}

// one forward step of a state pair: h <- a h + B delta u
__device__ __forceinline__ void recompute_pair(f32x2& h, f32x2 a, f32x2 bb, float du) {
    h = a * h + bb * du;
}

// the pair's part of one reverse step (the terms listed at the top).  h arrives as h_j and leaves as h_{j-1} = hp.
template <bool HAS_Z, bool PIN_DA>
__device__ __forceinline__ void adjoint_pair(f32x2& h, const f32x2& hp, f32x2& carry, f32x2& dA, f32x2& yp2, f32x2& GB2, f32x2& dlA2,
                                             const f32x2& A2k, const f32x2& a, const f32x2& bb, const f32x2& cc, float gy, float du, float dlo, f32x2& dBp, f32x2& dCp) {
    const f32x2 hj = h;
    if (HAS_Z) yp2 += cc * hj;
    const f32x2 G = cc * gy + carry;             // dL/dh_j
    dCp = hj * gy;
    carry = a * G;                               // a_j * dL/dh_j, flows to step j-1
    const f32x2 Gt = carry * hp;                 // = G * a * h_{j-1}
    dlA2 += A2k * Gt;
    dA += Gt * dlo;
    if (PIN_DA) {
        dA.x = opaque(dA.x);                     // accumulate NOW: left alone the scheduler defers all 8 steps'
        dA.y = opaque(dA.y);                     // products to the chunk end and keeps 64 VGPRs alive for them
    }
    GB2 += G * bb;
    dBp = G * du;
    h = hp;
}

// the bare recursion of K2c's pass 1 (no states, no outputs)
__device__ __forceinline__ void carry_only_pair(f32x2& carry, f32x2 a, f32x2 cc, float gy) {
    carry = a * (cc * gy + carry);
}

// the gate's part of a step: gy = g silu(z), and sigma(z) for the z gradient
template <bool HAS_Z>
__device__ __forceinline__ float gate_gy(float g, float z, float& sz) {
    sz = 1.f;
    if (!HAS_Z) return g;
    sz = sigmoid_f(z);
    return g * z * sz;
}

// (dpp<>, slice_sum<SPLIT>: dm_common.h -- the forward splits wide channels over lanes the same way)

// the lane's sums over its states (yp2: C.h, GB2: lambda.B, dlA2: A2.Gt, one f32x2 of partial sums each) turned into the step's
// outputs.  The lane that owns the channel adds dDi to its dD sum and ddl to its dbias sum.
template <int DMODE, int SPLIT>
__device__ __forceinline__ void step_outputs(const f32x2& yp2, const f32x2& GB2, const f32x2& dlA2, const float& u, const float& dlo, const float& gy, const float& Dv,
                                             float& ddl, float& duv, float& ypre, float& dDi) {
    ypre = slice_sum<SPLIT>(yp2.x + yp2.y) + Dv * u;
    const float GB = slice_sum<SPLIT>(GB2.x + GB2.y);
    const float dlA = slice_sum<SPLIT>(dlA2.x + dlA2.y);
    ddl = u * GB + LN2 * dlA;
    duv = dlo * GB + gy * Dv;
    if (DMODE != 0) ddl *= (1.0f - fast_exp2(-dlo * LOG2E));   // softplus'(x) = sigmoid(x) = 1 - exp(-softplus(x))
    dDi = gy * u;
}
// dz = g_out y~ silu'(z), from the pre-gate output ypre that step_outputs returns
__device__ __forceinline__ float gate_grad(float g, float ypre, float z, float sz) {
    return g * ypre * sz * (1.0f + z * (1.0f - sz));
}

// ---- the forward's checkpoints (the state entering every DM_SCAN_CKPT_EVERY-step sub-chunk) ------------------------------------
// which slot holds the state entering sub-chunk ci: slot ci for 0 < SUB ci < L, slot 0 (= the state after the last step) for
// SUB ci == L, none (-1: the state is zero) for ci == 0 and past the end.  (L by reference: see "Form" at the top.)
__device__ __forceinline__ int ckpt_slot(int ci, const int& L) {
    constexpr int SUB = DM_SCAN_CKPT_EVERY;
    return (ci > 0 && ci * SUB < L) ? ci : ((ci > 0 && ci * SUB == L) ? 0 : -1);
}
// raw checkpoint words (PACKED: one word per bf16 pair; else two fp32 words per pair) to the NP state pairs from first_pair on
template <bool PACKED, int NP, int W>
__device__ __forceinline__ void unpack_ckpt(f32x2 (&h)[NP], const uint32_t (&w)[W], int first_pair) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int kk = first_pair + k;
        if constexpr (PACKED) {
            h[k].x = __uint_as_float(w[kk] << 16);
            h[k].y = __uint_as_float(w[kk] & 0xffff0000u);
        } else {
            h[k].x = __uint_as_float(w[2 * kk]);
            h[k].y = __uint_as_float(w[2 * kk + 1]);
        }
    }
}

// ---- dB/dC lane-group sums on the matrix pipe (16-bit I/O only) ------------------------------------------------------------
// v_mfma_f32_16x16x32_bf16 with a 0/1 selector as the A fragment sums the B fragment over the 4 lane groups:
// lane l supplies B[k = (l>>4, e)][j = l&15] = value e of lane l, and A[i = l&15][k = (l>>4, e)] = (e == i) gives
// D[i][j] = sum_g value_i(lane j + 16 g).  Two instructions (values 0..7, 8..15) leave register r of lane l
// holding the lane-group total of value 4*(l>>4) + r for row position l&15 -- the same reduce-scatter as the
// 12 permlane swaps + 12 adds of lane_group_reduce, on the otherwise idle matrix pipe.  The products are rounded to bf16
// first (they are re-rounded to the 16-bit I/O dtype later anyway); fp32 I/O keeps the exact VALU path.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t pack_bf16(f32x2 v) {
    return dm_cvt_pk_bf16(v.x, v.y);
}
__device__ __forceinline__ void mfma_selectors(int lane, u32x4_t& a_lo, u32x4_t& a_hi) {
    const int i = lane & 15;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        a_lo[p] = ((i == 2 * p) ? 0x3F80u : 0u) | ((i == 2 * p + 1) ? 0x3F800000u : 0u);
        a_hi[p] = ((i == 2 * p + 8) ? 0x3F80u : 0u) | ((i == 2 * p + 9) ? 0x3F800000u : 0u);
    }
}
// 16 values per lane as eight bf16 pairs pk[0..8) -> their lane-group totals (register r of lane l = value 4*(l>>4) + r)
__device__ __forceinline__ f32x4 group_sum16(const u32x4_t& a_lo, const u32x4_t& a_hi, const uint32_t* pk) {
    const u32x4_t v_lo = {pk[0], pk[1], pk[2], pk[3]};
    const u32x4_t v_hi = {pk[4], pk[5], pk[6], pk[7]};
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a_lo), __builtin_bit_cast(bf16x8_t, v_lo), d, 0, 0, 0);
    d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a_hi), __builtin_bit_cast(bf16x8_t, v_hi), d, 0, 0, 0);
    return d;
}

}  // namespace dm
