#pragma once
// K2c  chunk-parallel selective-scan BACKWARD for SMALL launches (graphed small-batch training: the reference's own
// config/brain.yaml trains at global batch 8, i.e. 1-8 samples per GPU).
//
// The sequential kernel (scan_bwd_impl.h) puts one wave on (sequence, 64 channels) for all L steps; at nseq 24 that is 96
// workgroups on 256 CUs and every launch costs the full 196-step dependent chain (~190 us, a quarter of the graphed batch-8
// step).  The adjoint recurrence is LINEAR in its carry,
//       G_j = C_j * gy_j + carry_{j+1},      carry_j = a_j * G_j            (a_j = exp(delta_j * A), reverse time)
// so the time axis is cut into NW chunks of LC steps, one WAVE per chunk inside a workgroup that owns (sequence, 64 channels):
//   pass 1   every wave sweeps its chunk backwards from carry = 0 with the bare recursion (no states, no outputs) and
//            publishes, per state, the carry leaving the chunk on the left  c_loc  and the chunk's total decay
//            Q = exp(A * sum(delta))                                                                          -> LDS
//   combine  after one barrier wave c folds the chunks to its right:  X <- c_loc(j) + Q(j) * X,  j = NW-1 .. c+1
//   pass 2   every wave runs the full backward of its chunk (recompute from the forward's checkpoints -- chunk starts are
//            multiples of the checkpoint spacing --, adjoint sweep, all gradients) starting from the true carry X.
// The dependent chain is ~(0.25 + 1) * L/NW steps instead of L.  dB/dC: a wave owns its steps alone, so the lane sum is
// finished in the wave (matrix-pipe lane-group sums as in the sequential kernel, then a DPP row sum) and stored as ONE partial
// row per (step, 64 channels); dA/dD/dbias of the NW waves meet in LDS.  This is the "wavefront-parallel" form of the north
// star taken where latency, not throughput, is the limit; selection by launch size: bwd_chunked_lc().
//
// LONG (196 < L <= 1024: the 256- and 512-pixel image sizes at patch 2) puts a segment loop around that body, the mirror image of
// the forward's (scan_fwd_chunked.h).  The workgroup walks the sequence in segments of G = NW * LC tokens aligned at token 0, from
// the LAST segment to the first; within a segment wave c owns LC consecutive steps as above and its local carry is still computed
// from zero.  The fold starts from the carry entering the segment from the right instead of 0, and the same fold continued over
// chunk 0 is the carry entering the next segment to the left.  Only wave 0's fold ends there, so it completes it and leaves the
// result in LDS (carry_lds, two buffers alternating by segment parity), where every wave picks it up after the next publish barrier.
// The segment count is workgroup-uniform: every wave runs every segment and meets both barriers of it; a wave whose chunk lies past
// L has nl = 0 (decay 1, carry 0, no stores).  The second barrier separates the last fold read of xch_lds from the next segment's
// publish (and, after the last segment walked, from the parameter-gradient partials).  dA / dD / dbias stay in registers across the
// whole loop and meet in LDS once after it.  Checkpoints and dB/dC partial rows use the global step index, so the kernel reads what
// either forward wrote and every partial row is still written once.  Launches with L <= 196 are the one-segment instantiations, unchanged.
// Two things keep values out of the loop's live set, which is full at 256 VGPRs in pass 2: the slab copy goes through buffer
// addressing with a per-lane offset rebuilt in every segment, and the epilogue rebuilds its lane index.
//
// Resources per instantiation (gfx950, tools/kernel_regs.sh scan_bwd_<dtype> scan_bwd_chunked_kernel; 448 threads at two waves per
// SIMD: 256 VGPRs per wave, 160 KB LDS):
//                                         one segment (7 x 28 and 7 x 8)          LONG (7 x 28)
//   LDS                                   89 600 / 71 680 B                       97 792 B (slab 25 088 + xch 64 512 + carry 8 192)
//   no z (the mixer's hoisted launch, delta modes 0 / 1 / 2, with and without row tables), every dtype
//     VGPRs                               246-256                                 254-256
//     scratch / spilled VGPRs             0 / 0                                   0 / 0
//   z + A shared (the Mamba-2 pattern)    220-234, 0 / 0                          223-230, 0 / 0
//   z, per-state decay: 256 VGPRs, spilled VGPRs (scratch bytes)
//     bf16                                17-28 (60-84)                           20 (80)
//     fp16                                9-21 (32-56)                            11-14 (40-52)
//     fp32                                5-16 (24-52)                            13-16 (44-48)
// The gated per-state instantiations spill in the step body they share with their one-segment twins (the gate's z, silu and dz on
// top of a full pass 2); the segment loop adds nothing to it.
#include <cstdlib>
#include "scan_bwd_impl.h"

namespace dm {

template <typename T, typename TBC, bool HAS_Z, bool IDX, int DMODE, int NW, int LC, bool ASH = false, bool LONG = false>   // DMODE, ASH: scan_bwd_step.h
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2))) void scan_bwd_chunked_kernel(const mix_args<dm_scan_bwd_args> pm) {
    const dm_scan_bwd_args& p = pm.a[blockIdx.z];      // grid.z = congruent launches sharing this one (the two mixers of a block)
    constexpr int N = 16, NPL = N / 2, SUB = DM_SCAN_CKPT_EVERY, M = 2 * N;
    constexpr int ES = (int)sizeof(T);
    constexpr bool MFMA_RED = std::is_same<T, bf16_t>::value;
    constexpr int G = NW * LC;                          // tokens per segment
    static_assert(LC % SUB == 0, "chunks must start on checkpoints");
    __shared__ __attribute__((aligned(16))) float bc_lds[NW][LC][2 * N];        // [B row | C row] of every step of the wave's chunk
    __shared__ float xch_lds[NW][2][N + 2][WAVE];                                 // pass 1: [chunk][c_loc | Q][state][lane]; end: dA|dD|dbias partials
    __shared__ float carry_lds[LONG ? 2 : 1][LONG ? N : 1][WAVE];                 // LONG: [segment parity][state][lane]

    const int lane = threadIdx.x & 63;
    const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);               // wave = chunk index
    const int d_raw = blockIdx.x * WAVE + lane;
    const bool active = d_raw < p.dim;
    const int d = active ? d_raw : p.dim - 1;
    const int s = blockIdx.y;
    const int L = p.seqlen;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int grp = (blockIdx.x * WAVE) / (p.dim / p.ngroups);
    const int nwg = gridDim.x;

    const rsrc_t r_u = make_rsrc((const T*)p.u + (int64_t)s * p.u_ss);
    const rsrc_t r_dt = make_rsrc((const T*)p.delta + (int64_t)s * p.dt_ss);
    const rsrc_t r_z = make_rsrc(HAS_Z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_g = make_rsrc((const T*)p.dout + (int64_t)((IDX && !(p.flags & DM_FLAG_DOUT_PER_SEQ)) ? sb : s) * p.do_ss);
    const rsrc_t r_du = make_rsrc((T*)p.du + (int64_t)s * p.du_ss);
    const rsrc_t r_ddt = make_rsrc((T*)p.ddelta + (int64_t)s * p.ddt_ss);
    const rsrc_t r_dz = make_rsrc(HAS_Z ? (T*)p.dz + (int64_t)s * p.dz_ss : nullptr);
    const TBC* __restrict__ Bg = (const TBC*)p.B + (int64_t)s * p.B_ss + (int64_t)grp * p.B_sg;
    const TBC* __restrict__ Cg = (const TBC*)p.C + (int64_t)s * p.C_ss + (int64_t)grp * p.C_sg;
    const rsrc_t r_B = make_rsrc(Bg), r_C = make_rsrc(Cg);                        // LONG: the slab copy of every segment
    constexpr bool CK_PACKED = std::is_same<T, bf16_t>::value;
    constexpr int CK_ROWS = CK_PACKED ? N / 2 : N;
    constexpr int H0W = CK_PACKED ? NPL : 2 * NPL;
    const int nck = (L + SUB - 1) / SUB;
    const rsrc_t r_ck = make_rsrc((const uint32_t*)p.ckpt + (int64_t)s * nck * CK_ROWS * p.dim);
    const int vo = d * ES, vo_ck = d * 4;
    const int sl_u = (int)p.u_sl * ES, sl_dt = (int)p.dt_sl * ES, sl_z = (int)p.z_sl * ES, sl_g = (int)p.do_sl * ES;
    const int sl_du = (int)p.du_sl * ES, sl_ddt = (int)p.ddt_sl * ES, sl_dz = (int)p.dz_sl * ES;
    const cptr<int32_t> zidx = IDX ? as_const(p.z_row_index + (int64_t)dir * L) : nullptr;
    const cptr<int32_t> oidx = IDX ? as_const(p.out_row_index + (int64_t)dir * L) : nullptr;

    f32x2 A2[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        A2[k].x = p.A[(int64_t)d * N + 2 * k] * LOG2E;
        A2[k].y = p.A[(int64_t)d * N + 2 * k + 1] * LOG2E;
    }
    const float Dv = p.D ? p.D[d] : 0.0f;
    const float bias = p.delta_bias ? p.delta_bias[d] : 0.0f;
    // the parameter gradients: per lane, across every segment
    f32x2 dA[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) dA[k] = (f32x2){0.f, 0.f};
    float dD_acc = 0.f, dbias_acc = 0.f;

    // LONG: the sequence in segments of G tokens, LAST segment first (header comment); every wave runs every segment and meets
    // every barrier
    const int nseg = LONG ? (L + G - 1) / G : 1;        // workgroup-uniform
#pragma nounroll
    for (int g = nseg - 1; g >= 0; --g) {
    const int l0 = g * G + c * LC;
    const int nl = (L - l0 < LC) ? ((L - l0 > 0) ? L - l0 : 0) : LC;              // steps of this chunk (0 for waves past the end)

    // B/C rows of the chunk -> wave-private LDS slab
    if constexpr (LONG) {                                // the same rows through buffer addressing, WAVE / N rows of B and of C per trip:
        constexpr int RPT = WAVE / N;                    // the per-lane part is rebuilt from the lane index in every segment, so the
        static_assert(LC % RPT == 0, "slab copy: whole rows per trip");           // loop keeps no 64-bit pointers live across pass 2
        int ln = lane;
        asm volatile("" : "+v"(ln));                     // (opaque per segment: hoisted out of the loop, jr is spilled instead)
        const int jr = ln / N, cc = ln % N;
#pragma unroll
        for (int j = 0; j < LC; j += RPT) {
            const int l = (l0 + j + jr < L) ? l0 + j + jr : L - 1;
            bc_lds[c][j + jr][cc] = bio<TBC>::ld(r_B, (l * (int)p.B_sl + cc) * (int)sizeof(TBC), 0);
            bc_lds[c][j + jr][N + cc] = bio<TBC>::ld(r_C, (l * (int)p.C_sl + cc) * (int)sizeof(TBC), 0);
        }
    } else
    for (int e = lane; e < LC * 2 * N; e += WAVE) {
        const int j = e / (2 * N), cc = e % (2 * N);
        const int l = (l0 + j < L) ? l0 + j : L - 1;
        bc_lds[c][j][cc] = (cc < N) ? io<TBC>::ld(Bg + (int64_t)l * p.B_sl + cc) : io<TBC>::ld(Cg + (int64_t)l * p.C_sl + cc - N);
    }

    // inputs of one sub-chunk (SUB steps); rows past the end re-read row L-1 and only ever meet g = 0
    struct Sub { float uu[SUB], dl[SUB], zz[SUB], gg[SUB]; int zrow[SUB]; };
    auto load_sub = [&](int sc, Sub& in, bool with_u) {
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
            const int lr = l0 + sc * SUB + i;
            const int l = (lr < L) ? lr : L - 1;
            in.zrow[i] = IDX ? zidx[l] : l;
            const int orow = IDX ? oidx[l] : l;
            in.uu[i] = with_u ? bio<T>::ld(r_u, vo, l * sl_u) : 0.f;
            in.dl[i] = bio<T>::ld(r_dt, vo, l * sl_dt);
            in.zz[i] = HAS_Z ? bio<T>::ld(r_z, vo, in.zrow[i] * sl_z) : 0.f;
            in.gg[i] = bio<T>::ld(r_g, vo, orow * sl_g);
        }
    };
    auto finish_sub = [&](int sc, Sub& in) {                                      // softplus, zero gradients past the end
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
            in.dl[i] = activate_delta<DMODE>(in.dl[i], bias);
            in.gg[i] = ((l0 + sc * SUB + i) < L && active) ? in.gg[i] : 0.f;
        }
    };
    const int nsub = (nl + SUB - 1) / SUB;                                        // wave-uniform

    // ---- pass 1: bare adjoint recursion from carry = 0; total decay of the chunk -----------------------------------------
    f32x2 carry[NPL];
#pragma unroll
    for (int k = 0; k < NPL; ++k) carry[k] = (f32x2){0.f, 0.f};
    float sd = 0.f;
    for (int sc = nsub - 1; sc >= 0; --sc) {
        Sub in;
        load_sub(sc, in, false);
        finish_sub(sc, in);
#pragma unroll
        for (int i = SUB - 1; i >= 0; --i) {
            const bool valid = (l0 + sc * SUB + i) < L;                           // wave-uniform
            const float dlo = valid ? in.dl[i] : 0.f;                              // steps past the end: decay 1, no contribution
            sd += dlo;
            float gy = in.gg[i];
            if (HAS_Z) gy *= silu_f(in.zz[i]);
            const float* crow = &bc_lds[c][sc * SUB + i][N];
            const float a_sh = decay_shared<ASH>(A2[0], dlo);
#pragma unroll
            for (int k = 0; k < NPL; ++k) carry_only_pair(carry[k], decay_pair<ASH>(A2[k], dlo, a_sh), (f32x2){crow[2 * k], crow[2 * k + 1]}, gy);
        }
    }
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        const f32x2 t = A2[k] * sd;
        xch_lds[c][0][2 * k][lane] = carry[k].x;
        xch_lds[c][0][2 * k + 1][lane] = carry[k].y;
        xch_lds[c][1][2 * k][lane] = fast_exp2(t.x);
        xch_lds[c][1][2 * k + 1][lane] = fast_exp2(t.y);
    }
    __syncthreads();
    // ---- combine: the carry entering this chunk from the right, folded from the one entering the segment (0 in the last) -----
    if (LONG && g + 1 < nseg) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            carry[k].x = carry_lds[g & 1][2 * k][lane];
            carry[k].y = carry_lds[g & 1][2 * k + 1][lane];
        }
    } else {
#pragma unroll
        for (int k = 0; k < NPL; ++k) carry[k] = (f32x2){0.f, 0.f};
    }
    for (int j = NW - 1; j > c; --j) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            f32x2 cl, q;
            cl.x = xch_lds[j][0][2 * k][lane];
            cl.y = xch_lds[j][0][2 * k + 1][lane];
            q.x = xch_lds[j][1][2 * k][lane];
            q.y = xch_lds[j][1][2 * k + 1][lane];
            carry[k] = q * carry[k] + cl;
        }
    }
    // the same fold continued over chunk 0 is the carry entering the next segment to the left: wave 0, whose fold ends there,
    // completes it and leaves it in LDS.  Two buffers alternate, because wave 0 writes the next one while the others may still
    // read this one.  The barrier keeps the next publish (LONG) or the parameter-gradient partials (after the last segment
    // walked) behind every wave's reads of xch_lds.
    if (LONG && g > 0 && c == 0) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            carry_lds[(g + 1) & 1][2 * k][lane] = xch_lds[0][1][2 * k][lane] * carry[k].x + xch_lds[0][0][2 * k][lane];
            carry_lds[(g + 1) & 1][2 * k + 1][lane] = xch_lds[0][1][2 * k + 1][lane] * carry[k].y + xch_lds[0][0][2 * k + 1][lane];
        }
    }
    __syncthreads();

    // ---- pass 2: the full backward of the chunk from the true carry ----------------------------------------------------------
    u32x4_t sel_lo, sel_hi;
    if (MFMA_RED) mfma_selectors(lane, sel_lo, sel_hi);

    auto load_state = [&](int ci, uint32_t(&w)[H0W]) {                            // ci = global sub-chunk index (K2's convention)
        const int slot = ckpt_slot(ci, L);
        if (slot < 0) {
#pragma unroll
            for (int k = 0; k < H0W; ++k) w[k] = 0u;
        } else {
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                if constexpr (CK_PACKED) {
                    if (k % 4 == 0) {                            // [chunk][N/8][d][4 words]: 16 bytes at a time
                        const u32x4_t qv = __builtin_amdgcn_raw_buffer_load_b128(r_ck, vo_ck * 4, (slot * (N / 8) + k / 4) * p.dim * 16, 0);
                        w[k] = qv[0]; w[k + 1] = qv[1]; w[k + 2] = qv[2]; w[k + 3] = qv[3];
                    }
                } else {
                    w[2 * k] = __builtin_amdgcn_raw_buffer_load_b32(r_ck, vo_ck, ((slot * N + 2 * k) * p.dim) * 4, 0);
                    w[2 * k + 1] = __builtin_amdgcn_raw_buffer_load_b32(r_ck, vo_ck, ((slot * N + 2 * k + 1) * p.dim) * 4, 0);
                }
            }
        }
    };
    for (int sc = nsub - 1; sc >= 0; --sc) {
        const int ci = l0 / SUB + sc;
        Sub in;
        load_sub(sc, in, true);
        uint32_t w0[H0W], w1[H0W];
        load_state(ci, w0);                                                       // state entering the sub-chunk
        load_state(ci + 1, w1);                                                   // state after its last step (= the next checkpoint, or slot 0)
        finish_sub(sc, in);
        f32x2 h[NPL], hs[SUB][NPL];
        unpack_ckpt<CK_PACKED>(h, w0, 0);
#pragma unroll
        for (int i = 0; i < SUB; ++i) {                                           // recompute: hs[i] = state before step sc*SUB + i
#pragma unroll
            for (int k = 0; k < NPL; ++k) hs[i][k] = h[k];
            if (i < SUB - 1) {
                const float* brow = &bc_lds[c][sc * SUB + i][0];
                const float dlo = in.dl[i];
                const float du = dlo * in.uu[i];
                const float a_sh = decay_shared<ASH>(A2[0], dlo);
#pragma unroll
                for (int k = 0; k < NPL; ++k) recompute_pair(h[k], decay_pair<ASH>(A2[k], dlo, a_sh), (f32x2){brow[2 * k], brow[2 * k + 1]}, du);
            }
        }
        unpack_ckpt<CK_PACKED>(h, w1, 0);
        // a partial last sub-chunk (L not a multiple of SUB): the state after its last VALID step is slot 0; the steps past the
        // end are exact no-ops (g = 0), and the states "before" them are never multiplied with a non-zero gradient
#pragma unroll
        for (int i = SUB - 1; i >= 0; --i) {
            const int lraw = l0 + sc * SUB + i;
            const bool valid = lraw < L;                                          // wave-uniform
            const int l = valid ? lraw : L - 1;
            const float* brow = &bc_lds[c][sc * SUB + i][0];
            const float g = in.gg[i];
            float sz;
            const float gy = gate_gy<HAS_Z>(g, in.zz[i], sz);
            const float dlo = in.dl[i];
            const float du = dlo * in.uu[i];
            const float a_rev = decay_shared<ASH>(A2[0], dlo);
            f32x2 yp2 = (f32x2){0.f, 0.f}, GB2 = (f32x2){0.f, 0.f}, dlA2 = (f32x2){0.f, 0.f};
            float red[M];
            uint32_t pk_all[M / 2];
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const f32x2 bb = {brow[2 * k], brow[2 * k + 1]}, cc = {brow[N + 2 * k], brow[N + 2 * k + 1]};
                const f32x2 a = decay_pair<ASH>(A2[k], dlo, a_rev);
                f32x2 dBp, dCp;                                                   // (steps past the end: g = 0 and carry = 0, exact no-ops)
                adjoint_pair<HAS_Z, false>(h[k], hs[i][k], carry[k], dA[k], yp2, GB2, dlA2, A2[k], a, bb, cc, gy, du, dlo, dBp, dCp);
                if constexpr (MFMA_RED) {
                    pk_all[k] = pack_bf16(dBp);
                    pk_all[NPL + k] = pack_bf16(dCp);
                } else {
                    red[2 * k] = dBp.x;
                    red[2 * k + 1] = dBp.y;
                    red[N + 2 * k] = dCp.x;
                    red[N + 2 * k + 1] = dCp.y;
                }
            }
            float ddl, duv, ypre, dDi;
            step_outputs<DMODE, 1>(yp2, GB2, dlA2, in.uu[i], dlo, gy, Dv, ddl, duv, ypre, dDi);
            dD_acc += dDi;
            dbias_acc += ddl;
            if (valid && active) {
                bio<T>::st(r_du, vo, l * sl_du, duv);
                bio<T>::st(r_ddt, vo, l * sl_ddt, ddl);
                if (HAS_Z) {
                    const float dzv = gate_grad(g, ypre, in.zz[i], sz);
                    bio<T>::st(r_dz, vo, in.zrow[i] * sl_dz, dzv);
                }
            }
            // ---- dB/dC of this step: finish the 64-lane sum inside the wave, one partial row per (step, 64 channels) ----
            float* const prow = p.dBC_partial + (((int64_t)s * L + l) * nwg + blockIdx.x) * (2 * N);
            if constexpr (MFMA_RED) {
#pragma unroll
                for (int g16 = 0; g16 < M / 16; ++g16) {                          // g16 = 0: dB, 1: dC;  register r of lane l = value 4*(l>>4) + r
                    f32x4 dsum = group_sum16(sel_lo, sel_hi, pk_all + 8 * g16);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dsum[r] = row_sum_dpp(dsum[r]);
                    if (valid && (lane & 15) == 0) *reinterpret_cast<f32x4*>(prow + g16 * N + 4 * (lane >> 4)) = dsum;
                }
            } else {
                lane_group_reduce<M>(red);                                        // register i = value 4*i + 2*b4 + b5
#pragma unroll
                for (int i8 = 0; i8 < M / 4; ++i8) {
                    const float tot = row_sum_dpp(red[i8]);
                    if (valid && (lane & 15) == 0) prow[4 * i8 + 2 * ((lane >> 4) & 1) + (lane >> 5)] = tot;
                }
            }
        }
    }
    }   // segments
    // ---- dA / dD / dbias: the NW waves of a (sequence, 64 channels) meet in LDS ------------------------------------------------
    // LONG: the lane index and what follows from it are rebuilt here from the lane count, an expression the compiler does not
    // merge with the prologue's, so that no value used only down here is kept (spilled) across the segment loop
    const int lane_e = LONG ? (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : lane;
    const int d_e = LONG ? (int)(blockIdx.x * WAVE) + lane_e : d;
    const bool active_e = LONG ? d_e < p.dim : active;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
        xch_lds[c][0][2 * k][lane_e] = dA[k].x;
        xch_lds[c][0][2 * k + 1][lane_e] = dA[k].y;
    }
    xch_lds[c][0][N][lane_e] = dD_acc;
    xch_lds[c][0][N + 1][lane_e] = dbias_acc;
    __syncthreads();
    if (c == 0 && active_e) {
        const int64_t pss_a = p.part_ss ? p.part_ss : (int64_t)p.dim * N, pss_d = p.part_ss ? p.part_ss : (int64_t)p.dim;
        float* dAp = p.dA_partial + (int64_t)s * pss_a + (int64_t)d_e * N;
#pragma unroll
        for (int n = 0; n < N + 2; ++n) {
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) acc += xch_lds[w][0][n][lane_e];
            if (n < N) dAp[n] = acc;
            else if (n == N) { if (p.dD_partial) p.dD_partial[(int64_t)s * pss_d + d_e] = acc; }
            else { if (p.dbias_partial) p.dbias_partial[(int64_t)s * pss_d + d_e] = acc; }
        }
    }
}

// Launch-size rule shared by the kernel dispatch and the host (which sizes the dB/dC partial rows: one per 64 channels here,
// one per 256 for the sequential kernel).  Measured break-even is near 250 workgroup-waves; the LDS footprint allows one
// workgroup per CU.
constexpr int BWD_CHUNKED_NW = 7, BWD_CHUNKED_LC_LONG = 28, BWD_CHUNKED_LC_SHORT = 8;
constexpr int BWD_CHUNKED_G = BWD_CHUNKED_NW * BWD_CHUNKED_LC_LONG;      // up to here a launch is one segment; longer ones take the LONG form ...
constexpr int BWD_CHUNKED_LC_SEG = 28;                                   // ... at 7 waves x 28 steps per segment
constexpr int BWD_CHUNKED_G_SEG = BWD_CHUNKED_NW * BWD_CHUNKED_LC_SEG;
constexpr int BWD_CHUNKED_MAXL = 1024;                                   // 512-pixel images at patch 2
constexpr int BWD_CHUNKED_WAVES = 512;                                   // nseq * ceil(dim / 64) up to which L <= 196 is routed here
// the same for 196 < L <= 1024, set by the project's routing rule (routed only where the kernel alone reaches 1.1 x the sequential
// one) from profiles/scan_bwd_chunked_long.json (bf16, hoisted call pattern, dim 1024 / 2048; one workgroup per CU, so the time
// steps at every 256 workgroups): 1.96-2.07 x at L 256 and 2.29-2.48 x at L 1024 up to 240 channel-waves; at 384-480 1.03-1.04 x at
// L 256 and 1.16-1.17 x at L 1024; 0.71-0.79 x at 768.  The second round of workgroups is therefore left to the sequential kernel
// at every length past 196 (at 1024 tokens alone it would pass the rule); larger launches remain reachable through
// DM_FLAG_SCAN_CHUNKED.
constexpr int BWD_CHUNKED_WAVES_SEG = 256;
// steps per chunk of the instantiation taken, 0 for the sequential kernel
static inline int bwd_chunked_lc(int nseq, int dim, int seqlen, int dstate, int flags) {
    const int forced = (flags & DM_FLAG_SCAN_SEQUENTIAL) ? 0 : ((flags & DM_FLAG_SCAN_CHUNKED) ? 1 : -1);
    if (forced == 0 || dstate != 16) return 0;
    const int64_t waves = (int64_t)nseq * ((dim + WAVE - 1) / WAVE);
    if (!(waves <= (seqlen > BWD_CHUNKED_G ? BWD_CHUNKED_WAVES_SEG : BWD_CHUNKED_WAVES) || forced == 1)) return 0;
    if (seqlen > BWD_CHUNKED_G && seqlen <= BWD_CHUNKED_MAXL) return BWD_CHUNKED_LC_SEG;
    if (seqlen > 2 * BWD_CHUNKED_LC_LONG && seqlen <= BWD_CHUNKED_G) return BWD_CHUNKED_LC_LONG;
    if (seqlen > 2 * BWD_CHUNKED_LC_SHORT && seqlen <= BWD_CHUNKED_NW * BWD_CHUNKED_LC_SHORT) return BWD_CHUNKED_LC_SHORT;
    return 0;
}
// dm_scan_bwd_launch_segment: tokens per segment of the instantiation a launch of this size takes, 0 for the sequential kernel
static inline int bwd_chunked_segment(int nseq, int dim, int seqlen, int dstate, int flags) {
    return BWD_CHUNKED_NW * bwd_chunked_lc(nseq, dim, seqlen, dstate, flags);
}
// steps per chunk if the launch goes to this family -- the one backward scan that takes two argument structs (bwd_dispatch, and
// the pairing rule of dm_selective_scan_bwd_n through scan_bwd_takes_two) -- else 0
static inline int bwd_goes_chunked(const dm_scan_bwd_args& a) {
    return (a.bc_dtype == DM_F32 || a.bc_dtype == a.io_dtype) ? bwd_chunked_lc(a.nseq, a.dim, a.seqlen, a.dstate, a.flags) : 0;
}

template <typename T, typename TBC, bool HAS_Z, bool IDX, int LC, bool LONG>
static void launch_bwd_chunked3(const dm_scan_bwd_args& a, const dm_scan_bwd_args* second, hipStream_t st) {
    unsigned gz;
    const mix_args<dm_scan_bwd_args> m = mix_make(a, second, gz);
    dim3 grid((a.dim + WAVE - 1) / WAVE, a.nseq, gz), block(WAVE * BWD_CHUNKED_NW);
    with_bwd_variant<16, HAS_Z, IDX>(a.flags, [&](auto dmode, auto ash) {
        hipLaunchKernelGGL((scan_bwd_chunked_kernel<T, TBC, HAS_Z, IDX, dmode.value, BWD_CHUNKED_NW, LC, ash.value, LONG>), grid, block, 0, st, m);
    });
}

template <typename T, typename TBC>
static int launch_bwd_chunked(const dm_scan_bwd_args& a, const dm_scan_bwd_args* second, hipStream_t st, int lc) {
    with_z_idx(a, [&](auto hz, auto ix) {
        if (a.seqlen > BWD_CHUNKED_G) launch_bwd_chunked3<T, TBC, hz.value, ix.value, BWD_CHUNKED_LC_SEG, true>(a, second, st);
        else if (lc == BWD_CHUNKED_LC_LONG) launch_bwd_chunked3<T, TBC, hz.value, ix.value, BWD_CHUNKED_LC_LONG, false>(a, second, st);
        else launch_bwd_chunked3<T, TBC, hz.value, ix.value, BWD_CHUNKED_LC_SHORT, false>(a, second, st);
    });
    return launch_status("dm_selective_scan_bwd (chunked)");
}

template <typename T>
static int bwd_dispatch(const dm_scan_bwd_args& a, const dm_scan_bwd_args* second, hipStream_t st) {
    const int lc = bwd_goes_chunked(a);
    if (lc > 0) return a.bc_dtype == DM_F32 ? launch_bwd_chunked<T, float>(a, second, st, lc) : launch_bwd_chunked<T, T>(a, second, st, lc);
    if (second) { set_error("dm_selective_scan_bwd: the sequential kernel takes one argument struct"); return DM_ERR_ARG; }
    return bwd_dispatch_bc<T>(a, st);
}

}  // namespace dm
