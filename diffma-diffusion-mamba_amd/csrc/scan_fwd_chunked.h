#pragma once
// K1c  chunk-parallel forward scan for SMALL launches (sampling and graphed small-batch training at batch 1..~10).
//
// The sequential kernel (scan_fwd_impl.h) needs nseq * dim/64 >= ~2000 waves to fill the chip; a p_sample step at
// batch 8 launches 384, and every launch then costs the full 196-step dependent chain (~70 us, 38 % of a
// graph-replayed step).  Here the time axis is cut into NW chunks, one WAVE per chunk inside a workgroup that owns
// (sequence, 64 channels):
//   pass 1  every wave runs the recurrence over its LC steps from h = 0 (no C, no z, no output) and publishes, per
//           state, its local end state and the chunk's total decay  P = exp(A * sum(delta))          -> LDS
//   combine after one barrier wave c folds the chunks before it:  H <- P_j * H + h_j ,  j = 0 .. c-1   (16 FMAs per chunk)
//   pass 2  every wave re-runs its chunk from the true entry state H and writes the gated outputs.
// The dependent chain is (0.75 + 1) * L/NW steps instead of L at 1.75x the arithmetic -- the trade the north star's
// "wavefront-parallel scan" asks for, taken only where latency (not throughput) is the limit.  Inputs of the chunk
// stay in registers between the passes; B/C rows of the chunk sit in a wave-private LDS slab.
//
// LONG (196 < L <= 1024: the 256- and 512-pixel image sizes at patch 2) puts a segment loop around that body.  The workgroup walks
// the sequence in segments of G = NW * LC tokens; within a segment wave c owns LC consecutive steps as above, and its local end
// state is still computed from zero.  The fold starts from the state entering the segment instead of 0, and the same fold continued
// over all NW chunks is the state entering the next segment.  Only the last wave's fold ends there, so it completes it and leaves
// the result in LDS (carry_lds, two buffers alternating), where every wave picks it up after the next publish barrier: carried in
// registers by every wave it costs 16 VGPRs across both passes and spilled in all 60 instantiations.  The segment count is
// workgroup-uniform: every wave runs every segment and meets every barrier; a wave whose chunk is empty has nl = 0 (decay 1, input
// 0, no stores).  A second barrier per segment separates the last fold read of xch_lds from the next segment's publish (two xch
// buffers would need 224 KB); the B/C slab stays wave-private.  Outputs and checkpoints use the global step index, so a training
// forward writes exactly what K2 reads.  Launches with L <= 196 are the one-segment instantiations, unchanged.
//
// Resources per instantiation (gfx950, tools/kernel_regs.sh scan_fwd_<dtype> chunked; 896 threads: 128 VGPRs per wave, 160 KB LDS):
//                                         one segment (14 x 14, 60 kernels)      LONG (14 x 10, 60 kernels)
//   VGPRs  no z                           102-106                                106
//          z, 16-bit I/O                  104-124                                112-120
//          z, fp32 I/O                    104-116                                112-116
//   LDS                                   139 776 B                              140 800 B (slab 17 920 + xch 114 688 + carry 8 192)
//   scratch / spilled VGPRs               0 / 0                                  0 / 0
// LONG at 14 x 14 needs 128 VGPRs and spills up to 7 more in the gated 16-bit instantiations; at 14 x 10 two segments still cover 256
// tokens and eight cover 1024 (six at 14 x 14, each 8 steps longer).
#include <cstdlib>
#include "scan_fwd_impl.h"

namespace dm {

template <typename T, typename TBC, int N, bool HAS_Z, bool IDX, bool SOFTPLUS, int NW, int LC, bool ASH = false, bool CKPT = false, bool LONG = false>
__global__ __launch_bounds__(64 * NW) void scan_fwd_chunked_kernel(const mix_args<dm_scan_fwd_args> pm) {
    const dm_scan_fwd_args& p = pm.a[blockIdx.z];      // grid.z = congruent launches sharing this one (the two mixers of a block)
    constexpr int NP = N / 2;
    constexpr int ES = (int)sizeof(T);
    constexpr int G = NW * LC;                          // tokens per segment
    __shared__ __attribute__((aligned(16))) float bc_lds[NW][LC][2 * N];      // [B row | C row] of every step of the wave's chunk
    __shared__ float xch_lds[NW][2][N][WAVE];                                   // [chunk][P | h_end][state][lane]
    __shared__ float carry_lds[LONG ? 2 : 1][LONG ? N : 1][WAVE];               // LONG: [segment parity][state][lane]
    const int lane = threadIdx.x & 63;
    const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);             // wave = chunk index (kept scalar)
    const int d_raw = blockIdx.x * WAVE + lane;
    const int d = (d_raw < p.dim) ? d_raw : p.dim - 1;                          // lanes past the end shadow the last channel
    const int s = blockIdx.y;
    const int L = p.seqlen;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int grp = (blockIdx.x * WAVE) / (p.dim / p.ngroups);
    const rsrc_t r_u = make_rsrc((const T*)p.u + (int64_t)s * p.u_ss);
    const rsrc_t r_dt = make_rsrc((const T*)p.delta + (int64_t)s * p.dt_ss);
    const rsrc_t r_z = make_rsrc(HAS_Z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_o = make_rsrc((T*)p.out + (int64_t)s * p.o_ss);
    const int vo = d * ES;
    const int sl_u = (int)p.u_sl * ES, sl_dt = (int)p.dt_sl * ES, sl_z = (int)p.z_sl * ES, sl_o = (int)p.o_sl * ES;
    const cptr<int32_t> zidx = IDX ? as_const(p.z_row_index + (int64_t)dir * L) : nullptr;
    const cptr<int32_t> oidx = IDX ? as_const(p.out_row_index + (int64_t)dir * L) : nullptr;
    const TBC* __restrict__ Bg = (const TBC*)p.B + (int64_t)s * p.B_ss + (int64_t)grp * p.B_sg;
    const TBC* __restrict__ Cg = (const TBC*)p.C + (int64_t)s * p.C_ss + (int64_t)grp * p.C_sg;
    constexpr bool CK_PACKED = std::is_same<T, bf16_t>::value;
    constexpr int CK_ROWS = CK_PACKED ? NP : N;
    const int nck = (L + DM_SCAN_CKPT_EVERY - 1) / DM_SCAN_CKPT_EVERY;
    const rsrc_t r_ck = make_rsrc(CKPT ? (const uint32_t*)p.ckpt + (int64_t)s * nck * CK_ROWS * p.dim : nullptr);
    f32x2 A2[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        A2[k].x = p.A[(int64_t)d * N + 2 * k] * LOG2E;
        A2[k].y = p.A[(int64_t)d * N + 2 * k + 1] * LOG2E;
    }
    const float Dv = p.D ? p.D[d] : 0.0f;
    const float bias = p.delta_bias ? p.delta_bias[d] : 0.0f;

    // LONG: the sequence in segments of G tokens (header comment); every wave runs every segment and meets every barrier
    const int nseg = LONG ? (L + G - 1) / G : 1;        // workgroup-uniform
#pragma nounroll
    for (int g = 0; g < nseg; ++g) {
    const int l0 = g * G + c * LC;
    const int nl = (L - l0 < LC) ? ((L - l0 > 0) ? L - l0 : 0) : LC;            // steps of this chunk (0 for waves past the end)

    // ---- this chunk's inputs: requested up front, kept in registers for both passes ------------------------------
    float uu[LC], dl[LC], zz[LC];
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        const int l = (l0 + j < L) ? l0 + j : L - 1;
        uu[j] = bio<T>::ld(r_u, vo, l * sl_u);
        dl[j] = bio<T>::ld(r_dt, vo, l * sl_dt);
        zz[j] = HAS_Z ? bio<T>::ld(r_z, vo, (IDX ? zidx[l] : l) * sl_z) : 0.0f;
    }
    // B/C rows of the chunk -> wave-private LDS slab (LC*2N values, cooperatively)
    if constexpr (LONG) {                                // the same rows; lane-constant address parts named, so that the segment loop
        constexpr int RPT = WAVE / (2 * N);              // keeps two pointers live across it instead of one per trip (rows per trip)
        static_assert(WAVE % (2 * N) == 0 && LC % RPT == 0, "slab copy: whole rows per trip");
        const int jh = lane / (2 * N), cc = lane % (2 * N);
        const TBC* __restrict__ src = (cc < N) ? Bg + cc : Cg + cc - N;
        const int64_t src_sl = (cc < N) ? p.B_sl : p.C_sl;
#pragma unroll
        for (int j = 0; j < LC; j += RPT) {
            const int l = (l0 + j + jh < L) ? l0 + j + jh : L - 1;
            bc_lds[c][j + jh][cc] = io<TBC>::ld(src + l * src_sl);
        }
    } else
    for (int e = lane; e < LC * 2 * N; e += WAVE) {
        const int j = e / (2 * N), cc = e % (2 * N);
        const int l = (l0 + j < L) ? l0 + j : L - 1;
        bc_lds[c][j][cc] = (cc < N) ? io<TBC>::ld(Bg + (int64_t)l * p.B_sl + cc) : io<TBC>::ld(Cg + (int64_t)l * p.C_sl + cc - N);
    }
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        float x = dl[j] + bias;
        if (SOFTPLUS) x = softplus_f(x);
        dl[j] = (j < nl) ? x : 0.0f;                     // steps past the end: decay 1, input 0 => exact no-ops
        uu[j] = (j < nl) ? uu[j] : 0.0f;
    }

    // ---- pass 1: local end state and total decay ------------------------------------------------------------------
    f32x2 h[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) h[k] = (f32x2){0.0f, 0.0f};
    float sd = 0.0f;
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        const float du = dl[j] * uu[j];
        sd += dl[j];
        float a_sh = 0.0f;
        if (ASH) a_sh = fast_exp2(A2[0].x * dl[j]);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            f32x2 a, bb;
            if (ASH) {
                a = (f32x2){a_sh, a_sh};
            } else {
                const f32x2 t = A2[k] * dl[j];
                a.x = fast_exp2(t.x);
                a.y = fast_exp2(t.y);
            }
            bb.x = bc_lds[c][j][2 * k];
            bb.y = bc_lds[c][j][2 * k + 1];
            h[k] = a * h[k] + bb * du;
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const f32x2 t = A2[k] * sd;
        xch_lds[c][0][2 * k][lane] = fast_exp2(t.x);
        xch_lds[c][0][2 * k + 1][lane] = fast_exp2(t.y);
        xch_lds[c][1][2 * k][lane] = h[k].x;
        xch_lds[c][1][2 * k + 1][lane] = h[k].y;
    }
    __syncthreads();

    // ---- combine: the state entering this chunk, folded from the state entering the segment (0 in the first) -------------
    if (LONG && g > 0) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            h[k].x = carry_lds[g & 1][2 * k][lane];
            h[k].y = carry_lds[g & 1][2 * k + 1][lane];
        }
    } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) h[k] = (f32x2){0.0f, 0.0f};
    }
    for (int j = 0; j < c; ++j) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            f32x2 pj, hj;
            pj.x = xch_lds[j][0][2 * k][lane];
            pj.y = xch_lds[j][0][2 * k + 1][lane];
            hj.x = xch_lds[j][1][2 * k][lane];
            hj.y = xch_lds[j][1][2 * k + 1][lane];
            h[k] = pj * h[k] + hj;
        }
    }
    // the same fold continued over the last chunk is the state entering the next segment: the last wave publishes it.  The second
    // barrier keeps the next segment's publish behind every wave's reads of this one (two xch buffers would need 224 KB); the carry
    // alternates between two buffers because the last wave writes the next one while the others may still read this one.
    if (LONG && g + 1 < nseg) {
        if (c == NW - 1) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                carry_lds[(g + 1) & 1][2 * k][lane] = xch_lds[c][0][2 * k][lane] * h[k].x + xch_lds[c][1][2 * k][lane];
                carry_lds[(g + 1) & 1][2 * k + 1][lane] = xch_lds[c][0][2 * k + 1][lane] * h[k].y + xch_lds[c][1][2 * k + 1][lane];
            }
        }
        __syncthreads();
    }

    // ---- pass 2: the chunk again from its true entry state, with outputs ----------------------------------------------
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        if (j < nl) {                                    // wave-uniform
            const int l = l0 + j;
            float Bc[N], Cc[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                Bc[k] = bc_lds[c][j][k];
                Cc[k] = bc_lds[c][j][N + k];
            }
            const float y = scan_step<N, HAS_Z, false, ASH>(h, A2, Bc, Cc, uu[j], dl[j], zz[j], Dv, 0.0f);
            bio<T>::st(r_o, vo, (IDX ? oidx[l] : l) * sl_o, y);
            if (CKPT && ((l + 1) % DM_SCAN_CKPT_EVERY == 0 || l + 1 == L)) {       // training: the state entering every 4-step chunk (wave-uniform);
                const int ci = (l + 1 < L) ? (l + 1) / DM_SCAN_CKPT_EVERY : 0;      // slot 0 = the state after the last step
                if constexpr (CK_PACKED) {                               // [chunk][N/8][d][4 words], see scan_fwd_impl.h
                    uint32_t w[NP];
#pragma unroll
                    for (int k = 0; k < NP; ++k) asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w[k]) : "v"(h[k].x), "v"(h[k].y));
                    bio_st_words<NP>(w, r_ck, d * 16, ci * p.dim * NP * 4, p.dim * 16);
                } else {
#pragma unroll
                    for (int k = 0; k < NP; ++k) {
                        bio<float>::st(r_ck, d * 4, ((ci * N + 2 * k) * p.dim) * 4, h[k].x);
                        bio<float>::st(r_ck, d * 4, ((ci * N + 2 * k + 1) * p.dim) * 4, h[k].y);
                    }
                }
            }
        }
    }
    }   // segments
}

constexpr int CHUNKED_NW = 14, CHUNKED_LC = 14;          // 14 waves x 14 steps: one segment covers L <= 196 (DiffMa's 14x14 token grid)
constexpr int CHUNKED_G = CHUNKED_NW * CHUNKED_LC;       // longer launches take the LONG form (segment loop) ...
constexpr int CHUNKED_LC_LONG = 10;                      // ... at 14 waves x 10 steps: the loop's live values cost ~12 VGPRs (table above)
constexpr int CHUNKED_G_LONG = CHUNKED_NW * CHUNKED_LC_LONG;
constexpr int CHUNKED_MAXL = 1024;                       // 512-pixel images at patch 2
constexpr int CHUNKED_WAVES = 512;                       // nseq * ceil(dim / 64) up to which L <= 196 is routed here
// the same for 196 < L <= 1024, set by the project's routing rule (routed only where it reaches 1.1 x the sequential kernel) from
// profiles/scan_fwd_chunked_long.json (bf16, hoisted call pattern, dim 1024 / 2048, L 256 / 1024; one workgroup per CU, so the time
// steps at every 256 workgroups): 1.8-2.3 x up to 240, without checkpoints 1.18-1.22 x at 288-480 and 1.02-1.06 x at 576, with
// checkpoints 1.01-1.08 x at 288-480.  Larger launches remain reachable through DM_FLAG_SCAN_CHUNKED.
constexpr int CHUNKED_WAVES_LONG = 512, CHUNKED_WAVES_LONG_CKPT = 256;

// true if the launch is small enough that latency, not throughput, is the limit (and the variant is instantiated).
// The 137 KB of LDS allow one workgroup per CU, i.e. 256 at a time: measured (bf16, dim 1024, L 196) 75 -> 24 us at
// nseq 3, 78 -> 50 us at nseq 24 (two rounds), break-even near nseq 48.
static inline bool use_chunked_fwd(const dm_scan_fwd_args& a) {
    const int forced = (a.flags & DM_FLAG_SCAN_SEQUENTIAL) ? 0 : ((a.flags & DM_FLAG_SCAN_CHUNKED) ? 1 : -1);
    if (forced == 0 || (a.flags & DM_FLAG_OUT_ACCUMULATE)) return false;
    const int64_t waves = (int64_t)a.nseq * ((a.dim + WAVE - 1) / WAVE);
    const int64_t limit = a.seqlen <= CHUNKED_G ? CHUNKED_WAVES : (a.ckpt ? CHUNKED_WAVES_LONG_CKPT : CHUNKED_WAVES_LONG);
    // checkpoints: built for the two model call patterns only (gated + softplus in the scan; gate and softplus hoisted out of it)
    if (a.ckpt && !(a.z_row_index && ((a.z && (a.flags & DM_FLAG_DELTA_SOFTPLUS)) || (!a.z && !(a.flags & DM_FLAG_DELTA_SOFTPLUS))))) return false;
    return !a.last_state && a.dstate == 16 && (waves <= limit || forced == 1) && a.seqlen > 4 * CHUNKED_NW && a.seqlen <= CHUNKED_MAXL;
}
// the launch goes to this family -- the one forward scan that takes two argument structs (dispatch_fwd, and the pairing rule of
// dm_selective_scan_fwd_n through scan_fwd_takes_two)
static inline bool fwd_goes_chunked(const dm_scan_fwd_args& a) {
    return use_chunked_fwd(a) && (a.bc_dtype == DM_F32 || a.bc_dtype == a.io_dtype);
}
// dm_scan_fwd_launch_segment: tokens per segment of the instantiation a launch of this size (no checkpoints, no last_state) takes,
// 0 for the sequential kernel
static inline int fwd_chunked_segment(int nseq, int dim, int seqlen, int dstate, int flags) {
    dm_scan_fwd_args a{};
    a.nseq = nseq, a.dim = dim, a.seqlen = seqlen, a.dstate = dstate, a.flags = flags;
    return !use_chunked_fwd(a) ? 0 : (seqlen > CHUNKED_G ? CHUNKED_G_LONG : CHUNKED_G);
}

template <typename T, typename TBC, bool HAS_Z, bool IDX, bool LONG>
static void launch_fwd_chunked2(const dm_scan_fwd_args& a, const dm_scan_fwd_args* second, hipStream_t st) {
    unsigned gz;
    const mix_args<dm_scan_fwd_args> m = mix_make(a, second, gz);
    dim3 grid((a.dim + WAVE - 1) / WAVE, a.nseq, gz), block(WAVE * CHUNKED_NW);
    const bool sp = (a.flags & DM_FLAG_DELTA_SOFTPLUS) != 0;
    constexpr int LC = LONG ? CHUNKED_LC_LONG : CHUNKED_LC;
    if constexpr (HAS_Z && IDX) {                   // the model's call pattern: also built with checkpoints (small-batch training)
        if ((a.flags & DM_FLAG_A_SHARED) && sp) {
            if (a.ckpt) hipLaunchKernelGGL((scan_fwd_chunked_kernel<T, TBC, 16, true, true, true, CHUNKED_NW, LC, true, true, LONG>), grid, block, 0, st, m);
            else hipLaunchKernelGGL((scan_fwd_chunked_kernel<T, TBC, 16, true, true, true, CHUNKED_NW, LC, true, false, LONG>), grid, block, 0, st, m);
            return;
        }
        if (a.ckpt && sp) {
            hipLaunchKernelGGL((scan_fwd_chunked_kernel<T, TBC, 16, true, true, true, CHUNKED_NW, LC, false, true, LONG>), grid, block, 0, st, m);
            return;
        }
    }
    if constexpr (!HAS_Z && IDX) {                  // hoisted gate + hoisted softplus (DM_FLAG_DELTA_ACTIVATED arrives here as "no softplus, no bias")
        if (a.ckpt && !sp) {
            hipLaunchKernelGGL((scan_fwd_chunked_kernel<T, TBC, 16, false, true, false, CHUNKED_NW, LC, false, true, LONG>), grid, block, 0, st, m);
            return;
        }
    }
    if (sp) hipLaunchKernelGGL((scan_fwd_chunked_kernel<T, TBC, 16, HAS_Z, IDX, true, CHUNKED_NW, LC, false, false, LONG>), grid, block, 0, st, m);
    else hipLaunchKernelGGL((scan_fwd_chunked_kernel<T, TBC, 16, HAS_Z, IDX, false, CHUNKED_NW, LC, false, false, LONG>), grid, block, 0, st, m);
}

template <typename T, typename TBC>
static int launch_fwd_chunked(const dm_scan_fwd_args& a, const dm_scan_fwd_args* second, hipStream_t st) {
    with_z_idx(a, [&](auto hz, auto ix) {
        if (a.seqlen > CHUNKED_G) launch_fwd_chunked2<T, TBC, hz.value, ix.value, true>(a, second, st);
        else launch_fwd_chunked2<T, TBC, hz.value, ix.value, false>(a, second, st);
    });
    return launch_status("dm_selective_scan_fwd (chunked)");
}

template <typename T>
static int dispatch_fwd(const dm_scan_fwd_args& a, const dm_scan_fwd_args* second, hipStream_t st) {
    if (fwd_goes_chunked(a)) return a.bc_dtype == DM_F32 ? launch_fwd_chunked<T, float>(a, second, st) : launch_fwd_chunked<T, T>(a, second, st);
    if (second) { set_error("dm_selective_scan_fwd: the sequential kernel takes one argument struct"); return DM_ERR_ARG; }
    return dispatch_bc<T>(a, st);
}

}  // namespace dm
