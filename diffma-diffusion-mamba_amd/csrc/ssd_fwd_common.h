// What the three SSD forward kernels (ssd.hip: ssd_fwd_kernel at d_state 16 and ssd_fwd_wide_kernel at 32 / 64 / 128, both one
// chunk; ssd_chunked.hip: ssd_fwd_chunked_kernel, all four widths past one chunk) share: the tile geometry, and the body of a
// wave's (head, 32-column half) over `len` rows that start at row `base` of the sequence (one chunk: base 0, len L) --
//     sf_x_issue                  the clamped 16-byte X row loads                                                         (wide)
//     sf_stage_bc                 the workgroup's raw B / C rows into LDS                                                 (wide)
//     sf_x_frags                  X rows -> B-operand fragments of the output product, keys in accumulator order          (all three)
//     sf_gate_issue               the gate tile of a query tile, by 16-byte pieces or by dwords      (all three; d_state 16: the 16-byte arm only)
//     sf_scores, sf_offdiag       a key tile strictly before the query tile: gamma dt . alpha delta on the accumulator    (wide, chunked)
//     sf_diag                     the diagonal tile: [dt .] exp2(s2_l - s2_i) and the causal mask on the accumulator     (all three)
//     sf_times_x                  the packed score tile times the resident X fragments                                   (all three)
//     sf_epilogue                 + D x, gate, 16-bit turn through the staging tile, scatter through the row table        (all three)
// and the host-side checks of both entry points (ssd_fwd_check).  Lane roles, the same in every block: col = lane & 31 and
// kh = lane >> 5 in a fragment, trow = lane >> 1 and thf = lane & 1 (row of the tile, 16-channel half of it) when staging.
//
// What stays in each kernel: the per-position tables and their prefix sums (Hillis-Steele through LDS over 224 / 256 entries in
// ssd.hip, a shuffle scan over 128 with two more tables in ssd_chunked.hip), how waves of heads past nheads leave, the d_state 16
// kernel's score products (dt and gamma are folded into its 16-bit B rows, alpha into its C rows, both held in registers), and
// the inter-chunk term and the state update of ssd_chunked.hip.
//
// The front of global loads (sf_x_issue, sf_stage_bc) is shared by the wide kernel only.  The chunked kernel keeps the same text in
// its chunk loop (2 pieces in flight per thread where the wide kernel has 4) and the d_state 16 kernel keeps its X loads interleaved
// with its B loads: as inlined functions they give the same bits and the same instruction counts, but the loads go out in another
// order and the kernels ran slower than the parent build by more than the session's parent-against-parent spread plus one point
// (chunked: 2 - 7 % at d_state 128 and 1 - 2 % at d_state 64, L 256 and 1024; d_state 16: 2 % at nseq 24).  The wide kernel is the
// other way round: 1 % slower than the parent at d_state 32, nseq 768, with the functions, 2 - 3 % with the kernel text.
// profiles/ssd_fwd_one_body.json has every table, the per-block restore runs included.
//
// No block is left out for its bits: as inlined functions the blocks give the outputs of the kernel text they replace bit for bit
// (tools/ssd_fwd_same_bits.py: 128 cases over the three kernels, both dtypes, with / without a gate and with the dword gate), no
// instantiation spills, and every one stays at two waves per SIMD (tools/kernel_regs.sh ssd, ssd_chunked).  None of them has a
// sum of two products, the spot where inlining moved an fma in the backward (ssd_bwd_common.h): the weights are products only,
// and `yacc + Dh * xv` is one product and one sum wherever it stands.
#pragma once
#include "dm_mfma.h"

namespace dm {

constexpr int SSD_TILE = 32;
constexpr int SSD_PITCH = 20;                                  // dwords per staged tile row (32 channels = 16 dwords, +4 pad)
constexpr int ssd_bc_pitch(int nk) { return 32 * nk + 16; }    // bytes per staged B / C row: an odd number of 16-byte pieces

// The clamped 16-byte X row loads of NT tiles; cb: byte offset of this lane's 16 staged channels in a row.  Rows past the end are
// clamped here and zeroed in sf_x_frags.
template <int NT>
__device__ __forceinline__ void sf_x_issue(u32x4_t (&xq)[NT][2], const rsrc_t& r_x, int sl_x, int cb, int base, int len, int lane) {
    const int trow = lane >> 1;
#pragma unroll
    for (int it = 0; it < NT; ++it) {
        const int i = SSD_TILE * it + trow;
        const int ic = base + (i < len ? i : len - 1);
#pragma unroll
        for (int q = 0; q < 2; ++q) xq[it][q] = ld16(r_x, ic * sl_x + cb + 16 * q);
    }
}

// The share of thread tid among nthr of `rows` (a multiple of 32) raw B / C rows of d_state 16 NK into LDS, U pieces in flight per
// thread: loads first, stores after.  Rows past the end are staged as copies of the last row.
template <int NK, int U>
__device__ __forceinline__ void sf_stage_bc(uint8_t* Bl, uint8_t* Cl, const rsrc_t& r_B, const rsrc_t& r_C, int sl_B, int sl_C, int base, int len, int rows,
                                            int tid, int nthr) {
    constexpr int PITCH = ssd_bc_pitch(NK), PPR = 2 * NK;              // 16-byte pieces of a row
    const int npieces = rows * PPR;
    for (int q0 = 0; q0 < npieces; q0 += U * nthr) {
        u32x4_t vb[U], vc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * nthr + tid;
            if (q < npieces) {
                const int r = q / PPR, pc = q - r * PPR;
                const int rc = base + (r < len ? r : len - 1);
                vb[u] = ld16(r_B, rc * sl_B + 16 * pc);
                vc[u] = ld16(r_C, rc * sl_C + 16 * pc);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * nthr + tid;
            if (q < npieces) {
                const int r = q / PPR, pc = q - r * PPR;
                *reinterpret_cast<u32x4_t*>(Bl + r * PITCH + 16 * pc) = vb[u];
                *reinterpret_cast<u32x4_t*>(Cl + r * PITCH + 16 * pc) = vc[u];
            }
        }
    }
}

// X as B-fragments of the output product through the wave's staging tile: slot e of (it, ks) is key 32it + 4kh + 8(2ks + e/4) + e%4.
// Global traffic is whole 16-byte pieces of a row; the (key, channel) element order of the fragments is produced by the LDS reads
// (row pitch 80 B: the two key halves of a fragment read land on disjoint banks).
template <int NT>
__device__ __forceinline__ void sf_x_frags(u32x4_t (&xfrag)[NT][2], const u32x4_t (&xq)[NT][2], uint32_t* tile, int len, int lane) {
    const int col = lane & 31, kh = lane >> 5, trow = lane >> 1, thf = lane & 1;
    const uint16_t* const t16 = reinterpret_cast<const uint16_t*>(tile);
#pragma unroll
    for (int it = 0; it < NT; ++it) {
        const bool row_live = SSD_TILE * it + trow < len;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            *reinterpret_cast<u32x4_t*>(&tile[trow * SSD_PITCH + thf * 8 + 4 * q]) = row_live ? xq[it][q] : (u32x4_t){0u, 0u, 0u, 0u};
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint32_t w4[4];
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
                const int k0 = 4 * kh + 8 * (2 * ks + (e2 >> 1)) + 2 * (e2 & 1);
                const uint32_t lo = t16[k0 * (2 * SSD_PITCH) + col], hi = t16[(k0 + 1) * (2 * SSD_PITCH) + col];
                w4[e2] = lo | (hi << 16);
            }
            xfrag[it][ks] = (u32x4_t){w4[0], w4[1], w4[2], w4[3]};
        }
        __syncthreads();
    }
}

// The gate tile of a query tile, in flight under the products; off: byte offset of this lane's 32 bytes.  The gate is a view of the
// in_proj output, whose rows are 2 Din + 2 N + H elements: a multiple of 8 with the factory models' 16 or 24 heads, not with the two
// heads of a d_model 64 mixer -- such rows sit on 4-byte boundaries only and are read as dwords.
__device__ __forceinline__ bool sf_gate_rows16(const void* z, int64_t z_ss, int64_t z_sl) {
    return (((uintptr_t)z & 15) | (uintptr_t)(z_ss & 7) | (uintptr_t)(z_sl & 7)) == 0;
}
__device__ __forceinline__ void sf_gate_issue(u32x4_t (&zq)[2], const rsrc_t& r_z, int off, bool rows16) {
    if (rows16) {
#pragma unroll
        for (int q = 0; q < 2; ++q) zq[q] = ld16(r_z, off + 16 * q);
    } else {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int w = 0; w < 4; ++w) zq[q][w] = __builtin_amdgcn_raw_buffer_load_b32(r_z, off + 16 * q + 4 * w, 0, 0);
    }
}

// Score tile G^T = B_it C_lt^T over NK slices of 16 states from the staged rows: rows = keys 32it + 4kh + 8r4 + r, columns = queries.
// brows: this lane's row of key tile it (B rows + (32 it + col) pitch + 16 kh); lane (row = col, kh) holds states 16k + 8kh .. +7 of slice k.
template <typename O, int NK>
__device__ __forceinline__ f32x16 sf_scores(const uint8_t* brows, const u32x4_t (&cfrag)[NK]) {
    f32x16 g;
#pragma unroll
    for (int r = 0; r < 16; ++r) g[r] = 0.0f;
#pragma unroll
    for (int k = 0; k < NK; ++k) g = O::m32(*reinterpret_cast<const u32x4_t*>(brows + 32 * k), cfrag[k], g);
    return g;
}

// yacc += (packed score tile, the accumulator registers being the A-operand) (X fragments of that key tile)
template <typename O>
__device__ __forceinline__ void sf_times_x(f32x16& yacc, const uint32_t (&wp)[8], const u32x4_t (&xf)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
        yacc = O::m32(wf, xf[ks], yacc);
    }
}

// A key tile strictly before the query tile: factorised decay on the accumulator.  gd: the gamma dt table at the tile's row 4 kh;
// ad = alpha_l delta(lt, it) = exp2(s2_l - m_{it+1}).
template <typename O, int NK>
__device__ __forceinline__ void sf_offdiag(f32x16& yacc, const uint8_t* brows, const u32x4_t (&cfrag)[NK], const float* gd, float ad, const u32x4_t (&xf)[2]) {
    const f32x16 g = sf_scores<O, NK>(brows, cfrag);
    uint32_t wp[8];
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(&gd[8 * r4]);
        wp[2 * r4] = O::pack(g[4 * r4] * (gv[0] * ad), g[4 * r4 + 1] * (gv[1] * ad));
        wp[2 * r4 + 1] = O::pack(g[4 * r4 + 2] * (gv[2] * ad), g[4 * r4 + 3] * (gv[3] * ad));
    }
    sf_times_x<O>(yacc, wp, xf);
}

// The diagonal tile: element-wise decay and causal mask on the score tile g of the unscaled operands.  s2t / dtt: the log-decay and
// dt tables at the tile's row 4 kh = position k0; lq, s2l: this lane's query and its log-decay.  DT_ON_ACC false: dt is folded into
// the B rows already (d_state 16) and dtt is not read.
template <typename O, bool DT_ON_ACC>
__device__ __forceinline__ void sf_diag(f32x16& yacc, const f32x16& g, const float* s2t, const float* dtt, int k0, int lq, float s2l, const u32x4_t (&xf)[2]) {
    uint32_t wp[8];
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
        const f32x4 si = *reinterpret_cast<const f32x4*>(&s2t[8 * r4]);
        f32x4 di = {1.0f, 1.0f, 1.0f, 1.0f};
        if (DT_ON_ACC) di = *reinterpret_cast<const f32x4*>(&dtt[8 * r4]);
        float wv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = fast_exp2(s2l - si[r]);
            wv[r] = (k0 + 8 * r4 + r <= lq) ? g[4 * r4 + r] * (DT_ON_ACC ? di[r] * e : e) : 0.0f;
        }
        wp[2 * r4] = O::pack(wv[0], wv[1]);
        wp[2 * r4 + 1] = O::pack(wv[2], wv[3]);
    }
    sf_times_x<O>(yacc, wp, xf);
}

// Epilogue of a query tile: + D x from the resident fragment, gate, scatter.  yacc[4 r4 + r] = Y[tile row 4kh + 8 r4 + r][this lane's
// channel].  The gate tile goes through `tin`, the 16-bit output tile through `tout` back to 16-byte row pieces; with ONE tile per
// wave (tin == tout: the lane that reads gate element (row, col) is the lane that writes the output element there) LEAD_BARRIER
// waits for the previous query tile's row reads.  live: this lane's row trow of the tile exists; orow_tab: its entry of the output
// row table.
template <typename O, bool LEAD_BARRIER>
__device__ __forceinline__ void sf_epilogue(const f32x16& yacc, const u32x4_t (&xf)[2], float Dh, bool gated, const u32x4_t (&zq)[2], uint32_t* tin, uint32_t* tout,
                                            const rsrc_t& r_o, int sl_o, int cb, const int* orow_tab, bool live, int lane) {
    const int col = lane & 31, kh = lane >> 5, trow = lane >> 1, thf = lane & 1;
    if (LEAD_BARRIER) __syncthreads();
    if (gated) {
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<u32x4_t*>(&tin[trow * SSD_PITCH + thf * 8 + 4 * q]) = zq[q];
    }
    __syncthreads();
    {
        const uint16_t* const in16 = reinterpret_cast<const uint16_t*>(tin);
        uint16_t* const out16 = reinterpret_cast<uint16_t*>(tout);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * kh + 8 * r4 + r;
                const int e = 4 * (r4 & 1) + r;
                const uint32_t xw = xf[r4 >> 1][e >> 1];
                const float xv = (e & 1) ? O::hi(xw) : O::lo(xw);
                float y = yacc[4 * r4 + r] + Dh * xv;
                if (gated) y *= silu_f(O::lo((uint32_t)in16[row * (2 * SSD_PITCH) + col]));
                out16[row * (2 * SSD_PITCH) + col] = (uint16_t)(O::pack(y, 0.0f) & 0xffffu);
            }
    }
    __syncthreads();
    if (live) {
        const int orow = *orow_tab;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const u32x4_t v = *reinterpret_cast<const u32x4_t*>(&tout[trow * SSD_PITCH + thf * 8 + 4 * q]);
            __builtin_amdgcn_raw_buffer_store_b128(v, r_o, orow * sl_o + cb + 16 * q, 0, 0);
        }
    }
}

// ---- host: the argument and layout checks of both entry points (who = the entry's name, maxl = its longest sequence).
// z16_at_d16: at d_state 16 the gate rows move as 16-byte pieces like every other row (dm_ssd_fwd); elsewhere they may sit on 4-byte
// boundaries.
static inline int ssd_fwd_check(const char* who, const dm_ssd_fwd_args* args, int (*supported)(int, int, int, int), int maxl, bool z16_at_d16) {
    if (!args) { set_error("%s: null args", who); return DM_ERR_ARG; }
    const dm_ssd_fwd_args& a = *args;
    if (!a.x || !a.B || !a.C || !a.dt || !a.A || !a.out) { set_error("%s: null tensor pointer", who); return DM_ERR_ARG; }
    if (a.nseq <= 0 || a.nheads <= 0 || a.seqlen <= 0) { set_error("%s: non-positive size", who); return DM_ERR_ARG; }
    if (!supported(a.seqlen, a.headdim, a.dstate, a.io_dtype)) {
        set_error("%s: needs 16-bit I/O, headdim 64, d_state 16 / 32 / 64 / 128, seqlen <= %d (got L %d P %d N %d dtype %d)", who, maxl, a.seqlen, a.headdim, a.dstate, a.io_dtype);
        return DM_ERR_ARG;
    }
    if (a.nseq > 65535) { set_error("%s: nseq %d > 65535", who, a.nseq); return DM_ERR_ARG; }
    if (a.batch_per_dir > 0 && a.nseq % a.batch_per_dir != 0) { set_error("%s: nseq %% batch_per_dir != 0", who); return DM_ERR_ARG; }
    if ((a.z_row_index == nullptr) != (a.out_row_index == nullptr)) { set_error("%s: both row-index tables or neither", who); return DM_ERR_ARG; }
    auto bad = [](const void* ptr, int64_t s0, int64_t s1) { return ((uintptr_t)ptr & 15) || (s0 & 7) || (s1 & 7); };
    if (bad(a.B, a.B_ss, a.B_sl) || bad(a.C, a.C_ss, a.C_sl)) { set_error("%s: B / C rows must be 16-byte aligned", who); return DM_ERR_LAYOUT; }
    const bool z16 = z16_at_d16 && a.dstate == 16;
    if (bad(a.x, a.x_ss, a.x_sl) || bad(a.out, a.o_ss, a.o_sl) || (a.z && z16 && bad(a.z, a.z_ss, a.z_sl))) {
        set_error("%s: x / %sout rows must be 16-byte aligned (tiles move as 16-byte pieces)", who, z16_at_d16 ? "z / " : ""); return DM_ERR_LAYOUT;
    }
    if (a.z && !z16 && (((uintptr_t)a.z & 3) || (a.z_ss & 1) || (a.z_sl & 1))) {
        if (z16_at_d16) set_error("%s: z rows must be 4-byte aligned at d_state %d", who, a.dstate);
        else set_error("%s: z rows must be 4-byte aligned", who);
        return DM_ERR_LAYOUT;
    }
    return DM_OK;
}

}  // namespace dm
