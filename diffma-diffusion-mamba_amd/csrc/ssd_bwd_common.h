// What the two SSD backward kernels (ssd_bwd.hip at d_state 16, ssd_bwd_wide.hip at 32 / 64 / 128) share: the tile geometry, the
// tail of the LDS map with its named tables, the swizzled X / gY row fragments, the one-hot selector fragments, the workgroup
// prefix sum, the issue half of the load front, phase 3 and the host-side checks.
//
// What they do NOT share although the text is the same in both:
//   * the per-position tables: as a function they cost the d_state 16 kernel, which sits at 256 registers, a fourth spill;
//   * the X / gY staging with its dD partial, the decay factors, the W / dG pack with its row / column sums and the dz / dx
//     epilogues.  Each has a sum of two products or an fma next to a 16-bit conversion, and which product the compiler contracts
//     into the fma (or whether it fuses the conversion) changes as soon as the block is an inlined function instead of kernel
//     text: d dt, dA, dD, d dt_bias and a few f16 dx elements then differ in their last bits.  The staging-tile turn inside the
//     epilogues has no such sum and keeps the bits as a function of its own, but it moves the register allocation of the
//     d_state 16 kernel (2 spilled instead of 3) and of the d_state 128 bf16 one (456 instead of 458) for 12 lines saved.
// The blocks below leave every floating-point expression of the optimised kernels, and their register figures, as they were.
#pragma once
#include "dm_mfma.h"

namespace dm {

constexpr int SB_MAXL = 196;                      // longest sequence
constexpr int SB_TILE = 32, SB_MAXT = 7;
constexpr int SB_TAB = SB_TILE * SB_MAXT;         // 224 tile-rounded positions
constexpr int SB_ROWS = SB_MAXL + 1;              // LDS rows of the operand arrays: row 196 is all zeros, every position past it aliases to it
constexpr int SB_WAVES = 4;
constexpr int SB_THREADS = 64 * SB_WAVES;
constexpr int SB_STG = 68;                        // dwords per staging-tile row (64 + 4)

enum { T_DT, T_CUM, T_S2, T_ALPHA, T_GAM, T_GDT, T_SIG, T_RS, T_CS, T_NTAB };   // fp32 tables [T_NTAB][224]

// LDS map.  A kernel places its operand arrays, then this tail (byte offsets from its 16-byte aligned start):
constexpr int SB_T_IDX = T_NTAB * SB_TAB * 4;                     // after the fp32 tables: uint16 tables of z rows, dout rows
constexpr int SB_T_STAGE = SB_T_IDX + 2 * SB_TAB * 2;             // 4 waves x [8][SB_STG] fp32
constexpr int SB_T_RED = SB_T_STAGE + SB_WAVES * 8 * SB_STG * 4;  // block-reduction scratch
constexpr int SB_T_BYTES = SB_T_RED + 128;
static_assert(SB_T_STAGE % 16 == 0, "16-byte aligned LDS arrays");

// The tail by name.  A kernel unpacks it with a structured binding in this order.
struct sb_tables {
    float *DT, *CUM, *S2, *ALPHA, *GAM, *GDT, *SIG, *RS, *CSV;
    uint16_t *zi, *oi;
    float *stage, *red;                           // this wave's staging tile; the workgroup's reduction scratch
    __device__ __forceinline__ sb_tables(uint8_t* tail, int w) {
        float* const tab = reinterpret_cast<float*>(tail);
        DT = tab + T_DT * SB_TAB;
        CUM = tab + T_CUM * SB_TAB;
        S2 = tab + T_S2 * SB_TAB;
        ALPHA = tab + T_ALPHA * SB_TAB;
        GAM = tab + T_GAM * SB_TAB;
        GDT = tab + T_GDT * SB_TAB;
        SIG = tab + T_SIG * SB_TAB;
        RS = tab + T_RS * SB_TAB;
        CSV = tab + T_CS * SB_TAB;
        zi = reinterpret_cast<uint16_t*>(tail + SB_T_IDX);
        oi = zi + SB_TAB;
        stage = reinterpret_cast<float*>(tail + SB_T_STAGE) + w * 8 * SB_STG;
        red = reinterpret_cast<float*>(tail + SB_T_RED);
    }
    __device__ __forceinline__ float m_of(int t) const { return t ? S2[SB_TILE * t - 1] : 0.0f; }   // log-decay just before tile t
};

__device__ __forceinline__ void wave_lds_sync() {         // make one wave's LDS writes visible to its other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 8 consecutive columns (chunk) of a row of the swizzled [197][64] arrays, as an MFMA operand fragment (rows >= 196: the zero row)
__device__ __forceinline__ u32x4_t row_frag(const uint8_t* base, int row, int chunk) {
    const int rc = row < SB_MAXL ? row : SB_MAXL;
    return *reinterpret_cast<const u32x4_t*>(base + rc * 128 + ((chunk ^ (rc & 7)) << 4));
}
// One-hot selector fragment: slot e (0..7) of this lane holds 1.0, every other slot 0 (e outside 0..7: all zero)
template <typename T>
__device__ __forceinline__ u32x4_t one_hot(int e) {
    constexpr uint32_t ONE = std::is_same<T, bf16_t>::value ? 0x3F80u : 0x3C00u;
    const uint32_t v = (e & 1) ? (ONE << 16) : ONE;
    const int d = e >> 1;
    const bool ok = e >= 0 && e < 8;
    return (u32x4_t){(ok && d == 0) ? v : 0u, (ok && d == 1) ? v : 0u, (ok && d == 2) ? v : 0u, (ok && d == 3) ? v : 0u};
}
// accumulator tile -> the two K-step fragments (8 positions each, accumulator order) of a 16-bit B-operand
template <typename O>
__device__ __forceinline__ void acc_to_frags(const f32x16& d, u32x4_t (&f)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
        f[ks] = (u32x4_t){O::pack(d[8 * ks], d[8 * ks + 1]), O::pack(d[8 * ks + 2], d[8 * ks + 3]), O::pack(d[8 * ks + 4], d[8 * ks + 5]),
                            O::pack(d[8 * ks + 6], d[8 * ks + 7])};
}

// Inclusive prefix sum over the workgroup's 256 threads (one value each): six shuffle steps inside each wave, one barrier to pass
// the wave totals on.  Every thread of the workgroup must call it.
__device__ __forceinline__ float block_prefix_sum(float v, int lane, int w, float* wtot) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const float t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    if (lane == WAVE - 1) wtot[w] = v;
    __syncthreads();
    float base = 0.0f;
#pragma unroll
    for (int j = 0; j < SB_WAVES - 1; ++j) base += (j < w) ? wtot[j] : 0.0f;
    return v + base;
}

// The kernel's argument struct is handed to the blocks below BY VALUE.  An observation of this compiler version, not a contract:
// bound to a reference, the struct's kernarg loads lose their no-clobber annotation and the optimiser's choices shift all over
// the kernel; by value the d_state 16 kernel stays at 256 registers / 3 spilled / 16 bytes of scratch.

// ---- phases 0 + 1: EVERY global load of the (sequence, head) is requested up front, in two dependent levels --------------------
// A chain of ~6 memory latencies before the first MFMA (row indices -> dt -> [prefix sums] -> x / dout / z of chunk w -> the same
// of chunk w + 4 -> B / C), each ended by LDS stores or a barrier, parked 35 % of the wave-cycles at barriers with no unit busy
// (profiles/r05_m2_ssd_pmc.txt).  Level 1 = the x rows and the row-index entries (the thread's own position and the 4 rows the
// lane moves; and B / C where a kernel stages them), level 2 = dt, dout, z through those indices -- 2 latencies; the tables are
// computed while level 2 flies.  Wave w moves the 16-byte chunks w and w + 4 of every row; lane rows r = lane + 64 j.
struct sb_front {
    u32x4_t xq4[2][4], dq4[2][4], zq4[2][4];
    float rawv;
    int zr0, orow0;
};
// hb: byte offset of the head's columns in a row; z_piece(byte offset): the kernel's 16-byte gate load
template <typename T, typename ZPiece>
__device__ __forceinline__ void sb_front_issue(sb_front& f, const dm_ssd_bwd_args p, const rsrc_t& r_x, const rsrc_t& r_do, const int32_t* __restrict__ zidx,
                                               const int32_t* __restrict__ oidx, const T* __restrict__ dtp, int hb, int tid, int lane, int w, ZPiece z_piece) {
    constexpr int ES = (int)sizeof(T);
    const int L = p.seqlen, sl_x = (int)p.x_sl * ES, sl_do = (int)p.do_sl * ES, sl_z = (int)p.z_sl * ES;
    const int pc = tid < L ? tid : L - 1;
    if (zidx) { f.zr0 = zidx[pc]; f.orow0 = oidx[pc]; } else { f.zr0 = pc; f.orow0 = pc; }
    int zrow[4], drow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = lane + 64 * j;
        const int rc = r < L ? r : L - 1;
        zrow[j] = zidx ? zidx[rc] : rc;
        drow[j] = oidx ? oidx[rc] : rc;
#pragma unroll
        for (int m = 0; m < 2; ++m) f.xq4[m][j] = ld16(r_x, rc * sl_x + hb + (w + 4 * m) * 16);
    }
    // level 2: through the indices
    f.rawv = 0.0f;
    if (tid < L) f.rawv = io<T>::ld(dtp + (int64_t)f.zr0 * p.dt_sl);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int cb = hb + (w + 4 * m) * 16;
            f.dq4[m][j] = ld16(r_do, drow[j] * sl_do + cb);
            f.zq4[m][j] = (u32x4_t){0u, 0u, 0u, 0u};
            if (p.z) f.zq4[m][j] = z_piece(zrow[j] * sl_z + cb);
        }
}

// ---- phase 3: d dt, dA, dD of (sequence s, head h) on the whole workgroup (thread t works on position 223 - t: the cumulative
// sum of d s runs from the end; shuffle scans inside the waves, one barrier).  Call it behind the barrier that ends phase 2.
__device__ __forceinline__ void sb_phase3(const dm_ssd_bwd_args p, const sb_tables& t, int s, int h, int tid, int lane, int w, float Ah, float dD_acc) {
    const int L = p.seqlen, H = p.nheads;
    const int pos = SB_TAB - 1 - tid;
    const bool live = tid < SB_TAB && pos < L;
    float csv = 0.0f, dsv = 0.0f;
    if (live) {
        csv = t.CSV[pos];
        dsv = t.RS[pos] - t.DT[pos] * csv;                                        // d s_l
    }
    const float rc = block_prefix_sum(dsv, lane, w, t.red + 24);                  // sum_{l >= pos} d s_l
    const float draw = live ? (csv + Ah * rc) * t.SIG[pos] : 0.0f;                // d(raw dt) through softplus
    {
        const float a = wave_sum_dpp(live ? dsv * t.CUM[pos] : 0.0f), d = wave_sum_dpp(dD_acc), b = wave_sum_dpp(draw);
        if (lane == 0) {
            t.red[w] = a;
            t.red[8 + w] = d;
            t.red[16 + w] = b;
        }
    }
    if (live) p.ddt[((int64_t)s * L + t.zi[pos]) * H + h] = draw;
    __syncthreads();
    if (tid < 3) {                                                                // dA | dD | d dt_bias partial sums of this (sequence, head)
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < SB_WAVES; ++k) sum += t.red[8 * tid + k];
        p.dAD_part[((int64_t)s * 3 + tid) * H + h] = sum;
    }
}

// ---- host: the argument and layout checks of both entry points (who = the entry's name).  wide: d_state 32 / 64 / 128, where the
// gate rows may sit on 4-byte boundaries (ssd_bwd_wide.hip); at d_state 16 they move as 16-byte pieces like every other row.
static inline int ssd_bwd_check(const char* who, const dm_ssd_bwd_args* args, int (*supported)(int, int, int, int), bool wide) {
    if (!args) { set_error("%s: null args", who); return DM_ERR_ARG; }
    const dm_ssd_bwd_args& a = *args;
    if (!a.x || !a.B || !a.C || !a.dt || !a.dout || !a.A || !a.dx || !a.dBC_part || !a.ddt || !a.dAD_part) {
        set_error("%s: null tensor pointer", who); return DM_ERR_ARG;
    }
    if ((a.z == nullptr) != (a.dz == nullptr)) { set_error("%s: z and dz go together", who); return DM_ERR_ARG; }
    if (a.nseq <= 0 || a.nheads <= 0 || a.seqlen <= 0) { set_error("%s: non-positive size", who); return DM_ERR_ARG; }
    if (!supported(a.seqlen, a.headdim, a.dstate, a.io_dtype)) {
        set_error("%s: needs 16-bit I/O, headdim 64, d_state %s, seqlen <= %d (got L %d P %d N %d dtype %d)", who, wide ? "32 / 64 / 128" : "16", SB_MAXL, a.seqlen,
                  a.headdim, a.dstate, a.io_dtype);
        return DM_ERR_ARG;
    }
    if (a.nseq > 65535) { set_error("%s: nseq %d > 65535", who, a.nseq); return DM_ERR_ARG; }
    if (a.batch_per_dir > 0 && a.nseq % a.batch_per_dir != 0) { set_error("%s: nseq %% batch_per_dir != 0", who); return DM_ERR_ARG; }
    if ((a.z_row_index == nullptr) != (a.out_row_index == nullptr)) { set_error("%s: both row-index tables or neither", who); return DM_ERR_ARG; }
    auto bad = [](const void* ptr, int64_t s0, int64_t s1) { return ((uintptr_t)ptr & 15) || (s0 & 7) || (s1 & 7); };
    if (bad(a.x, a.x_ss, a.x_sl) || bad(a.B, a.B_ss, a.B_sl) || bad(a.C, a.C_ss, a.C_sl) || bad(a.dout, a.do_ss, a.do_sl) ||
        bad(a.dx, a.dx_ss, a.dx_sl) || (a.dz && bad(a.dz, a.dz_ss, a.dz_sl)) || (!wide && a.z && bad(a.z, a.z_ss, a.z_sl))) {
        set_error("%s: %srows must be 16-byte aligned (tiles move as 16-byte pieces)", who, wide ? "x / B / C / dout / dx / dz " : ""); return DM_ERR_LAYOUT;
    }
    if (wide && a.z && (((uintptr_t)a.z & 3) || (a.z_ss & 1) || (a.z_sl & 1))) { set_error("%s: z rows must be 4-byte aligned", who); return DM_ERR_LAYOUT; }
    return DM_OK;
}

}  // namespace dm
