// K6  dm_ssd_fwd -- Mamba-2 state-space duality, single chunk, on the matrix pipe (forward).
//
// Replaces the SSD core of mamba_split_conv1d_scan_combined (reference call block/mamba2.py:392-410; mathematics SURVEY.md A.2)
// after the conv: with chunk_size 256 >= L the operator is ONE chunk, and because Mamba-2's decay is a scalar per head the
// recurrence factorises into dense products (the "dual" quadratic form):
//     s_l   = A_h * cumsum(dt)_l                          (log-decay, <= 0 and decreasing)
//     G     = (C B^T) .* exp(s_l - s_i) [i <= l]          [L x L], K = d_state
//     Y     = (G diag(dt)) X + D_h X                      [L x P], K = L          out = Y * silu(z)
// One wave64 owns one (sequence, head, 32-column half): 32 x 32 tiles, v_mfma_f32_32x32x16_{bf16,f16}.  The transposed score tile
// G^T = (dt .* B)_it C_lt^T is produced with keys as rows and queries as columns, so its accumulator registers ARE the
// A-operand of the second product (row = query l, K slots = keys in the order 4*(lane>>5) + 8*r4 + r): the decay factor and
// the causal mask are applied in registers, the tile is rounded to 16 bit and fed straight back -- no LDS round trip, no
// cross-lane move.  X is held as B-operand fragments in that same key order for the whole sequence (56 VGPRs), so the inner
// loop has no memory operation at all except the broadcast reads of the log-decays from LDS.  z is gathered and the output
// scattered through the row-index tables exactly like the scan kernels (CrossScan / CrossMerge folded into addressing); the
// per-head dt is read in the kernel (token order, through the gather table), no [nseq, L, Din] delta tensor exists.
// 16-bit I/O only (the score tile is rounded to the I/O dtype); fp32 I/O stays on the A-shared scan.  Backward twin: ssd_bwd.hip.
#include <type_traits>
#include "ssd_fwd_common.h"

namespace dm {

constexpr int SSD_MAXT = 7;                       // L <= 224
constexpr int SSD_MAXL = SSD_TILE * SSD_MAXT;

// One wave64 per (sequence, head, 32-column half of the head): 56 VGPRs of X fragments, ~150 registers, 3 waves per SIMD.
//
// Decay factorisation.  s2 = log2-domain log-decay prefix sums (decreasing), m_t = s2 just before tile t (m_0 = 0).  For a key
// tile it strictly before the query tile lt:   exp2(s2_l - s2_i) = alpha_l * delta(lt, it) * gamma_i   with
//     alpha_l = exp2(s2_l - m_lt),   gamma_i = exp2(m_{it+1} - s2_i),   delta = exp2(m_lt - m_{it+1}),     all three <= 1,
// so gamma (and dt) is folded into the B rows once, alpha into the C rows once per query tile, and an off-diagonal score tile
// costs one scalar exp and 16 multiplies.  Only the 7 diagonal tiles of 28 take the element-wise exp (on unscaled operands:
// there alpha * gamma could underflow while the true factor is O(1)).
template <typename T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void ssd_fwd_kernel(const dm_ssd_fwd_args p) {
    using O = mfma<T>;
    constexpr int ES = (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) float s2_lds[2][SSD_MAXL + 32];    // log2-domain log-decay (prefix sums, ping-pong)
    __shared__ __attribute__((aligned(16))) float dt_lds[SSD_MAXL];
    __shared__ int zi_lds[SSD_MAXL], oi_lds[SSD_MAXL];
    // 32-row x 32-channel staging tiles (ssd_fwd_common.h): the gate tile goes in through one, the output tile out through the other
    __shared__ __attribute__((aligned(16))) uint32_t tile_a[SSD_TILE * SSD_PITCH], tile_b[SSD_TILE * SSD_PITCH];

    const int lane = threadIdx.x;
    const int col = lane & 31, kh = lane >> 5;
    const int trow = lane >> 1, thf = lane & 1;                          // staging role: row of the tile, 16-channel half of it
    const int h = blockIdx.x >> 1, half = blockIdx.x & 1, s = blockIdx.y;
    const int L = p.seqlen;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int nt_l = (L + SSD_TILE - 1) / SSD_TILE;
    const int32_t* __restrict__ zidx = p.z_row_index ? p.z_row_index + (int64_t)dir * L : nullptr;
    const int32_t* __restrict__ oidx = p.out_row_index ? p.out_row_index + (int64_t)dir * L : nullptr;
    const float Ah = p.A[h] * LOG2E, Dh = p.D ? p.D[h] : 0.0f, bias = p.dt_bias ? p.dt_bias[h] : 0.0f;
    const rsrc_t r_x = make_rsrc((const T*)p.x + (int64_t)s * p.x_ss);
    const rsrc_t r_B = make_rsrc((const T*)p.B + (int64_t)s * p.B_ss);
    const rsrc_t r_C = make_rsrc((const T*)p.C + (int64_t)s * p.C_ss);
    const rsrc_t r_z = make_rsrc(p.z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_o = make_rsrc((T*)p.out + (int64_t)s * p.o_ss);
    const T* __restrict__ dtp = (const T*)p.dt + (int64_t)sb * p.dt_sb + h;
    const int sl_x = (int)p.x_sl * ES, sl_B = (int)p.B_sl * ES, sl_C = (int)p.C_sl * ES, sl_z = (int)p.z_sl * ES, sl_o = (int)p.o_sl * ES;

    // ---- every load that does not depend on the decays goes out first: one HBM round trip covers X, B and the dt gather ------
    const int cb = (h * 64 + half * 32 + thf * 16) * ES;                 // byte offset of this lane's 16 staged channels in a row
    u32x4_t xq[SSD_MAXT][2], bq[SSD_MAXT];
#pragma unroll
    for (int it = 0; it < SSD_MAXT; ++it) {
        const int i = SSD_TILE * it + trow;
        const int ic = i < L ? i : L - 1;                                 // rows past the end: clamped here, zeroed below
#pragma unroll
        for (int q = 0; q < 2; ++q) xq[it][q] = ld16(r_x, ic * sl_x + cb + 16 * q);
        const int j = SSD_TILE * it + col;
        const int jc = j < L ? j : L - 1;
        bq[it] = ld16(r_B, jc * sl_B + kh * 8 * ES);
    }

    // ---- per-position scalars: dt = softplus(raw + bias), log-decay prefix sums, row tables -------------------------------
#pragma unroll
    for (int k = 0; k < SSD_MAXL / WAVE + 1; ++k) {
        const int l = lane + WAVE * k;
        if (l < SSD_MAXL) {
            float dtv = 0.0f;
            int zr = 0, orow = 0;
            if (l < L) {
                zr = zidx ? zidx[l] : l;
                orow = oidx ? oidx[l] : l;
                dtv = softplus_f(io<T>::ld(dtp + (int64_t)zr * p.dt_sl) + bias);
            }
            dt_lds[l] = dtv;
            s2_lds[0][l] = Ah * dtv;
            zi_lds[l] = zr;
            oi_lds[l] = orow;
        }
    }
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int off = 1; off < SSD_MAXL; off <<= 1) {                       // inclusive prefix sum (Hillis-Steele, one wave)
#pragma unroll
        for (int k = 0; k < SSD_MAXL / WAVE + 1; ++k) {
            const int l = lane + WAVE * k;
            if (l < SSD_MAXL) s2_lds[cur ^ 1][l] = s2_lds[cur][l] + (l >= off ? s2_lds[cur][l - off] : 0.0f);
        }
        __syncthreads();
        cur ^= 1;
    }
    const float* const s2 = s2_lds[cur];
    auto m_of = [&](int t) -> float { return t == 0 ? 0.0f : s2[SSD_TILE * t - 1]; };   // log-decay just before tile t

    // ---- operands resident for the whole sequence ---------------------------------------------------------------------------
    // (gamma .* dt .* B) rows as A-fragments of the off-diagonal score products: lane (row i = col, kh) holds 8 states
    u32x4_t bfrag[SSD_MAXT];
#pragma unroll
    for (int it = 0; it < SSD_MAXT; ++it) {
        const int i = SSD_TILE * it + col;
        const int ic = i < L ? i : L - 1;
        const float sc = (i < L) ? dt_lds[ic] * fast_exp2(m_of(it + 1 < SSD_MAXT ? it + 1 : it) - s2[ic]) : 0.0f;   // (the last tile is never off-diagonal)
#pragma unroll
        for (int w = 0; w < 4; ++w) bfrag[it][w] = O::pack(O::lo(bq[it][w]) * sc, O::hi(bq[it][w]) * sc);
    }
    u32x4_t xfrag[SSD_MAXT][2];                                          // X as B-fragments of the output product, keys in accumulator order
    sf_x_frags(xfrag, xq, tile_a, L, lane);

    // C rows (the B-operand of the score product: lane (col l, kh) holds C[l][8kh .. +7]) and the unscaled B rows of the diagonal
    // tile are fetched one query tile ahead
    auto load_cb = [&](int t, u32x4_t& c, u32x4_t& b) {
        const int j = SSD_TILE * t + col;
        const int jc = j < L ? j : L - 1;
        c = ld16(r_C, jc * sl_C + kh * 8 * ES);
        b = ld16(r_B, jc * sl_B + kh * 8 * ES);
    };
    u32x4_t cnext, bnext;
    load_cb(0, cnext, bnext);
#pragma unroll
    for (int lt = 0; lt < SSD_MAXT; ++lt) {                              // (fully unrolled: every fragment index is a compile-time constant)
        if (lt >= nt_l) break;
        const int lq = SSD_TILE * lt + col;                              // this lane's query in the score tile (a column of G^T)
        const int lqc = lq < L ? lq : L - 1;
        const float s2l = s2[lqc], mlt = m_of(lt);
        const u32x4_t craw = cnext, qb = bnext;                         // raw C for the diagonal tile, alpha-scaled for the others
        const u32x4_t qc = craw;
        if (lt + 1 < SSD_MAXT) load_cb(lt + 1, cnext, bnext);
        u32x4_t zq[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};                // the gate tile of this query tile, in flight under the products
        const int lrow = SSD_TILE * lt + trow;
        const int lrc = lrow < L ? lrow : L - 1;
        if (p.z) sf_gate_issue(zq, r_z, zi_lds[lrc] * sl_z + cb, true);   // (dm_ssd_fwd takes 16-byte gate rows only at d_state 16)
        const float alpha = fast_exp2(s2l - mlt);
        u32x4_t cfrag;
#pragma unroll
        for (int w = 0; w < 4; ++w) cfrag[w] = O::pack(O::lo(qc[w]) * alpha, O::hi(qc[w]) * alpha);
        f32x16 yacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) yacc[r] = 0.0f;
        // ---- key tiles strictly before the query tile: factorised decay ----
#pragma unroll
        for (int it = 0; it < SSD_MAXT - 1; ++it) {
            if (it < lt) {                                                // wave-uniform
                f32x16 g;
#pragma unroll
                for (int r = 0; r < 16; ++r) g[r] = 0.0f;
                g = O::m32(bfrag[it], cfrag, g);                         // rows = keys 32it + 4kh + 8r4 + r, columns = queries
                const float delta = fast_exp2(mlt - m_of(it + 1));
                uint32_t wp[8];
#pragma unroll
                for (int r2 = 0; r2 < 8; ++r2) {
                    const f32x2 gs = (f32x2){g[2 * r2], g[2 * r2 + 1]} * (f32x2){delta, delta};        // v_pk_mul_f32
                    wp[r2] = O::pack(gs.x, gs.y);
                }
                sf_times_x<O>(yacc, wp, xfrag[it]);
            }
        }
        // ---- the diagonal tile: element-wise decay and causal mask on unscaled operands ----
        {
            const int i = SSD_TILE * lt + col;
            const int ic = i < L ? i : L - 1;
            const float dti = (i < L) ? dt_lds[ic] : 0.0f;
            u32x4_t bd;
#pragma unroll
            for (int w = 0; w < 4; ++w) bd[w] = O::pack(O::lo(qb[w]) * dti, O::hi(qb[w]) * dti);
            f32x16 g;
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = 0.0f;
            g = O::m32(bd, craw, g);
            sf_diag<O, false>(yacc, g, &s2[SSD_TILE * lt + 4 * kh], nullptr, SSD_TILE * lt + 4 * kh, lq, s2l, xfrag[lt]);
        }
        // ---- epilogue of the query tile: + D x, gate (in through tile_a), scatter (out through tile_b) ----
        sf_epilogue<O, false>(yacc, xfrag[lt], Dh, p.z != nullptr, zq, tile_a, tile_b, r_o, sl_o, cb, &oi_lds[lrc], lrow < L, lane);
    }
}

// ---- wide states: d_state = 16 NK, NK in {2, 4, 8} ----------------------------------------------------------------------------
//
// Same operator, same contract, same (head, 32-column half) role per wave with X resident; only the contraction of the score
// tile runs over NK slices of 16 states.  What changes is where B and C live: NK u32x4 fragments per key tile would be 224
// registers at d_state 128, and a private LDS copy per wave 112 KB.  B and C are head-independent (ngroups 1), so ONE workgroup
// of 8 waves serves 4 heads of a sequence and stages the sequence's raw B / C rows in LDS once (2 x 224 rows x (32 NK + 16)
// bytes: the 16-byte pad makes the row pitch an odd number of 16-byte pieces, so the 16 rows of a ds_read_b128 lane group fall
// on 16 different bank quads); every wave reads its A / B fragments of the score product from there, one ds_read_b128 per
// MFMA for the key side, the query side once per query tile.  At d_state 128 that is 153 KB with the tables: one workgroup per
// CU, two waves per SIMD.  Waves of heads past nheads help with the staging and leave.
//
// The operands stay raw.  gamma_i dt_i (per key = accumulator row, a table of the head) and alpha_l delta = exp2(s2_l - m_{it+1})
// (per query = one scalar per lane) multiply the fp32 accumulator instead of the 16-bit rows: two roundings per pair fewer than
// the d_state 16 kernel (B, C as given, the score tile once), and no subnormal B dt in fp16 on small-dt heads.  The diagonal
// tile takes dt_i, the element-wise exp2 and the mask on the accumulator too.
//
// Not chosen: fragments straight from L2 per tile pair (8 KB per pair and wave at d_state 128, 32 waves per sequence: 7 MB of L2
// reads per sequence against 0.1 MB staged four times here); a K-sliced ping-pong stage (needs a barrier per slice between waves
// that otherwise never wait for each other after the prologue's tables).
constexpr int SSDW_HEADS = 4;                                // heads per workgroup
constexpr int SSDW_WAVES = 2 * SSDW_HEADS;
constexpr int SSDW_THREADS = WAVE * SSDW_WAVES;
constexpr int SSDW_TAB = 256;                                // entries per per-position table (>= SSD_MAXL, a multiple of WAVE)
constexpr int SSDW_TABS = 0;                                 // byte offsets: per head s2 ping | s2 pong (then gamma dt) | dt
constexpr int SSDW_IDX = SSDW_TABS + SSDW_HEADS * 3 * SSDW_TAB * 4;                 // z rows | out rows
constexpr int SSDW_TILES = SSDW_IDX + 2 * SSDW_TAB * 4;                              // one 32 x 32 staging tile per wave
constexpr int SSDW_BC = SSDW_TILES + SSDW_WAVES * SSD_TILE * SSD_PITCH * 4;          // B rows, then C rows
constexpr int ssdw_lds_bytes(int nk, int rows) { return SSDW_BC + 2 * rows * ssd_bc_pitch(nk); }
static_assert(SSDW_TAB >= SSD_MAXL && SSDW_TAB % WAVE == 0 && SSDW_TAB == 256, "eight doubling steps leave the prefix sums in the ping table");
static_assert(ssdw_lds_bytes(8, SSD_MAXL) <= 160 * 1024, "LDS of a CU");

template <typename T, int NK>
__global__ __launch_bounds__(SSDW_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void ssd_fwd_wide_kernel(const dm_ssd_fwd_args p) {
    using O = mfma<T>;
    constexpr int ES = (int)sizeof(T);
    constexpr int PITCH = ssd_bc_pitch(NK);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & (WAVE - 1);
    const int col = lane & 31, kh = lane >> 5;
    const int trow = lane >> 1, thf = lane & 1;                          // staging role: row of the tile, 16-channel half of it
    const int hh = wave >> 1, half = wave & 1;
    const int h = blockIdx.x * SSDW_HEADS + hh, s = blockIdx.y;
    const bool head_live = h < p.nheads;                                 // wave-uniform
    const int L = p.seqlen;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int nt_l = (L + SSD_TILE - 1) / SSD_TILE;
    const int rows = SSD_TILE * nt_l;
    const int32_t* __restrict__ zidx = p.z_row_index ? p.z_row_index + (int64_t)dir * L : nullptr;
    const int32_t* __restrict__ oidx = p.out_row_index ? p.out_row_index + (int64_t)dir * L : nullptr;

    float* const S2A = reinterpret_cast<float*>(lds + SSDW_TABS) + hh * 3 * SSDW_TAB;
    float* const DT = S2A + 2 * SSDW_TAB;
    int* const zi_lds = reinterpret_cast<int*>(lds + SSDW_IDX);
    int* const oi_lds = zi_lds + SSDW_TAB;
    uint32_t* const tile = reinterpret_cast<uint32_t*>(lds + SSDW_TILES) + wave * (SSD_TILE * SSD_PITCH);
    uint8_t* const Bl = lds + SSDW_BC;
    uint8_t* const Cl = Bl + rows * PITCH;

    const rsrc_t r_x = make_rsrc((const T*)p.x + (int64_t)s * p.x_ss);
    const rsrc_t r_B = make_rsrc((const T*)p.B + (int64_t)s * p.B_ss);
    const rsrc_t r_C = make_rsrc((const T*)p.C + (int64_t)s * p.C_ss);
    const rsrc_t r_z = make_rsrc(p.z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_o = make_rsrc((T*)p.out + (int64_t)s * p.o_ss);
    const int sl_x = (int)p.x_sl * ES, sl_B = (int)p.B_sl * ES, sl_C = (int)p.C_sl * ES, sl_z = (int)p.z_sl * ES, sl_o = (int)p.o_sl * ES;

    // ---- X of this wave's (head, half) goes out first, then the workgroup's share of the B / C rows ---------------------------
    const int cb = ((head_live ? h : 0) * 64 + half * 32 + thf * 16) * ES;   // byte offset of this lane's 16 staged channels in a row
    u32x4_t xq[SSD_MAXT][2];
    if (head_live) sf_x_issue(xq, r_x, sl_x, cb, 0, L, lane);
    sf_stage_bc<NK, 4>(Bl, Cl, r_B, r_C, sl_B, sl_C, 0, L, rows, tid, SSDW_THREADS);

    // ---- per-position scalars of a head by its first wave: dt = softplus(raw + bias), log-decay; row tables by wave 0 ---------
    float Ah = 0.0f, Dh = 0.0f;
    if (head_live) {
        Ah = p.A[h] * LOG2E;
        Dh = p.D ? p.D[h] : 0.0f;
    }
    if (head_live && half == 0) {
        const float bias = p.dt_bias ? p.dt_bias[h] : 0.0f;
        const T* __restrict__ dtp = (const T*)p.dt + (int64_t)sb * p.dt_sb + h;
#pragma unroll
        for (int k = 0; k < SSDW_TAB / WAVE; ++k) {
            const int l = lane + WAVE * k;
            float dtv = 0.0f;
            if (l < L) {
                const int zr = zidx ? zidx[l] : l;
                dtv = softplus_f(io<T>::ld(dtp + (int64_t)zr * p.dt_sl) + bias);
            }
            DT[l] = dtv;
            S2A[l] = Ah * dtv;
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < SSDW_TAB / WAVE; ++k) {
            const int l = lane + WAVE * k;
            zi_lds[l] = (l < L) ? (zidx ? zidx[l] : l) : 0;
            oi_lds[l] = (l < L) ? (oidx ? oidx[l] : l) : 0;
        }
    }
    __syncthreads();
    if (!head_live) return;                                              // (a finished wave no longer counts at the barriers below)

    int cur = 0;
#pragma unroll
    for (int off = 1; off < SSDW_TAB; off <<= 1) {                       // inclusive prefix sum (Hillis-Steele, one wave per head)
        if (half == 0) {
            const float* const src = S2A + cur * SSDW_TAB;
            float* const dst = S2A + (cur ^ 1) * SSDW_TAB;
#pragma unroll
            for (int k = 0; k < SSDW_TAB / WAVE; ++k) {
                const int l = lane + WAVE * k;
                dst[l] = src[l] + (l >= off ? src[l - off] : 0.0f);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    const float* const s2 = S2A;                                         // log2-domain log-decay prefix sums (eight steps: back in ping)
    float* const GD = S2A + SSDW_TAB;                                    // gamma_i dt_i = dt_i exp2(m_{it+1} - s2_i); 0 past the end
    if (half == 0) {
#pragma unroll
        for (int k = 0; k < SSDW_TAB / WAVE; ++k) {
            const int l = lane + WAVE * k;
            GD[l] = DT[l] * fast_exp2(s2[l | (SSD_TILE - 1)] - s2[l]);
        }
    }
    __syncthreads();
    auto m_of = [&](int t) -> float { return t == 0 ? 0.0f : s2[SSD_TILE * t - 1]; };   // log-decay just before tile t

    u32x4_t xfrag[SSD_MAXT][2];                                          // X as B-fragments of the output product, keys in accumulator order
    sf_x_frags(xfrag, xq, tile, L, lane);

    const bool z_rows16 = sf_gate_rows16(p.z, p.z_ss, p.z_sl);
    // fragments of the score product G^T = B_it C_lt^T: lane (row = col, kh) holds states 16k + 8kh .. +7 of slice k
    const uint8_t* const bl = Bl + col * PITCH + 16 * kh;
    const uint8_t* const cl = Cl + col * PITCH + 16 * kh;
#pragma unroll
    for (int lt = 0; lt < SSD_MAXT; ++lt) {                              // (fully unrolled: every fragment index is a compile-time constant)
        if (lt >= nt_l) break;
        const int lq = SSD_TILE * lt + col;                              // this lane's query in the score tile (a column of G^T)
        const int lqc = lq < L ? lq : L - 1;
        const float s2l = s2[lqc];
        u32x4_t zq[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};                // the gate tile of this query tile, in flight under the products
        const int lrow = SSD_TILE * lt + trow;
        const int lrc = lrow < L ? lrow : L - 1;
        if (p.z) sf_gate_issue(zq, r_z, zi_lds[lrc] * sl_z + cb, z_rows16);
        u32x4_t cfrag[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) cfrag[k] = *reinterpret_cast<const u32x4_t*>(cl + (SSD_TILE * lt) * PITCH + 32 * k);
        f32x16 yacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) yacc[r] = 0.0f;
        // ---- key tiles strictly before the query tile: factorised decay, applied to the accumulator ----
#pragma unroll
        for (int it = 0; it < SSD_MAXT - 1; ++it) {
            if (it < lt)                                                  // wave-uniform; alpha_l delta(lt, it) = exp2(s2_l - m_{it+1})
                sf_offdiag<O, NK>(yacc, bl + (SSD_TILE * it) * PITCH, cfrag, &GD[SSD_TILE * it + 4 * kh], fast_exp2(s2l - m_of(it + 1)), xfrag[it]);
        }
        // ---- the diagonal tile: dt, element-wise decay and causal mask on the accumulator of the unscaled operands ----
        sf_diag<O, true>(yacc, sf_scores<O, NK>(bl + (SSD_TILE * lt) * PITCH, cfrag), &s2[SSD_TILE * lt + 4 * kh], &DT[SSD_TILE * lt + 4 * kh],
                         SSD_TILE * lt + 4 * kh, lq, s2l, xfrag[lt]);
        // ---- epilogue of the query tile: + D x, gate, scatter, through the wave's one tile ----
        sf_epilogue<O, true>(yacc, xfrag[lt], Dh, p.z != nullptr, zq, tile, tile, r_o, sl_o, cb, &oi_lds[lrc], lrow < L, lane);
    }
}

template <typename T, int NK>
static int ssd_fwd_wide_launch(const dm_ssd_fwd_args& a, hipStream_t st) {
    if (const int rc = reserve_dynamic_lds<&ssd_fwd_wide_kernel<T, NK>>("dm_ssd_fwd", ssdw_lds_bytes(NK, SSD_MAXL))) return rc;
    const int rows = SSD_TILE * ((a.seqlen + SSD_TILE - 1) / SSD_TILE);
    dim3 grid((a.nheads + SSDW_HEADS - 1) / SSDW_HEADS, a.nseq), block(SSDW_THREADS);
    hipLaunchKernelGGL((ssd_fwd_wide_kernel<T, NK>), grid, block, ssdw_lds_bytes(NK, rows), st, a);
    return launch_status("dm_ssd_fwd");
}

template <typename T>
static int ssd_fwd_wide_dispatch(const dm_ssd_fwd_args& a, hipStream_t st) {
    switch (a.dstate) {
        case 32: return ssd_fwd_wide_launch<T, 2>(a, st);
        case 64: return ssd_fwd_wide_launch<T, 4>(a, st);
        default: return ssd_fwd_wide_launch<T, 8>(a, st);
    }
}

}  // namespace dm

extern "C" int dm_ssd_fwd_supported(int seqlen, int headdim, int dstate, int io_dtype) {
    const bool width = dstate == 16 || dstate == 32 || dstate == 64 || dstate == 128;
    return (seqlen >= 1 && seqlen <= dm::SSD_MAXL && headdim == 64 && width && (io_dtype == DM_BF16 || io_dtype == DM_F16)) ? 1 : 0;
}

extern "C" int dm_ssd_fwd(const dm_ssd_fwd_args* args, void* stream) {
    using namespace dm;
    if (const int rc = ssd_fwd_check("dm_ssd_fwd", args, dm_ssd_fwd_supported, SSD_MAXL, true)) return rc;
    const dm_ssd_fwd_args& a = *args;
    hipStream_t st = (hipStream_t)stream;
    if (a.dstate != 16) return a.io_dtype == DM_BF16 ? ssd_fwd_wide_dispatch<bf16_t>(a, st) : ssd_fwd_wide_dispatch<f16_t>(a, st);
    dim3 grid(a.nheads * 2, a.nseq), block(WAVE);          // two 32-column halves per head
    if (a.io_dtype == DM_BF16) hipLaunchKernelGGL((ssd_fwd_kernel<bf16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((ssd_fwd_kernel<f16_t>), grid, block, 0, st, a);
    return launch_status("dm_ssd_fwd");
}
