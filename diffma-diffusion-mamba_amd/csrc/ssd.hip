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
#include "dm_mfma.h"

namespace dm {

constexpr int SSD_TILE = 32;
constexpr int SSD_MAXT = 7;                       // L <= 224
constexpr int SSD_MAXL = SSD_TILE * SSD_MAXT;
constexpr int SSD_PITCH = 20;                     // dwords per staged tile row (32 channels = 16 dwords, +4 pad)

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
    // 32-row x 32-channel staging tiles (row pitch 80 B: the two key halves of a fragment read land on disjoint banks): global
    // traffic is whole 16-byte pieces of a row, the (key, channel) element order of the fragments is produced by LDS reads
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
        for (int q = 0; q < 2; ++q) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_x, ic * sl_x + cb + 16 * q, 0, 0);
            xq[it][q] = (u32x4_t){v[0], v[1], v[2], v[3]};
        }
        const int j = SSD_TILE * it + col;
        const int jc = j < L ? j : L - 1;
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_B, jc * sl_B + kh * 8 * ES, 0, 0);
        bq[it] = (u32x4_t){v[0], v[1], v[2], v[3]};
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
    // X as B-fragments of the output product, keys in accumulator order: slot e of (it, ks) is key 32it + 4kh + 8(2ks + e/4) + e%4
    u32x4_t xfrag[SSD_MAXT][2];
    {
        const uint16_t* const ta16 = reinterpret_cast<const uint16_t*>(tile_a);
#pragma unroll
        for (int it = 0; it < SSD_MAXT; ++it) {
            const bool live = SSD_TILE * it + trow < L;
#pragma unroll
            for (int q = 0; q < 2; ++q)
                *reinterpret_cast<u32x4_t*>(&tile_a[trow * SSD_PITCH + thf * 8 + 4 * q]) = live ? xq[it][q] : (u32x4_t){0u, 0u, 0u, 0u};
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint32_t w4[4];
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    const int k0 = 4 * kh + 8 * (2 * ks + (e2 >> 1)) + 2 * (e2 & 1);
                    const uint32_t lo = ta16[k0 * (2 * SSD_PITCH) + col], hi = ta16[(k0 + 1) * (2 * SSD_PITCH) + col];
                    w4[e2] = lo | (hi << 16);
                }
                xfrag[it][ks] = (u32x4_t){w4[0], w4[1], w4[2], w4[3]};
            }
            __syncthreads();
        }
    }

    // C rows (the B-operand of the score product: lane (col l, kh) holds C[l][8kh .. +7]) and the unscaled B rows of the diagonal
    // tile are fetched one query tile ahead
    auto load_cb = [&](int t, u32x4_t& c, u32x4_t& b) {
        const int j = SSD_TILE * t + col;
        const int jc = j < L ? j : L - 1;
        const auto vc = __builtin_amdgcn_raw_buffer_load_b128(r_C, jc * sl_C + kh * 8 * ES, 0, 0);
        const auto vb = __builtin_amdgcn_raw_buffer_load_b128(r_B, jc * sl_B + kh * 8 * ES, 0, 0);
        c = (u32x4_t){vc[0], vc[1], vc[2], vc[3]};
        b = (u32x4_t){vb[0], vb[1], vb[2], vb[3]};
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
        if (p.z) {
            const int zr = zi_lds[lrc];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_z, zr * sl_z + cb + 16 * q, 0, 0);
                zq[q] = (u32x4_t){v[0], v[1], v[2], v[3]};
            }
        }
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
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                    yacc = O::m32(wf, xfrag[it][ks], yacc);
                }
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
            uint32_t wp[8];
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 si = *reinterpret_cast<const f32x4*>(&s2[SSD_TILE * lt + 4 * kh + 8 * r4]);
                float wv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ik = SSD_TILE * lt + 4 * kh + 8 * r4 + r;
                    wv[r] = (ik <= lq) ? g[4 * r4 + r] * fast_exp2(s2l - si[r]) : 0.0f;
                }
                wp[2 * r4] = O::pack(wv[0], wv[1]);
                wp[2 * r4 + 1] = O::pack(wv[2], wv[3]);
            }
#pragma unroll
            for (int it = 0; it < SSD_MAXT; ++it) {                       // (compile-time index into xfrag)
                if (it == lt) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                        yacc = O::m32(wf, xfrag[it][ks], yacc);
                    }
                }
            }
        }
        // ---- epilogue of the query tile: + D x, gate, scatter.  yacc[4 r4 + r] = Y[32lt + 4kh + 8 r4 + r][this lane's channel] ----
        if (p.z) {
#pragma unroll
            for (int q = 0; q < 2; ++q) *reinterpret_cast<u32x4_t*>(&tile_a[trow * SSD_PITCH + thf * 8 + 4 * q]) = zq[q];
        }
        __syncthreads();
        {
            const uint16_t* const ta16 = reinterpret_cast<const uint16_t*>(tile_a);
            uint16_t* const tb16 = reinterpret_cast<uint16_t*>(tile_b);
#pragma unroll
            for (int it = 0; it < SSD_MAXT; ++it) {                       // (compile-time index into xfrag)
                if (it == lt) {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * kh + 8 * r4 + r;
                            const int e = 4 * (r4 & 1) + r;
                            const uint32_t xw = xfrag[it][r4 >> 1][e >> 1];
                            const float xv = (e & 1) ? O::hi(xw) : O::lo(xw);
                            float y = yacc[4 * r4 + r] + Dh * xv;
                            if (p.z) y *= silu_f(O::lo((uint32_t)ta16[row * (2 * SSD_PITCH) + col]));
                            tb16[row * (2 * SSD_PITCH) + col] = (uint16_t)(O::pack(y, 0.0f) & 0xffffu);
                        }
                }
            }
        }
        __syncthreads();
        if (lrow < L) {
            const int orow = oi_lds[lrow];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32x4_t v = *reinterpret_cast<const u32x4_t*>(&tile_b[trow * SSD_PITCH + thf * 8 + 4 * q]);
                __builtin_amdgcn_raw_buffer_store_b128(v, r_o, orow * sl_o + cb + 16 * q, 0, 0);
            }
        }
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
constexpr int ssdw_pitch(int nk) { return 32 * nk + 16; }                           // bytes per staged B / C row
constexpr int ssdw_lds_bytes(int nk, int rows) { return SSDW_BC + 2 * rows * ssdw_pitch(nk); }
static_assert(SSDW_TAB >= SSD_MAXL && SSDW_TAB % WAVE == 0 && SSDW_TAB == 256, "eight doubling steps leave the prefix sums in the ping table");
static_assert(ssdw_lds_bytes(8, SSD_MAXL) <= 160 * 1024, "LDS of a CU");

template <typename T, int NK>
__global__ __launch_bounds__(SSDW_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void ssd_fwd_wide_kernel(const dm_ssd_fwd_args p) {
    using O = mfma<T>;
    constexpr int ES = (int)sizeof(T);
    constexpr int PITCH = ssdw_pitch(NK);
    constexpr int PPR = 2 * NK;                                          // 16-byte pieces of a B / C row
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
    if (head_live) {
#pragma unroll
        for (int it = 0; it < SSD_MAXT; ++it) {
            const int i = SSD_TILE * it + trow;
            const int ic = i < L ? i : L - 1;                             // rows past the end: clamped here, zeroed below
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_x, ic * sl_x + cb + 16 * q, 0, 0);
                xq[it][q] = (u32x4_t){v[0], v[1], v[2], v[3]};
            }
        }
    }
    {
        const int npieces = rows * PPR;                                  // rows past the end are staged as copies of the last row
        for (int q0 = 0; q0 < npieces; q0 += 4 * SSDW_THREADS) {
            u32x4_t vb[4], vc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u * SSDW_THREADS + tid;
                if (q < npieces) {
                    const int r = q / PPR, pc = q - r * PPR;
                    const int rc = r < L ? r : L - 1;
                    const auto b = __builtin_amdgcn_raw_buffer_load_b128(r_B, rc * sl_B + 16 * pc, 0, 0);
                    const auto c = __builtin_amdgcn_raw_buffer_load_b128(r_C, rc * sl_C + 16 * pc, 0, 0);
                    vb[u] = (u32x4_t){b[0], b[1], b[2], b[3]};
                    vc[u] = (u32x4_t){c[0], c[1], c[2], c[3]};
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u * SSDW_THREADS + tid;
                if (q < npieces) {
                    const int r = q / PPR, pc = q - r * PPR;
                    *reinterpret_cast<u32x4_t*>(Bl + r * PITCH + 16 * pc) = vb[u];
                    *reinterpret_cast<u32x4_t*>(Cl + r * PITCH + 16 * pc) = vc[u];
                }
            }
        }
    }

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

    // ---- X as B-fragments of the output product, keys in accumulator order: slot e of (it, ks) is key 32it + 4kh + 8(2ks + e/4) + e%4
    u32x4_t xfrag[SSD_MAXT][2];
    {
        const uint16_t* const t16 = reinterpret_cast<const uint16_t*>(tile);
#pragma unroll
        for (int it = 0; it < SSD_MAXT; ++it) {
            const bool row_live = SSD_TILE * it + trow < L;
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

    // the gate is a view of the in_proj output, whose rows are 2 Din + 2 N + H elements: a multiple of 8 with the factory models' 16 or
    // 24 heads, not with the two heads of a d_model 64 mixer
    const bool z_rows16 = (((uintptr_t)p.z & 15) | (uintptr_t)(p.z_ss & 7) | (uintptr_t)(p.z_sl & 7)) == 0;
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
        if (p.z) {
            const int zr = zi_lds[lrc];
            if (z_rows16) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_z, zr * sl_z + cb + 16 * q, 0, 0);
                    zq[q] = (u32x4_t){v[0], v[1], v[2], v[3]};
                }
            } else {                                                      // rows on 4-byte boundaries only: the same 32 bytes as dwords
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int w = 0; w < 4; ++w) zq[q][w] = __builtin_amdgcn_raw_buffer_load_b32(r_z, zr * sl_z + cb + 16 * q + 4 * w, 0, 0);
            }
        }
        u32x4_t cfrag[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) cfrag[k] = *reinterpret_cast<const u32x4_t*>(cl + (SSD_TILE * lt) * PITCH + 32 * k);
        f32x16 yacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) yacc[r] = 0.0f;
        // ---- key tiles strictly before the query tile: factorised decay, applied to the accumulator ----
#pragma unroll
        for (int it = 0; it < SSD_MAXT - 1; ++it) {
            if (it < lt) {                                                // wave-uniform
                f32x16 g;
#pragma unroll
                for (int r = 0; r < 16; ++r) g[r] = 0.0f;
#pragma unroll
                for (int k = 0; k < NK; ++k) {                           // rows = keys 32it + 4kh + 8r4 + r, columns = queries
                    const u32x4_t bf = *reinterpret_cast<const u32x4_t*>(bl + (SSD_TILE * it) * PITCH + 32 * k);
                    g = O::m32(bf, cfrag[k], g);
                }
                const float ad = fast_exp2(s2l - m_of(it + 1));          // alpha_l delta(lt, it)
                uint32_t wp[8];
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 gd = *reinterpret_cast<const f32x4*>(&GD[SSD_TILE * it + 4 * kh + 8 * r4]);
                    wp[2 * r4] = O::pack(g[4 * r4] * (gd[0] * ad), g[4 * r4 + 1] * (gd[1] * ad));
                    wp[2 * r4 + 1] = O::pack(g[4 * r4 + 2] * (gd[2] * ad), g[4 * r4 + 3] * (gd[3] * ad));
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                    yacc = O::m32(wf, xfrag[it][ks], yacc);
                }
            }
        }
        // ---- the diagonal tile: dt, element-wise decay and causal mask on the accumulator of the unscaled operands ----
        {
            f32x16 g;
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = 0.0f;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const u32x4_t bf = *reinterpret_cast<const u32x4_t*>(bl + (SSD_TILE * lt) * PITCH + 32 * k);
                g = O::m32(bf, cfrag[k], g);
            }
            uint32_t wp[8];
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 si = *reinterpret_cast<const f32x4*>(&s2[SSD_TILE * lt + 4 * kh + 8 * r4]);
                const f32x4 di = *reinterpret_cast<const f32x4*>(&DT[SSD_TILE * lt + 4 * kh + 8 * r4]);
                float wv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ik = SSD_TILE * lt + 4 * kh + 8 * r4 + r;
                    wv[r] = (ik <= lq) ? g[4 * r4 + r] * (di[r] * fast_exp2(s2l - si[r])) : 0.0f;
                }
                wp[2 * r4] = O::pack(wv[0], wv[1]);
                wp[2 * r4 + 1] = O::pack(wv[2], wv[3]);
            }
#pragma unroll
            for (int it = 0; it < SSD_MAXT; ++it) {                       // (compile-time index into xfrag)
                if (it == lt) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                        yacc = O::m32(wf, xfrag[it][ks], yacc);
                    }
                }
            }
        }
        // ---- epilogue of the query tile: + D x, gate, scatter.  yacc[4 r4 + r] = Y[32lt + 4kh + 8 r4 + r][this lane's channel].
        // One tile per wave: the lane that reads gate element (row, col) is the lane that writes the output element there. ----
        __syncthreads();                                                  // the previous query tile's row reads are done
        if (p.z) {
#pragma unroll
            for (int q = 0; q < 2; ++q) *reinterpret_cast<u32x4_t*>(&tile[trow * SSD_PITCH + thf * 8 + 4 * q]) = zq[q];
        }
        __syncthreads();
        {
            uint16_t* const t16 = reinterpret_cast<uint16_t*>(tile);
#pragma unroll
            for (int it = 0; it < SSD_MAXT; ++it) {                       // (compile-time index into xfrag)
                if (it == lt) {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 4 * kh + 8 * r4 + r;
                            const int e = 4 * (r4 & 1) + r;
                            const uint32_t xw = xfrag[it][r4 >> 1][e >> 1];
                            const float xv = (e & 1) ? O::hi(xw) : O::lo(xw);
                            float y = yacc[4 * r4 + r] + Dh * xv;
                            if (p.z) y *= silu_f(O::lo((uint32_t)t16[row * (2 * SSD_PITCH) + col]));
                            t16[row * (2 * SSD_PITCH) + col] = (uint16_t)(O::pack(y, 0.0f) & 0xffffu);
                        }
                }
            }
        }
        __syncthreads();
        if (lrow < L) {
            const int orow = oi_lds[lrow];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const u32x4_t v = *reinterpret_cast<const u32x4_t*>(&tile[trow * SSD_PITCH + thf * 8 + 4 * q]);
                __builtin_amdgcn_raw_buffer_store_b128(v, r_o, orow * sl_o + cb + 16 * q, 0, 0);
            }
        }
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
    if (!args) { set_error("dm_ssd_fwd: null args"); return DM_ERR_ARG; }
    const dm_ssd_fwd_args& a = *args;
    if (!a.x || !a.B || !a.C || !a.dt || !a.A || !a.out) { set_error("dm_ssd_fwd: null tensor pointer"); return DM_ERR_ARG; }
    if (a.nseq <= 0 || a.nheads <= 0 || a.seqlen <= 0) { set_error("dm_ssd_fwd: non-positive size"); return DM_ERR_ARG; }
    if (!dm_ssd_fwd_supported(a.seqlen, a.headdim, a.dstate, a.io_dtype)) {
        set_error("dm_ssd_fwd: needs 16-bit I/O, headdim 64, d_state 16 / 32 / 64 / 128, seqlen <= %d (got L %d P %d N %d dtype %d)", SSD_MAXL, a.seqlen, a.headdim, a.dstate, a.io_dtype);
        return DM_ERR_ARG;
    }
    if (a.nseq > 65535) { set_error("dm_ssd_fwd: nseq %d > 65535", a.nseq); return DM_ERR_ARG; }
    if (a.batch_per_dir > 0 && a.nseq % a.batch_per_dir != 0) { set_error("dm_ssd_fwd: nseq %% batch_per_dir != 0"); return DM_ERR_ARG; }
    if ((a.z_row_index == nullptr) != (a.out_row_index == nullptr)) { set_error("dm_ssd_fwd: both row-index tables or neither"); return DM_ERR_ARG; }
    if (((uintptr_t)a.B & 15) || ((uintptr_t)a.C & 15) || (a.B_ss & 7) || (a.B_sl & 7) || (a.C_ss & 7) || (a.C_sl & 7)) {
        set_error("dm_ssd_fwd: B / C rows must be 16-byte aligned"); return DM_ERR_LAYOUT;
    }
    if (((uintptr_t)a.x & 15) || ((uintptr_t)a.out & 15) || (a.x_ss & 7) || (a.x_sl & 7) || (a.o_ss & 7) || (a.o_sl & 7) ||
        (a.z && a.dstate == 16 && (((uintptr_t)a.z & 15) || (a.z_ss & 7) || (a.z_sl & 7)))) {
        set_error("dm_ssd_fwd: x / z / out rows must be 16-byte aligned (tiles move as 16-byte pieces)"); return DM_ERR_LAYOUT;
    }
    if (a.z && a.dstate != 16 && (((uintptr_t)a.z & 3) || (a.z_ss & 1) || (a.z_sl & 1))) {
        set_error("dm_ssd_fwd: z rows must be 4-byte aligned at d_state %d", a.dstate); return DM_ERR_LAYOUT;
    }
    hipStream_t st = (hipStream_t)stream;
    if (a.dstate != 16) return a.io_dtype == DM_BF16 ? ssd_fwd_wide_dispatch<bf16_t>(a, st) : ssd_fwd_wide_dispatch<f16_t>(a, st);
    dim3 grid(a.nheads * 2, a.nseq), block(WAVE);          // two 32-column halves per head
    if (a.io_dtype == DM_BF16) hipLaunchKernelGGL((ssd_fwd_kernel<bf16_t>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((ssd_fwd_kernel<f16_t>), grid, block, 0, st, a);
    return launch_status("dm_ssd_fwd");
}
