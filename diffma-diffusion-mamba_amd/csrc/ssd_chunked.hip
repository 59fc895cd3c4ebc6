// K6d  dm_ssd_fwd_chunked -- Mamba-2 state-space duality past one chunk, on the matrix pipe (forward, no-grad regime).
//
// Same operator and operands as dm_ssd_fwd (ssd.hip), for 1 <= L <= 1024: the sequence is walked in chunks of Q tokens by the same
// workgroup, the SSD state h [d_state x 64] of every head carried from chunk to chunk in fp32 registers.  With chunk-local log-decay
// prefix sums s (log2 domain: s2) and s_end the prefix sum at the chunk's last token:
//     y_l    = [ single-chunk dual form over the keys of l's own chunk ]  +  exp(s_l) sum_n C_l[n] h[n][p]  +  D x_l
//     h_next = exp(s_end) h  +  sum_{i in chunk} exp(s_end - s_i) dt_i B_i[n] x_i[p]                 out = y silu(z)
// Every decay factor is a true partial decay (<= 1).  The chunk body is ssd_fwd_wide_kernel's: the same blocks of ssd_fwd_common.h
// with the chunk's length in place of L (one workgroup per sequence and group of heads, the chunk's raw B / C rows staged in LDS
// once, one wave per (head, 32-column half) with the chunk's X fragments resident, gamma dt and alpha delta on the fp32
// accumulator) for every width NK = d_state / 16 in {1, 2, 4, 8}.  The two extra products reuse the fragments that body holds:
//   * state, kept as h^T tiles of 32 states x 32 channels (f32x16 per tile: N / 2 registers): row 4 kh + 8 r4 + r of a tile is
//     accumulator register 4 r4 + r, so registers 8 ks .. 8 ks + 7 rounded to the I/O dtype ARE the B-operand (K = states) of the
//     inter-chunk product [32 queries x N] [N x 32 channels], whose A-operand is the C row read from LDS in that same state order
//     (two 8-byte reads).  The 16-bit copy is rebuilt per query tile (8 conversions per MFMA), never held.  exp2(s2_l) multiplies the
//     fp32 result (per accumulator row), not the 16-bit rows.
//   * update [N x tokens] [tokens x 32 channels]: the resident X fragments (keys in accumulator order) are the token-contracted
//     B-operand; the per-key weight dt_i exp2(s2_end - s2_i) is indexed by the contraction and multiplies X (one 16-bit rounding
//     per element, once per fragment whatever the width); B^T comes from the staged rows through transposing LDS reads
//     (ds_read_tr16_b64: lane j of a 16-lane group supplies 4 states of token (j >> 2) and receives 4 tokens of state j).
//
// One 8-wave workgroup per (sequence, 4 heads), two waves per SIMD, at every width; the chunk length follows the register budget
// (bf16 registers; no instantiation spills; tools/kernel_regs.sh ssd_chunked):
//     d_state  16   Q 128   218 VGPRs   43 KB LDS
//     d_state  32   Q 128   226 VGPRs   51 KB LDS
//     d_state  64   Q  96   218 VGPRs   58 KB LDS      (Q 128: one accumulator tile spilled)
//     d_state 128   Q  64   249 VGPRs   65 KB LDS      (Q 128: 123 registers spilled)
// The chunk body needs about 200 registers by itself and the state N / 2 more; each tile less of a chunk frees 8 of X fragments and
// 8 in flight.  The inter-chunk term comes AFTER the diagonal tile, into an accumulator of its own: ahead of the score products it
// kept 13 registers too many alive at d_state 128.  Per 32 tokens the intra-chunk work is (T + 1) / 2 (NK + 2) MFMAs (T = Q / 32) and
// the two new products cost 2 NK whatever Q is, so a shorter chunk does less arithmetic, while every chunk pays one exposed round
// trip for its rows, its dt gather and two workgroup barriers.  Measured at d_state 128 against four-wave workgroups (2 heads) at one
// wave per SIMD with Q 128 (418 registers): 139 vs 243 us at L 256 and 556 vs 1050 us at L 1024 (nseq 192), equal at nseq 24.  Not
// chosen besides: a 16-bit state copy held across the chunk (N / 4 registers for 8 conversions per MFMA saved); weighting the B
// rows instead of X (NK / 2 times the conversions); a chunk-parallel decomposition (its state pass needs a second kernel or a
// grid-wide wait).
//
// Barriers: waves of heads past nheads leave before the first barrier and take no part in any staging; every remaining wave runs
// every chunk with the same, workgroup-uniform trip counts, so all of them meet the same barriers.  The barrier at the top of a
// chunk keeps the restaging of B / C and the tables behind the last reads of the chunk before.
#include <type_traits>
#include "ssd_fwd_common.h"

namespace dm {

constexpr int ssdc_t(int nk) { return nk == 8 ? 2 : (nk == 4 ? 3 : 4); }               // tiles per chunk
constexpr int ssdc_q(int nk) { return SSD_TILE * ssdc_t(nk); }                         // chunk length Q
constexpr int SSDC_TABLE = 128;                              // entries per per-position table (>= Q; two positions per lane of a wave)
constexpr int SSDC_MAXL = 1024;
constexpr int SSDC_HEADS = 4;                                // heads per workgroup (two waves each)
constexpr int SSDC_NTAB = 5;                                 // per head: s2 | gamma dt | dt | exp2(s2) | dt exp2(s2_end - s2)
constexpr int SSDC_TABS = 0;
constexpr int SSDC_IDX = SSDC_TABS + SSDC_HEADS * SSDC_NTAB * SSDC_TABLE * 4;          // z rows | out rows of the chunk (global)
constexpr int SSDC_TILES = SSDC_IDX + 2 * SSDC_TABLE * 4;                               // one 32 x 32 staging tile per wave
constexpr int SSDC_BC = SSDC_TILES + 2 * SSDC_HEADS * SSD_TILE * SSD_PITCH * 4;   // B rows, then C rows
constexpr int ssdc_lds_bytes(int nk, int rows) { return SSDC_BC + 2 * rows * ssd_bc_pitch(nk); }
static_assert(SSDC_TABLE == 2 * WAVE, "the table pass gives every lane two consecutive positions");
static_assert(ssdc_lds_bytes(8, ssdc_q(8)) <= 160 * 1024, "LDS of a CU");

typedef short ssdc_v4s __attribute__((ext_vector_type(4)));
typedef uint32_t ssdc_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) ssdc_v4s* ssdc_tr_ptr;

template <typename T, int NK>
__global__ __launch_bounds__(2 * WAVE * SSDC_HEADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void ssd_fwd_chunked_kernel(const dm_ssd_fwd_args p) {
    using O = mfma<T>;
    constexpr int ES = (int)sizeof(T);
    constexpr int PITCH = ssd_bc_pitch(NK);
    constexpr int PPR = 2 * NK;                                          // 16-byte pieces of a B / C row
    constexpr int NJ = (NK + 1) / 2;                                     // state tiles of 32 states (d_state 16: half a tile)
    constexpr int KS = NK == 1 ? 1 : 2;                                  // 16-state slices per state tile
    constexpr int SSDC_T = ssdc_t(NK), SSDC_Q = ssdc_q(NK);
    static_assert(SSDC_Q % 32 == 0 && SSDC_Q >= 64 && SSDC_Q <= 224 && SSDC_Q <= SSDC_TABLE, "chunk length");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & (WAVE - 1);
    const int col = lane & 31, kh = lane >> 5;
    const int trow = lane >> 1, thf = lane & 1;                          // staging role: row of the tile, 16-channel half of it
    const int hh = wave >> 1, half = wave & 1;
    const int h = blockIdx.x * SSDC_HEADS + hh, s = blockIdx.y;
    if (h >= p.nheads) return;                                           // surplus waves take no part: no barrier below counts them
    const int heads_here = min(SSDC_HEADS, p.nheads - (int)blockIdx.x * SSDC_HEADS);
    const int nthr = 2 * WAVE * heads_here;                              // the live waves are the workgroup's first 2 heads_here
    const int L = p.seqlen;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int nchunks = (L + SSDC_Q - 1) / SSDC_Q;
    const int rows_staged = L < SSDC_Q ? SSD_TILE * ((L + SSD_TILE - 1) / SSD_TILE) : SSDC_Q;   // as the launch sizes the LDS
    const int32_t* __restrict__ zidx = p.z_row_index ? p.z_row_index + (int64_t)dir * L : nullptr;
    const int32_t* __restrict__ oidx = p.out_row_index ? p.out_row_index + (int64_t)dir * L : nullptr;

    float* const S2 = reinterpret_cast<float*>(lds + SSDC_TABS) + hh * SSDC_NTAB * SSDC_TABLE;   // chunk-local log2-domain prefix sums
    float* const GD = S2 + SSDC_TABLE;                                       // gamma_i dt_i = dt_i exp2(m_{it+1} - s2_i); 0 past the end
    float* const DT = S2 + 2 * SSDC_TABLE;
    float* const EX = S2 + 3 * SSDC_TABLE;                                   // exp2(s2_l): the decay from the chunk's start to query l
    float* const WT = S2 + 4 * SSDC_TABLE;                                   // dt_i exp2(s2_end - s2_i): key i's weight in the next state
    int* const zi_lds = reinterpret_cast<int*>(lds + SSDC_IDX);
    int* const oi_lds = zi_lds + SSDC_TABLE;
    uint32_t* const tile = reinterpret_cast<uint32_t*>(lds + SSDC_TILES) + wave * (SSD_TILE * SSD_PITCH);
    uint8_t* const Bl = lds + SSDC_BC;
    uint8_t* const Cl = Bl + rows_staged * PITCH;

    const rsrc_t r_x = make_rsrc((const T*)p.x + (int64_t)s * p.x_ss);
    const rsrc_t r_B = make_rsrc((const T*)p.B + (int64_t)s * p.B_ss);
    const rsrc_t r_C = make_rsrc((const T*)p.C + (int64_t)s * p.C_ss);
    const rsrc_t r_z = make_rsrc(p.z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_o = make_rsrc((T*)p.out + (int64_t)s * p.o_ss);
    const int sl_x = (int)p.x_sl * ES, sl_B = (int)p.B_sl * ES, sl_C = (int)p.C_sl * ES, sl_z = (int)p.z_sl * ES, sl_o = (int)p.o_sl * ES;
    const int cb = (h * 64 + half * 32 + thf * 16) * ES;                 // byte offset of this lane's 16 staged channels in a row
    const float Ah = p.A[h] * LOG2E, Dh = p.D ? p.D[h] : 0.0f, bias = p.dt_bias ? p.dt_bias[h] : 0.0f;
    const T* __restrict__ dtp = (const T*)p.dt + (int64_t)sb * p.dt_sb + h;
    const bool z_rows16 = sf_gate_rows16(p.z, p.z_ss, p.z_sl);
    // fragments of the score product G^T = B_it C_lt^T: lane (row = col, kh) holds states 16k + 8kh .. +7 of slice k
    const uint8_t* const bl = Bl + col * PITCH + 16 * kh;
    const uint8_t* const cl = Cl + col * PITCH + 16 * kh;
    // the inter-chunk product's C rows in the state order of an h^T tile: lane (query = col, kh), slice ks of tile j holds states
    // 32 j + 16 ks + 4 kh + {0 .. 3} and those + 8
    const uint8_t* const cs = Cl + col * PITCH + 8 * kh;
    // B^T through transposing reads: lane (j = lane & 15) of a 16-lane group supplies the 8-byte piece (token + (j >> 2), states
    // c0 + 4 (j & 3) ..) and receives tokens + 0 .. 3 of state c0 + j; c0 = 16 ((lane >> 4) & 1) makes that state 32 j' + col
    const uint8_t* const bt = Bl + (4 * kh + ((lane & 15) >> 2)) * PITCH + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;

    f32x16 hacc[NJ];                                                     // h^T: hacc[j][4 r4 + r] = h[32 j + 4 kh + 8 r4 + r][this lane's channel]
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) hacc[j][r] = 0.0f;

    for (int c = 0; c < nchunks; ++c) {
        const int base = c * SSDC_Q;                                     // global index of the chunk's first token
        const int Lc = min(SSDC_Q, L - base);                            // tokens of this chunk (the last one may be ragged)
        const int nt_c = (Lc + SSD_TILE - 1) / SSD_TILE;
        const int rows = SSD_TILE * nt_c;

        // ---- X of this wave's (head, half) goes out first (kernel text, as the staging below: ssd_fwd_common.h says why) ---------
        u32x4_t xq[SSDC_T][2];
#pragma unroll
        for (int it = 0; it < SSDC_T; ++it) {
            const int i = SSD_TILE * it + trow;
            const int ic = base + (i < Lc ? i : Lc - 1);                  // rows past the end: clamped here, zeroed below
#pragma unroll
            for (int q = 0; q < 2; ++q) xq[it][q] = ld16(r_x, ic * sl_x + cb + 16 * q);
        }
        __syncthreads();                                                  // every wave is done with the rows and tables of the chunk before
        // ---- the live waves' share of the chunk's B / C rows ------------------------------------------------------------------
        {
            const int npieces = rows * PPR;                              // rows past the end are staged as copies of the last row
            for (int q0 = 0; q0 < npieces; q0 += 2 * nthr) {
                u32x4_t vb[2], vc[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int q = q0 + u * nthr + tid;
                    if (q < npieces) {
                        const int r = q / PPR, pc = q - r * PPR;
                        const int rc = base + (r < Lc ? r : Lc - 1);
                        vb[u] = ld16(r_B, rc * sl_B + 16 * pc);
                        vc[u] = ld16(r_C, rc * sl_C + 16 * pc);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int q = q0 + u * nthr + tid;
                    if (q < npieces) {
                        const int r = q / PPR, pc = q - r * PPR;
                        *reinterpret_cast<u32x4_t*>(Bl + r * PITCH + 16 * pc) = vb[u];
                        *reinterpret_cast<u32x4_t*>(Cl + r * PITCH + 16 * pc) = vc[u];
                    }
                }
            }
        }
        // ---- per-position scalars of a head by its first wave: lane owns positions 2 lane, 2 lane + 1 of the chunk.  dt =
        //      softplus(raw + bias) read through the GLOBAL table entry base + local; the prefix sums restart at every chunk ----
        if (half == 0) {
            float dtv[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int l = 2 * lane + e;
                dtv[e] = 0.0f;
                if (l < Lc) {
                    const int zr = zidx ? zidx[base + l] : base + l;
                    dtv[e] = softplus_f(io<T>::ld(dtp + (int64_t)zr * p.dt_sl) + bias);
                }
            }
            const float a0 = Ah * dtv[0], a1 = Ah * dtv[1];
            float inc = a0 + a1;                                         // inclusive prefix sum over the lanes' pair sums
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const float up = __shfl_up(inc, off, WAVE);
                if (lane >= off) inc += up;
            }
            const float before = __shfl_up(inc, 1, WAVE);                // s2 at 2 lane - 1
            const float sa = lane == 0 ? a0 : before + a0, s1 = inc;     // s2 at 2 lane and at 2 lane + 1: at most 8 additions each
            const float tile_end = __shfl(inc, lane | 15, WAVE);         // s2 at the last position of this lane's tile
            const float s_end = __shfl(inc, WAVE - 1, WAVE);             // s2 at the chunk's last position (flat past a ragged end)
            const float sv[2] = {sa, s1};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int l = 2 * lane + e;
                S2[l] = sv[e];
                DT[l] = dtv[e];
                GD[l] = dtv[e] * fast_exp2(tile_end - sv[e]);
                EX[l] = fast_exp2(sv[e]);
                WT[l] = dtv[e] * fast_exp2(s_end - sv[e]);
            }
        }
        if (wave == 0) {                                                 // (wave 0's head is always live)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int l = lane + WAVE * e;
                zi_lds[l] = (l < Lc) ? (zidx ? zidx[base + l] : base + l) : 0;
                oi_lds[l] = (l < Lc) ? (oidx ? oidx[base + l] : base + l) : 0;
            }
        }
        __syncthreads();
        const float* const s2 = S2;
        auto m_of = [&](int t) -> float { return t == 0 ? 0.0f : s2[SSD_TILE * t - 1]; };   // log-decay just before tile t of the chunk

        u32x4_t xfrag[SSDC_T][2];                                        // X as B-fragments, chunk keys in accumulator order
        sf_x_frags(xfrag, xq, tile, Lc, lane);

#pragma unroll
        for (int lt = 0; lt < SSDC_T; ++lt) {                            // (fully unrolled: every fragment index is a compile-time constant)
            if (lt >= nt_c) break;
            const int lq = SSD_TILE * lt + col;                         // this lane's query in the score tile (a column of G^T), chunk-local
            const int lqc = lq < Lc ? lq : Lc - 1;
            const float s2l = s2[lqc];
            u32x4_t zq[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};            // the gate tile of this query tile, in flight under the products
            const int lrow = SSD_TILE * lt + trow;
            const int lrc = lrow < Lc ? lrow : Lc - 1;
            if (p.z) sf_gate_issue(zq, r_z, zi_lds[lrc] * sl_z + cb, z_rows16);
            f32x16 yacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[r] = 0.0f;
            u32x4_t cfrag[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) cfrag[k] = *reinterpret_cast<const u32x4_t*>(cl + (SSD_TILE * lt) * PITCH + 32 * k);
            // ---- key tiles of the chunk strictly before the query tile: factorised decay, applied to the accumulator ----
#pragma unroll
            for (int it = 0; it < SSDC_T - 1; ++it) {
                if (it < lt)                                              // wave-uniform; alpha_l delta(lt, it) = exp2(s2_l - m_{it+1})
                    sf_offdiag<O, NK>(yacc, bl + (SSD_TILE * it) * PITCH, cfrag, &GD[SSD_TILE * it + 4 * kh], fast_exp2(s2l - m_of(it + 1)), xfrag[it]);
            }
            // ---- the diagonal tile: dt, element-wise decay and causal mask on the accumulator of the unscaled operands ----
            sf_diag<O, true>(yacc, sf_scores<O, NK>(bl + (SSD_TILE * lt) * PITCH, cfrag), &s2[SSD_TILE * lt + 4 * kh], &DT[SSD_TILE * lt + 4 * kh],
                             SSD_TILE * lt + 4 * kh, lq, s2l, xfrag[lt]);
            // ---- inter-chunk term: C_l (state order of the h^T tiles) times the carried state rounded to the I/O dtype, then
            //      exp2(s2_l) per accumulator row on the fp32 result ----
            if (c > 0) {                                                  // wave-uniform
                f32x16 yi;
#pragma unroll
                for (int r = 0; r < 16; ++r) yi[r] = 0.0f;
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const uint8_t* const cp = cs + (SSD_TILE * lt) * PITCH + (32 * j + 16 * ks) * 2;
                        const ssdc_u32x2 c0 = *reinterpret_cast<const ssdc_u32x2*>(cp), c1 = *reinterpret_cast<const ssdc_u32x2*>(cp + 16);
                        const u32x4_t cf = {c0.x, c0.y, c1.x, c1.y};
                        u32x4_t hb;
#pragma unroll
                        for (int w = 0; w < 4; ++w) hb[w] = O::pack(hacc[j][8 * ks + 2 * w], hacc[j][8 * ks + 2 * w + 1]);
                        yi = O::m32(cf, hb, yi);
                    }
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 ex = *reinterpret_cast<const f32x4*>(&EX[SSD_TILE * lt + 4 * kh + 8 * r4]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) yacc[4 * r4 + r] += yi[4 * r4 + r] * ex[r];
                }
            }
            // ---- epilogue of the query tile: + D x, gate, scatter through the chunk's table (global rows: built from entries base + local) ----
            sf_epilogue<O, true>(yacc, xfrag[lt], Dh, p.z != nullptr, zq, tile, tile, r_o, sl_o, cb, &oi_lds[lrc], lrow < Lc, lane);
        }

        // ---- the state after this chunk (a chunk that has a successor is full): h = exp2(s2_end) h + (B^T)(w .* X) -------------
        if (c + 1 < nchunks) {                                            // workgroup-uniform
            const float dec = fast_exp2(s2[SSDC_Q - 1]);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) hacc[j][r] *= dec;
#pragma unroll
            for (int it = 0; it < SSDC_T; ++it)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(&WT[SSD_TILE * it + 4 * kh + 16 * ks]);
                    const f32x4 w1 = *reinterpret_cast<const f32x4*>(&WT[SSD_TILE * it + 4 * kh + 16 * ks + 8]);
                    const u32x4_t xf = xfrag[it][ks];
                    const u32x4_t xw = {O::pack(O::lo(xf[0]) * w0[0], O::hi(xf[0]) * w0[1]), O::pack(O::lo(xf[1]) * w0[2], O::hi(xf[1]) * w0[3]),
                                        O::pack(O::lo(xf[2]) * w1[0], O::hi(xf[2]) * w1[1]), O::pack(O::lo(xf[3]) * w1[2], O::hi(xf[3]) * w1[3])};
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const uint8_t* const bp = bt + (SSD_TILE * it + 16 * ks) * PITCH + 64 * j;
                        const ssdc_v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ssdc_tr_ptr)bp);
                        const ssdc_v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ssdc_tr_ptr)(bp + 8 * PITCH));
                        const ssdc_u32x2 v0 = __builtin_bit_cast(ssdc_u32x2, a0), v1 = __builtin_bit_cast(ssdc_u32x2, a1);
                        u32x4_t bf = {v0.x, v0.y, v1.x, v1.y};
                        if (NK == 1 && col >= 16) bf = (u32x4_t){0u, 0u, 0u, 0u};   // d_state 16: rows 16 .. 31 of the one state tile do not exist
                        hacc[j] = O::m32(bf, xw, hacc[j]);
                    }
                }
        }
    }
}

template <typename T, int NK>
static int ssd_fwd_chunked_launch(const dm_ssd_fwd_args& a, hipStream_t st) {
    constexpr int Q = ssdc_q(NK);
    if (const int rc = reserve_dynamic_lds<&ssd_fwd_chunked_kernel<T, NK>>("dm_ssd_fwd_chunked", ssdc_lds_bytes(NK, Q))) return rc;
    const int rows = a.seqlen < Q ? SSD_TILE * ((a.seqlen + SSD_TILE - 1) / SSD_TILE) : Q;
    dim3 grid((a.nheads + SSDC_HEADS - 1) / SSDC_HEADS, a.nseq), block(2 * WAVE * SSDC_HEADS);
    hipLaunchKernelGGL((ssd_fwd_chunked_kernel<T, NK>), grid, block, ssdc_lds_bytes(NK, rows), st, a);
    return launch_status("dm_ssd_fwd_chunked");
}

template <typename T>
static int ssd_fwd_chunked_dispatch(const dm_ssd_fwd_args& a, hipStream_t st) {
    switch (a.dstate) {
        case 16: return ssd_fwd_chunked_launch<T, 1>(a, st);
        case 32: return ssd_fwd_chunked_launch<T, 2>(a, st);
        case 64: return ssd_fwd_chunked_launch<T, 4>(a, st);
        default: return ssd_fwd_chunked_launch<T, 8>(a, st);
    }
}

}  // namespace dm

extern "C" int dm_ssd_fwd_chunk_len(int dstate) {
    return (dstate == 16 || dstate == 32 || dstate == 64 || dstate == 128) ? dm::ssdc_q(dstate / 16) : 0;
}

extern "C" int dm_ssd_fwd_chunked_supported(int seqlen, int headdim, int dstate, int io_dtype) {
    return (seqlen >= 1 && seqlen <= dm::SSDC_MAXL && headdim == 64 && dm_ssd_fwd_chunk_len(dstate) > 0 && (io_dtype == DM_BF16 || io_dtype == DM_F16)) ? 1 : 0;
}

extern "C" int dm_ssd_fwd_chunked(const dm_ssd_fwd_args* args, void* stream) {
    using namespace dm;
    static_assert(SSDC_MAXL == DM_SSD_FWD_CHUNKED_MAXL, "the header states the cap");
    if (const int rc = ssd_fwd_check("dm_ssd_fwd_chunked", args, dm_ssd_fwd_chunked_supported, SSDC_MAXL, false)) return rc;
    const dm_ssd_fwd_args& a = *args;
    hipStream_t st = (hipStream_t)stream;
    return a.io_dtype == DM_BF16 ? ssd_fwd_chunked_dispatch<bf16_t>(a, st) : ssd_fwd_chunked_dispatch<f16_t>(a, st);
}
