// K6b  dm_ssd_bwd -- backward of the Mamba-2 single-chunk SSD core on the matrix pipe (twin of ssd.hip).
//
// Operator (reference call block/mamba2.py:392-410 under autograd), per (sequence, head), L <= 196, P = 64, N = 16:
//     dt = softplus(raw + bias),  s_l = A * cumsum(dt)_l,  M[l,i] = exp(s_l - s_i) [i <= l],  G = C B^T,  W = G .* M .* dt_i
//     Y = W X,   u = Y + D X,   out = u .* silu(z)
// Gradients, with gY = dout .* silu(z) and R = gY X^T (K = headdim):
//     dz = dout .* u .* silu'(z)                        dX = W^T gY + D gY                 dD = sum gY .* X
//     dG = R .* M .* dt_i:   dC = dG B,  dB = dG^T C    (partial per head; B and C are shared by the heads)
//     V  = R .* G .* M:      ds_l = sum_i V[l,i] dt_i - dt_l sum_q V[q,l];   d dt_i = sum_l V[l,i] + A * sum_{l >= i} ds_l
//     dA = sum_l ds_l cumsum(dt)_l;    d raw = d dt * sigmoid(raw + bias)
// Nothing is saved by the forward.  One 256-thread workgroup per (sequence, head) holds X, gY, B, C row-major in 79 KB of LDS
// (TWO workgroups per CU: the load / compute / store phases of different heads overlap) and walks the 28 causal 32 x 32 tile
// pairs twice, concurrently:
//   * waves 0-1, "T" orientation (score tile with keys as rows, queries as columns): its accumulator registers are the
//     A-operand of  Y += W X  and  dC += dG B  -- they own query tiles {6,3,2,0} and {5,4,1} (15 / 13 pairs);
//   * waves 2-3, "N" orientation (queries as rows, keys as columns): accumulators are the A-operand of  dX += W^T gY  and
//     dB += dG^T C  -- they own key tiles {0,3,4,6} and {1,2,5}.
// Each orientation computes its own G (1 MFMA) and R (4 MFMAs, K = 64) per pair, applies the decay (factorised per tile pair as in
// the forward: alpha_l * delta(lt,it) * gamma_i off the diagonal, element-wise exp + causal mask on the 7 diagonal tiles), feeds
// the rounded tiles straight back (no LDS round trip), and accumulates the row sums (T) / column sums (N) of V that d dt and dA
// need.  The second products contract over sequence positions, i.e. they want X / gY / B / C with positions in the K slots: instead
// of transposed LDS copies, the row-major fragments already loaded for R (rows = positions, K = channels) are multiplied by 0/1
// selector fragments -- the result X[position][channel] comes out in accumulator layout, which IS that B-operand layout (exact:
// one product by 1.0 per element).  16 MFMAs and ~160 VALU per pair and orientation.  Tile epilogues turn 8 rows at a time through a 2 KB staging tile so
// every global access is a 16-byte piece of a row.  The final d dt / dA reverse cumulative sum runs on the whole workgroup
// (shuffle scans inside the waves, one barrier).  Measured and profiled: DESIGN.md section 3 (K6b), profiles/r02_pmc_scan_kernels.txt.
#include "ssd_bwd_common.h"

namespace dm {

// LDS map (byte offsets); rows [L, 196] of the operand arrays are zero
constexpr int SB_XS = 0;                          // X   [197][64]  16-byte chunks XOR-swizzled by (row & 7)
constexpr int SB_GS = SB_XS + SB_ROWS * 128;      // gY  [197][64]  same layout
constexpr int SB_BS = SB_GS + SB_ROWS * 128;      // B   [197][16]
constexpr int SB_CS = SB_BS + SB_ROWS * 32;       // C   [197][16]
constexpr int SB_TAIL = SB_CS + SB_ROWS * 32;     // tables, staging tiles, scratch (ssd_bwd_common.h)
constexpr int SB_LDS_BYTES = SB_TAIL + SB_T_BYTES;
static_assert(SB_LDS_BYTES <= 80 * 1024, "two workgroups per CU");
static_assert(SB_TAIL % 16 == 0, "16-byte aligned LDS arrays");

// 8 states of a B / C row
__device__ __forceinline__ u32x4_t bc_frag(const uint8_t* base, int row, int kh) {
    const int rc = row < SB_MAXL ? row : SB_MAXL;
    return *reinterpret_cast<const u32x4_t*>(base + rc * 32 + kh * 16);
}

template <typename T>
__global__ __launch_bounds__(SB_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void ssd_bwd_kernel(const dm_ssd_bwd_args p) {
    using O = mfma<T>;
    constexpr int ES = (int)sizeof(T);
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sb_tables t(lds + SB_TAIL, w);
    const auto [DT, CUM, S2, ALPHA, GAM, GDT, SIG, RS, CSV, zi, oi, stage, red] = t;
    const int h = blockIdx.x, s = blockIdx.y;
    const int L = p.seqlen;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int nt_l = (L + SB_TILE - 1) / SB_TILE;
    const int32_t* __restrict__ zidx = p.z_row_index ? p.z_row_index + (int64_t)dir * L : nullptr;
    const int32_t* __restrict__ oidx = p.out_row_index ? p.out_row_index + (int64_t)dir * L : nullptr;
    const float Ah = p.A[h], a2 = Ah * LOG2E, Dh = p.D ? p.D[h] : 0.0f, bias = p.dt_bias ? p.dt_bias[h] : 0.0f;
    const rsrc_t r_x = make_rsrc((const T*)p.x + (int64_t)s * p.x_ss);
    const rsrc_t r_B = make_rsrc((const T*)p.B + (int64_t)s * p.B_ss);
    const rsrc_t r_C = make_rsrc((const T*)p.C + (int64_t)s * p.C_ss);
    const rsrc_t r_z = make_rsrc(p.z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_do = make_rsrc((const T*)p.dout + (int64_t)s * p.do_ss);
    const rsrc_t r_dx = make_rsrc((T*)p.dx + (int64_t)s * p.dx_ss);
    const rsrc_t r_dz = make_rsrc(p.dz ? (T*)p.dz + (int64_t)s * p.dz_ss : nullptr);
    const T* __restrict__ dtp = (const T*)p.dt + (int64_t)sb * p.dt_sb + h;
    const int sl_B = (int)p.B_sl * ES, sl_C = (int)p.C_sl * ES, sl_z = (int)p.z_sl * ES;
    const int sl_do = (int)p.do_sl * ES, sl_dx = (int)p.dx_sl * ES, sl_dz = (int)p.dz_sl * ES;
    const int hb = h * 64 * ES;                                                   // byte offset of the head's columns in a row
    float* const dbc_part = p.dBC_part + ((int64_t)h * p.nseq + s) * L * 32;          // head-major: the caller's sum over heads is a column sum

    // ---- phases 0 + 1: the load front (ssd_bwd_common.h), with B / C at its level 1 -----------------------------------------------
    u32x4_t bq[2], cq[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {                                                 // B / C: two 16-byte chunks per row, two rows per thread
        const int e = tid + SB_THREADS * i;
        const int r = e >> 1, hf = e & 1;
        const int rc = r < L ? r : L - 1;
        const auto b = __builtin_amdgcn_raw_buffer_load_b128(r_B, rc * sl_B + hf * 16, 0, 0);
        const auto c = __builtin_amdgcn_raw_buffer_load_b128(r_C, rc * sl_C + hf * 16, 0, 0);
        bq[i] = (u32x4_t){b[0], b[1], b[2], b[3]};
        cq[i] = (u32x4_t){c[0], c[1], c[2], c[3]};
    }
    sb_front f;
    sb_front_issue(f, p, r_x, r_do, zidx, oidx, dtp, hb, tid, lane, w, [&](int byte_off) -> u32x4_t { return ld16(r_z, byte_off); });
    // B / C into LDS (level 1 has landed by the time the dt value is needed)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + SB_THREADS * i;
        const int r = e >> 1, hf = e & 1;
        if (r < SB_ROWS) {
            const u32x4_t zero4 = {0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4_t*>(lds + SB_BS + r * 32 + hf * 16) = r < L ? bq[i] : zero4;
            *reinterpret_cast<u32x4_t*>(lds + SB_CS + r * 32 + hf * 16) = r < L ? cq[i] : zero4;
        }
    }
    // per-position scalars (thread t <-> position t); kernel text in both kernels: as a shared function it costs K6b a fourth spill
    float dtv = 0.0f, sg0 = 0.0f;
    int zr0 = f.zr0, orow0 = f.orow0;
    if (tid < L) {
        const float raw = f.rawv + bias;
        dtv = softplus_f(raw);
        sg0 = (raw > 20.0f) ? 1.0f : sigmoid_f(raw);                               // d softplus / d raw (identity above 20)
    } else {
        zr0 = 0;
        orow0 = 0;
    }
    if (tid < SB_TAB) {
        DT[tid] = dtv;
        SIG[tid] = sg0;
        zi[tid] = (uint16_t)zr0;
        oi[tid] = (uint16_t)orow0;
    }
    {
        const float c = block_prefix_sum(dtv, lane, w, red);                       // cumsum(dt)
        if (tid < SB_TAB) {
            CUM[tid] = c;
            S2[tid] = a2 * c;                                                     // log2-domain log-decay
        }
    }
    __syncthreads();
    if (tid < SB_TAB) {
        const int tt = tid >> 5;
        const float sv = S2[tid];
        const float m_t = tt ? S2[SB_TILE * tt - 1] : 0.0f, m_n = S2[SB_TILE * tt + SB_TILE - 1];
        const float al = fast_exp2(sv - m_t), ga = fast_exp2(m_n - sv);
        ALPHA[tid] = al;
        GAM[tid] = ga;
        GDT[tid] = ga * DT[tid];
    }

    // X, gY = dout .* silu(z) into LDS (kernel text, not a shared function: see ssd_bwd_common.h)
    float dD_acc = 0.0f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int ck = w + 4 * m;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = lane + 64 * j;
            if (r < SB_ROWS) {
                u32x4_t xv = {0u, 0u, 0u, 0u}, gv = {0u, 0u, 0u, 0u};
                if (r < L) {
                    const u32x4_t xq = f.xq4[m][j], dq = f.dq4[m][j], zq = f.zq4[m][j];
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        float g0 = O::lo(dq[d]), g1 = O::hi(dq[d]);
                        if (p.z) {
                            g0 *= silu_f(O::lo(zq[d]));
                            g1 *= silu_f(O::hi(zq[d]));
                        }
                        dD_acc += g0 * O::lo(xq[d]) + g1 * O::hi(xq[d]);
                        xv[d] = xq[d];
                        gv[d] = O::pack(g0, g1);
                    }
                }
                const int so = r * 128 + ((ck ^ (r & 7)) << 4);
                *reinterpret_cast<u32x4_t*>(lds + SB_XS + so) = xv;
                *reinterpret_cast<u32x4_t*>(lds + SB_GS + so) = gv;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: the two orientations of the 28 tile pairs ---------------------------------------------------------------------
    const int q = lane & 31, kh = lane >> 5;                                      // fragment role: row/column of a tile, K half
    const int row8 = lane >> 3, c8 = lane & 7;                                    // epilogue role: row of an 8-row slab, 16-byte chunk
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // selectors: a [positions x 64 channels] row-major fragment set times these = the 32-channel half nt in accumulator layout
    // (K-step j of the half: channel 32 nt + q sits in slot q - 16 j - 8 kh); states likewise (16 of them, columns 16-31 empty)
    const u32x4_t selx[2] = {one_hot<T>(q - 8 * kh), one_hot<T>(q - 16 - 8 * kh)};
    const u32x4_t sel16 = one_hot<T>(q < 16 ? q - 8 * kh : -1);
    // role of the wave: waves land on SIMD (w & 3); the T waves carry the heavier epilogue, so odd heads swap the roles and the two
    // workgroups a CU holds put one T and one N wave on every SIMD
    const int wr = (w + 2 * (int)(blockIdx.x & 1)) & 3;

    if (wr < 2) {
        // ===== T orientation: query tile lt; rows of the score tile = keys (registers), columns = queries (lanes) =====
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int lt = (wr == 0) ? (pass == 0 ? 6 : pass == 1 ? 3 : pass == 2 ? 2 : 0) : (pass == 0 ? 5 : pass == 1 ? 4 : pass == 2 ? 1 : -1);
            if (lt < 0 || lt >= nt_l) continue;
            const int ql = SB_TILE * lt + q;
            const u32x4_t cB = bc_frag(lds + SB_CS, ql, kh);
            u32x4_t gB[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) gB[ks] = row_frag(lds + SB_GS, ql, 2 * ks + kh);
            const float s2q = S2[ql], aq = ALPHA[ql], mlt = t.m_of(lt);
            u32x4_t zq4[4], dq4[4];                                             // the epilogue's z / dout pieces, in flight under the products
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int l = SB_TILE * lt + 8 * r4 + row8;
                const int lc = l < L ? l : L - 1;
                zq4[r4] = (u32x4_t){0u, 0u, 0u, 0u};
                dq4[r4] = (u32x4_t){0u, 0u, 0u, 0u};
                if (p.dz) {
                    const auto zq = __builtin_amdgcn_raw_buffer_load_b128(r_z, (int)zi[lc] * sl_z + hb + c8 * 16, 0, 0);
                    const auto dq = __builtin_amdgcn_raw_buffer_load_b128(r_do, (int)oi[lc] * sl_do + hb + c8 * 16, 0, 0);
                    zq4[r4] = (u32x4_t){zq[0], zq[1], zq[2], zq[3]};
                    dq4[r4] = (u32x4_t){dq[0], dq[1], dq[2], dq[3]};
                }
            }
            f32x16 Y0 = zero16, Y1 = zero16, dC = zero16;
            float rs = 0.0f;
#pragma unroll 1
            for (int it = 0; it <= lt; ++it) {
                const int ki = SB_TILE * it + q;
                const u32x4_t bA = bc_frag(lds + SB_BS, ki, kh);
                f32x16 g = O::m32(bA, cB, zero16);                               // G[query][key]: keys 32it + 4kh + 8r4 + r in registers
                u32x4_t xA[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) xA[ks] = row_frag(lds + SB_XS, ki, 2 * ks + kh);
                f32x16 rr = zero16;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) rr = O::m32(xA[ks], gB[ks], rr);   // R = gY . X
                // X and B of the key tile with the keys in the K slots (accumulator order): selector products
                u32x4_t xf0[2], xf1[2], bf[2];
                acc_to_frags<O>(O::m32(xA[1], selx[1], O::m32(xA[0], selx[0], zero16)), xf0);
                acc_to_frags<O>(O::m32(xA[3], selx[1], O::m32(xA[2], selx[0], zero16)), xf1);
                acc_to_frags<O>(O::m32(bA, sel16, zero16), bf);
                const int kb = SB_TILE * it + 4 * kh;
                float md[16];                                                     // M[query][key] * dt_key
                if (it < lt) {
                    const float cq = aq * fast_exp2(mlt - S2[SB_TILE * it + SB_TILE - 1]);
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const f32x4 f = *reinterpret_cast<const f32x4*>(&GDT[kb + 8 * r4]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) md[4 * r4 + r] = cq * f[r];
                    }
                } else {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const f32x4 sk = *reinterpret_cast<const f32x4*>(&S2[kb + 8 * r4]);
                        const f32x4 dk = *reinterpret_cast<const f32x4*>(&DT[kb + 8 * r4]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) md[4 * r4 + r] = (kb + 8 * r4 + r <= ql) ? fast_exp2(s2q - sk[r]) * dk[r] : 0.0f;
                    }
                }
                uint32_t wp[8], dp[8];
#pragma unroll
                for (int r2 = 0; r2 < 8; ++r2) {
                    const float w0 = g[2 * r2] * md[2 * r2], w1 = g[2 * r2 + 1] * md[2 * r2 + 1];
                    rs += w0 * rr[2 * r2] + w1 * rr[2 * r2 + 1];                   // row sum of R .* W
                    wp[r2] = O::pack(w0, w1);
                    dp[r2] = O::pack(rr[2 * r2] * md[2 * r2], rr[2 * r2 + 1] * md[2 * r2 + 1]);
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                    const u32x4_t df = {dp[4 * ks], dp[4 * ks + 1], dp[4 * ks + 2], dp[4 * ks + 3]};
                    Y0 = O::m32(wf, xf0[ks], Y0);
                    Y1 = O::m32(wf, xf1[ks], Y1);
                    dC = O::m32(df, bf[ks], dC);
                }
            }
            rs += __shfl_xor(rs, 32);
            if (kh == 0) RS[ql] = rs;
            if (q < 16) {                                                         // dC[32lt + 4kh + 8r4 + r][state q], partial of this head
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = SB_TILE * lt + 4 * kh + 8 * r4 + r;
                        if (row < L) dbc_part[row * 32 + 16 + q] = dC[4 * r4 + r];
                    }
            }
            // dz = dout .* (Y + D x) .* silu'(z): 8 rows at a time through the staging tile
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    stage[(4 * kh + r) * SB_STG + q] = Y0[4 * r4 + r];
                    stage[(4 * kh + r) * SB_STG + 32 + q] = Y1[4 * r4 + r];
                }
                wave_lds_sync();
                const f32x4 ua = *reinterpret_cast<const f32x4*>(&stage[row8 * SB_STG + 8 * c8]);
                const f32x4 ub = *reinterpret_cast<const f32x4*>(&stage[row8 * SB_STG + 8 * c8 + 4]);
                wave_lds_sync();
                const int l = SB_TILE * lt + 8 * r4 + row8;
                if (p.dz && l < L) {
                    const u32x4_t xq = row_frag(lds + SB_XS, l, c8);
                    const int zr = zi[l];
                    const u32x4_t zq = zq4[r4], dq = dq4[r4];
                    u32x4_t o;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        float res[2];
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const float u = (d < 2 ? ua[2 * d + e] : ub[2 * (d - 2) + e]) + Dh * (e ? O::hi(xq[d]) : O::lo(xq[d]));
                            const float zv = e ? O::hi(zq[d]) : O::lo(zq[d]);
                            const float dv = e ? O::hi(dq[d]) : O::lo(dq[d]);
                            const float sg = sigmoid_f(zv);
                            res[e] = dv * u * sg * (1.0f + zv * (1.0f - sg));
                        }
                        o[d] = O::pack(res[0], res[1]);
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(o, r_dz, zr * sl_dz + hb + c8 * 16, 0, 0);
                }
            }
        }
    } else {
        // ===== N orientation: key tile it; rows of the score tile = queries (registers), columns = keys (lanes) =====
        const int v = wr - 2;
#pragma unroll 1
        for (int pass = 0; pass < 4; ++pass) {
            const int it = (v == 0) ? (pass == 0 ? 0 : pass == 1 ? 3 : pass == 2 ? 4 : 6) : (pass == 0 ? 1 : pass == 1 ? 2 : pass == 2 ? 5 : -1);
            if (it < 0 || it >= nt_l) continue;
            const int ki = SB_TILE * it + q;
            const int kic = ki < SB_TAB ? ki : SB_TAB - 1;
            const u32x4_t bB = bc_frag(lds + SB_BS, ki, kh);
            u32x4_t xB[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) xB[ks] = row_frag(lds + SB_XS, ki, 2 * ks + kh);
            const float dtk = DT[kic], gamk = GAM[kic], s2k = S2[kic], mnext = S2[SB_TILE * it + SB_TILE - 1];
            f32x16 X0 = zero16, X1 = zero16, dB = zero16;
            float cv = 0.0f;
#pragma unroll 1
            for (int lt = it; lt < nt_l; ++lt) {
                const int qrow = SB_TILE * lt + q;
                const u32x4_t cA = bc_frag(lds + SB_CS, qrow, kh);
                f32x16 g = O::m32(cA, bB, zero16);                               // G[query][key]: queries 32lt + 4kh + 8r4 + r in registers
                u32x4_t gA[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) gA[ks] = row_frag(lds + SB_GS, qrow, 2 * ks + kh);
                f32x16 rr = zero16;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) rr = O::m32(gA[ks], xB[ks], rr);
                u32x4_t gf0[2], gf1[2], cf[2];                                   // gY and C of the query tile with the queries in the K slots
                acc_to_frags<O>(O::m32(gA[1], selx[1], O::m32(gA[0], selx[0], zero16)), gf0);
                acc_to_frags<O>(O::m32(gA[3], selx[1], O::m32(gA[2], selx[0], zero16)), gf1);
                acc_to_frags<O>(O::m32(cA, sel16, zero16), cf);
                const int qb = SB_TILE * lt + 4 * kh;
                float mf[16];                                                     // M[query][key] (without dt)
                if (lt > it) {
                    const float ck = gamk * fast_exp2(t.m_of(lt) - mnext);
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(&ALPHA[qb + 8 * r4]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) mf[4 * r4 + r] = ck * a[r];
                    }
                } else {
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const f32x4 sq = *reinterpret_cast<const f32x4*>(&S2[qb + 8 * r4]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) mf[4 * r4 + r] = (ki <= qb + 8 * r4 + r) ? fast_exp2(sq[r] - s2k) : 0.0f;
                    }
                }
                uint32_t wp[8], dp[8];
#pragma unroll
                for (int r2 = 0; r2 < 8; ++r2) {
                    const float gm0 = g[2 * r2] * mf[2 * r2], gm1 = g[2 * r2 + 1] * mf[2 * r2 + 1];
                    cv += gm0 * rr[2 * r2] + gm1 * rr[2 * r2 + 1];                 // column sum of V = R .* G .* M
                    wp[r2] = O::pack(gm0 * dtk, gm1 * dtk);
                    dp[r2] = O::pack(rr[2 * r2] * (mf[2 * r2] * dtk), rr[2 * r2 + 1] * (mf[2 * r2 + 1] * dtk));
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                    const u32x4_t df = {dp[4 * ks], dp[4 * ks + 1], dp[4 * ks + 2], dp[4 * ks + 3]};
                    X0 = O::m32(wf, gf0[ks], X0);
                    X1 = O::m32(wf, gf1[ks], X1);
                    dB = O::m32(df, cf[ks], dB);
                }
            }
            cv += __shfl_xor(cv, 32);
            if (kh == 0) CSV[ki] = cv;
            if (q < 16) {
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = SB_TILE * it + 4 * kh + 8 * r4 + r;
                        if (row < L) dbc_part[row * 32 + q] = dB[4 * r4 + r];
                    }
            }
            // dx = W^T gY + D gY
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    stage[(4 * kh + r) * SB_STG + q] = X0[4 * r4 + r];
                    stage[(4 * kh + r) * SB_STG + 32 + q] = X1[4 * r4 + r];
                }
                wave_lds_sync();
                const f32x4 ua = *reinterpret_cast<const f32x4*>(&stage[row8 * SB_STG + 8 * c8]);
                const f32x4 ub = *reinterpret_cast<const f32x4*>(&stage[row8 * SB_STG + 8 * c8 + 4]);
                wave_lds_sync();
                const int l = SB_TILE * it + 8 * r4 + row8;
                if (l < L) {
                    const u32x4_t gq = row_frag(lds + SB_GS, l, c8);
                    u32x4_t o;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const float u0 = (d < 2 ? ua[2 * d] : ub[2 * (d - 2)]) + Dh * O::lo(gq[d]);
                        const float u1 = (d < 2 ? ua[2 * d + 1] : ub[2 * (d - 2) + 1]) + Dh * O::hi(gq[d]);
                        o[d] = O::pack(u0, u1);
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(o, r_dx, l * sl_dx + hb + c8 * 16, 0, 0);
                }
            }
        }
    }
    __syncthreads();

    sb_phase3(p, t, s, h, tid, lane, w, Ah, dD_acc);
}

template <typename T>
static int ssd_bwd_launch(const dm_ssd_bwd_args& a, hipStream_t st) {
    if (const int rc = reserve_dynamic_lds<&ssd_bwd_kernel<T>>("dm_ssd_bwd", SB_LDS_BYTES)) return rc;
    dim3 grid(a.nheads, a.nseq), block(SB_THREADS);
    hipLaunchKernelGGL((ssd_bwd_kernel<T>), grid, block, SB_LDS_BYTES, st, a);
    return launch_status("dm_ssd_bwd");
}

}  // namespace dm

extern "C" int dm_ssd_bwd_supported(int seqlen, int headdim, int dstate, int io_dtype) {
    return (seqlen >= 1 && seqlen <= dm::SB_MAXL && headdim == 64 && dstate == 16 && (io_dtype == DM_BF16 || io_dtype == DM_F16)) ? 1 : 0;
}

extern "C" int dm_ssd_bwd(const dm_ssd_bwd_args* args, void* stream) {
    using namespace dm;
    if (const int rc = ssd_bwd_check("dm_ssd_bwd", args, dm_ssd_bwd_supported, /*wide*/ false)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return args->io_dtype == DM_BF16 ? ssd_bwd_launch<bf16_t>(*args, st) : ssd_bwd_launch<f16_t>(*args, st);
}
