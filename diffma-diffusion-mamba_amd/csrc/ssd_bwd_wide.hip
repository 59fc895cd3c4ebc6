// K6c  dm_ssd_bwd_wide -- backward of the Mamba-2 single-chunk SSD core on the matrix pipe at d_state 32 / 64 / 128.
//
// Same operator, same gradients and the same roundings as ssd_bwd.hip (its header, lines 3-10): the stored gY, the W tile and the
// dG tile are rounded to the I/O dtype, dz and dx on the way out, everything else stays fp32.  Only the contractions over the
// state run over N = 16 NK instead of 16: the score tile G = C B^T takes NK MFMAs, and dB / dC are NK / 2 accumulator tiles of
// 32 positions x 32 states each.  Nothing is saved by the forward.
//
// Frame.  One 256-thread workgroup per (sequence, group of DM_SSD_BWD_WIDE_HEADS heads) walks its heads one after the other;
// per head it is the d_state 16 kernel: X and gY row-major in LDS (50 KB), waves 0-1 in the T orientation (Y -> dz, dC), waves
// 2-3 in the N orientation (dX, dB), the 28 causal tile pairs each, selector MFMAs to bring positions into the K slots.
// Where B and C live is what differs.  X + gY + raw B + C rows of d_state 128 do not fit in the 160 KB of a CU together with
// the tables, so B and C are NOT staged: each orientation keeps the B / C fragments of its own tile in registers (NK u32x4) for
// the whole pass and reads the fragments of the streamed tile straight from global memory (L2: a sequence's B and C are 2 x 50 KB
// at most and every workgroup of the sequence reads them), 16 bytes per lane, requested one tile pair ahead.  LDS is then 67 KB at
// every width.  One wave per SIMD (512 registers per lane): d_state 128 needs far more than 256 (64 for the dB / dC tiles alone,
// 96 for the resident, the current and the next B / C fragments), and at 256 the 32 and 64 instantiations spilled.
//
// dB / dC partial rows.  A wave owns the same tiles for every head of the group, so the lane that wrote an element of the
// partial rows for the group's first head is the lane that adds the later heads to it: a plain fp32 read-add-write by one
// thread in head order, no atomics, bit-reproducible.  The caller sums the [ceil(H / HEADS)][S][L][2N] rows over the groups.
#include "ssd_bwd_common.h"

namespace dm {

constexpr int SBW_HEADS = DM_SSD_BWD_WIDE_HEADS;

// LDS map (byte offsets); rows [L, 196] of the operand arrays are zero
constexpr int SBW_XS = 0;                          // X   [197][64]  16-byte chunks XOR-swizzled by (row & 7)
constexpr int SBW_GS = SBW_XS + SB_ROWS * 128;     // gY  [197][64]  same layout
constexpr int SBW_TAIL = SBW_GS + SB_ROWS * 128;   // tables, staging tiles, scratch (ssd_bwd_common.h)
constexpr int SBW_LDS_BYTES = SBW_TAIL + SB_T_BYTES;
static_assert(SBW_LDS_BYTES <= 160 * 1024, "LDS of a CU");
static_assert(SBW_TAIL % 16 == 0, "16-byte aligned LDS arrays");

// NK fragments (8 states each at 16 j + 8 kh) of a B / C row, straight from global memory.  A row past L is never read: the lane
// asks for row L - 1 instead and zeroes what comes back.
template <int NK>
__device__ __forceinline__ void bc_row_load(u32x4_t (&f)[NK], const rsrc_t& r, int row, int L, int sl, int kh) {
    const int rc = row < L ? row : L - 1;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, rc * sl + 32 * j + 16 * kh, 0, 0);
        f[j] = (u32x4_t){v[0], v[1], v[2], v[3]};
    }
}
template <int NK>
__device__ __forceinline__ void bc_row_mask(u32x4_t (&f)[NK], bool live) {
#pragma unroll
    for (int j = 0; j < NK; ++j)
#pragma unroll
        for (int d = 0; d < 4; ++d) f[j][d] = live ? f[j][d] : 0u;
}

template <typename T, int NK>
__global__ __launch_bounds__(SB_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void ssd_bwd_wide_kernel(const dm_ssd_bwd_args p) {
    using O = mfma<T>;
    constexpr int ES = (int)sizeof(T);
    constexpr int N = 16 * NK, NC = NK / 2;                                       // states; 32-state accumulator tiles of dB / dC
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const sb_tables t(lds + SBW_TAIL, w);
    const auto [DT, CUM, S2, ALPHA, GAM, GDT, SIG, RS, CSV, zi, oi, stage, red] = t;
    const int s = blockIdx.y;
    const int L = p.seqlen, H = p.nheads;
    const int bpd = (p.batch_per_dir > 0) ? p.batch_per_dir : p.nseq;
    const int dir = s / bpd;
    const int sb = s - dir * bpd;
    const int nt_l = (L + SB_TILE - 1) / SB_TILE;
    const int32_t* __restrict__ zidx = p.z_row_index ? p.z_row_index + (int64_t)dir * L : nullptr;
    const int32_t* __restrict__ oidx = p.out_row_index ? p.out_row_index + (int64_t)dir * L : nullptr;
    const rsrc_t r_x = make_rsrc((const T*)p.x + (int64_t)s * p.x_ss);
    const rsrc_t r_B = make_rsrc((const T*)p.B + (int64_t)s * p.B_ss);
    const rsrc_t r_C = make_rsrc((const T*)p.C + (int64_t)s * p.C_ss);
    const rsrc_t r_z = make_rsrc(p.z ? (const T*)p.z + (int64_t)sb * p.z_ss : nullptr);
    const rsrc_t r_do = make_rsrc((const T*)p.dout + (int64_t)s * p.do_ss);
    const rsrc_t r_dx = make_rsrc((T*)p.dx + (int64_t)s * p.dx_ss);
    const rsrc_t r_dz = make_rsrc(p.dz ? (T*)p.dz + (int64_t)s * p.dz_ss : nullptr);
    const int sl_B = (int)p.B_sl * ES, sl_C = (int)p.C_sl * ES, sl_z = (int)p.z_sl * ES;
    const int sl_do = (int)p.do_sl * ES, sl_dx = (int)p.dx_sl * ES, sl_dz = (int)p.dz_sl * ES;
    // the gate is a view of the in_proj output: its rows start on 16-byte boundaries with the factory models' 16 or 24 heads, on
    // 4-byte boundaries with the two heads of a d_model 64 mixer (then the same 16 bytes are read as dwords)
    const bool z_rows16 = (((uintptr_t)p.z & 15) | (uintptr_t)(p.z_ss & 7) | (uintptr_t)(p.z_sl & 7)) == 0;
    auto z_piece = [&](int byte_off) -> u32x4_t {
        u32x4_t o;
        if (z_rows16) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_z, byte_off, 0, 0);
            o = (u32x4_t){v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) o[d] = __builtin_amdgcn_raw_buffer_load_b32(r_z, byte_off + 4 * d, 0, 0);
        }
        return o;
    };
    // partial rows of the group: dB (0 .. N-1) | dC (N .. 2N-1) per position
    float* const dbc_part = p.dBC_part + ((int64_t)blockIdx.x * p.nseq + s) * L * (2 * N);

    const int q = lane & 31, kh = lane >> 5;                                      // fragment role: row/column of a tile, K half
    const int row8 = lane >> 3, c8 = lane & 7;                                    // epilogue role: row of an 8-row slab, 16-byte chunk
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // selectors: a [positions x 32 channels / states] row-major fragment pair times these = those 32 columns in accumulator layout
    // (K-step j of the pair: column q sits in slot q - 16 j - 8 kh)
    const u32x4_t selx[2] = {one_hot<T>(q - 8 * kh), one_hot<T>(q - 16 - 8 * kh)};

#pragma unroll 1
    for (int hh = 0; hh < SBW_HEADS; ++hh) {
        const int h = blockIdx.x * SBW_HEADS + hh;
        if (h >= H) break;                                                        // workgroup-uniform: a head past nheads leaves nothing behind
        const bool first = hh == 0;
        const float Ah = p.A[h], a2 = Ah * LOG2E, Dh = p.D ? p.D[h] : 0.0f, bias = p.dt_bias ? p.dt_bias[h] : 0.0f;
        const T* __restrict__ dtp = (const T*)p.dt + (int64_t)sb * p.dt_sb + h;
        const int hb = h * 64 * ES;                                               // byte offset of the head's columns in a row

        // ---- phases 0 + 1: the load front (ssd_bwd_common.h) ----
        sb_front f;
        sb_front_issue(f, p, r_x, r_do, zidx, oidx, dtp, hb, tid, lane, w, z_piece);
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
                    *reinterpret_cast<u32x4_t*>(lds + SBW_XS + so) = xv;
                    *reinterpret_cast<u32x4_t*>(lds + SBW_GS + so) = gv;
                }
            }
        }
        __syncthreads();

        // ---- phase 2: the two orientations of the 28 tile pairs.  The role of a wave is the same for every head of the group:
        // the lane that owns an element of the partial rows owns it for all of them.  Waves land on SIMD (w & 3) and the T waves
        // carry the heavier epilogue, so every other workgroup swaps the roles. ----
        const int wr = (w + 2 * (int)((blockIdx.x + blockIdx.y) & 1)) & 3;
        if (wr < 2) {
            // ===== T orientation: query tile lt; rows of the score tile = keys (registers), columns = queries (lanes) =====
#pragma unroll 1
            for (int pass = 0; pass < 4; ++pass) {
                const int lt = (wr == 0) ? (pass == 0 ? 6 : pass == 1 ? 3 : pass == 2 ? 2 : 0) : (pass == 0 ? 5 : pass == 1 ? 4 : pass == 2 ? 1 : -1);
                if (lt < 0 || lt >= nt_l) continue;
                const int ql = SB_TILE * lt + q;
                u32x4_t cB[NK], bN[NK];
                bc_row_load<NK>(cB, r_C, ql, L, sl_C, kh);
                bc_row_load<NK>(bN, r_B, q, L, sl_B, kh);                          // key tile 0
                bc_row_mask<NK>(cB, ql < L);
                u32x4_t gB[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) gB[ks] = row_frag(lds + SBW_GS, ql, 2 * ks + kh);
                const float s2q = S2[ql], aq = ALPHA[ql], mlt = t.m_of(lt);
                f32x16 Y0 = zero16, Y1 = zero16, dC[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) dC[c] = zero16;
                float rs = 0.0f;
#pragma unroll 1
                for (int it = 0; it <= lt; ++it) {
                    const int ki = SB_TILE * it + q;
                    u32x4_t bA[NK];
#pragma unroll
                    for (int j = 0; j < NK; ++j) bA[j] = bN[j];
                    bc_row_mask<NK>(bA, ki < L);
                    if (it < lt) bc_row_load<NK>(bN, r_B, ki + SB_TILE, L, sl_B, kh);   // the next key tile, under this pair's products
                    f32x16 g = zero16;                                             // G[query][key]: keys 32it + 4kh + 8r4 + r in registers
#pragma unroll
                    for (int j = 0; j < NK; ++j) g = O::m32(bA[j], cB[j], g);
                    u32x4_t xA[4];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) xA[ks] = row_frag(lds + SBW_XS, ki, 2 * ks + kh);
                    f32x16 rr = zero16;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) rr = O::m32(xA[ks], gB[ks], rr);   // R = gY . X
                    // X of the key tile with the keys in the K slots (accumulator order): selector products
                    u32x4_t xf0[2], xf1[2];
                    acc_to_frags<O>(O::m32(xA[1], selx[1], O::m32(xA[0], selx[0], zero16)), xf0);
                    acc_to_frags<O>(O::m32(xA[3], selx[1], O::m32(xA[2], selx[0], zero16)), xf1);
                    const int kb = SB_TILE * it + 4 * kh;
                    float md[16];                                                 // M[query][key] * dt_key
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
                        rs += w0 * rr[2 * r2] + w1 * rr[2 * r2 + 1];               // row sum of R .* W
                        wp[r2] = O::pack(w0, w1);
                        dp[r2] = O::pack(rr[2 * r2] * md[2 * r2], rr[2 * r2 + 1] * md[2 * r2 + 1]);
                    }
                    u32x4_t df[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                        df[ks] = (u32x4_t){dp[4 * ks], dp[4 * ks + 1], dp[4 * ks + 2], dp[4 * ks + 3]};
                        Y0 = O::m32(wf, xf0[ks], Y0);
                        Y1 = O::m32(wf, xf1[ks], Y1);
                    }
                    // dC += dG B, 32 states at a time: B of the key tile with the keys in the K slots, as X above
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        u32x4_t bf[2];
                        acc_to_frags<O>(O::m32(bA[2 * c + 1], selx[1], O::m32(bA[2 * c], selx[0], zero16)), bf);
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) dC[c] = O::m32(df[ks], bf[ks], dC[c]);
                    }
                }
                rs += __shfl_xor(rs, 32);
                if (kh == 0) RS[ql] = rs;
                // dC[32lt + 4kh + 8r4 + r][state 32c + q]: the first head of the group writes, the later ones add
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = SB_TILE * lt + 4 * kh + 8 * r4 + r;
                            if (row < L) {
                                float* const dst = dbc_part + row * (2 * N) + N + 32 * c + q;
                                *dst = first ? dC[c][4 * r4 + r] : *dst + dC[c][4 * r4 + r];
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
                        const u32x4_t xq = row_frag(lds + SBW_XS, l, c8);
                        const int zr = zi[l];
                        const u32x4_t zq = z_piece(zr * sl_z + hb + c8 * 16);
                        const auto dqv = __builtin_amdgcn_raw_buffer_load_b128(r_do, (int)oi[l] * sl_do + hb + c8 * 16, 0, 0);
                        const u32x4_t dq = {dqv[0], dqv[1], dqv[2], dqv[3]};
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
                u32x4_t bB[NK], cN[NK];
                bc_row_load<NK>(bB, r_B, ki, L, sl_B, kh);
                bc_row_load<NK>(cN, r_C, ki, L, sl_C, kh);                         // query tile it (the diagonal pair comes first)
                bc_row_mask<NK>(bB, ki < L);
                u32x4_t xB[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) xB[ks] = row_frag(lds + SBW_XS, ki, 2 * ks + kh);
                const float dtk = DT[kic], gamk = GAM[kic], s2k = S2[kic], mnext = S2[SB_TILE * it + SB_TILE - 1];
                f32x16 X0 = zero16, X1 = zero16, dB[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) dB[c] = zero16;
                float cv = 0.0f;
#pragma unroll 1
                for (int lt = it; lt < nt_l; ++lt) {
                    const int qrow = SB_TILE * lt + q;
                    u32x4_t cA[NK];
#pragma unroll
                    for (int j = 0; j < NK; ++j) cA[j] = cN[j];
                    bc_row_mask<NK>(cA, qrow < L);
                    if (lt + 1 < nt_l) bc_row_load<NK>(cN, r_C, qrow + SB_TILE, L, sl_C, kh);   // the next query tile
                    f32x16 g = zero16;                                             // G[query][key]: queries 32lt + 4kh + 8r4 + r in registers
#pragma unroll
                    for (int j = 0; j < NK; ++j) g = O::m32(cA[j], bB[j], g);
                    u32x4_t gA[4];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) gA[ks] = row_frag(lds + SBW_GS, qrow, 2 * ks + kh);
                    f32x16 rr = zero16;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) rr = O::m32(gA[ks], xB[ks], rr);
                    u32x4_t gf0[2], gf1[2];                                        // gY of the query tile with the queries in the K slots
                    acc_to_frags<O>(O::m32(gA[1], selx[1], O::m32(gA[0], selx[0], zero16)), gf0);
                    acc_to_frags<O>(O::m32(gA[3], selx[1], O::m32(gA[2], selx[0], zero16)), gf1);
                    const int qb = SB_TILE * lt + 4 * kh;
                    float mf[16];                                                 // M[query][key] (without dt)
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
                        cv += gm0 * rr[2 * r2] + gm1 * rr[2 * r2 + 1];             // column sum of V = R .* G .* M
                        wp[r2] = O::pack(gm0 * dtk, gm1 * dtk);
                        dp[r2] = O::pack(rr[2 * r2] * (mf[2 * r2] * dtk), rr[2 * r2 + 1] * (mf[2 * r2 + 1] * dtk));
                    }
                    u32x4_t df[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        const u32x4_t wf = {wp[4 * ks], wp[4 * ks + 1], wp[4 * ks + 2], wp[4 * ks + 3]};
                        df[ks] = (u32x4_t){dp[4 * ks], dp[4 * ks + 1], dp[4 * ks + 2], dp[4 * ks + 3]};
                        X0 = O::m32(wf, gf0[ks], X0);
                        X1 = O::m32(wf, gf1[ks], X1);
                    }
                    // dB += dG^T C, 32 states at a time: C of the query tile with the queries in the K slots
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        u32x4_t cf[2];
                        acc_to_frags<O>(O::m32(cA[2 * c + 1], selx[1], O::m32(cA[2 * c], selx[0], zero16)), cf);
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) dB[c] = O::m32(df[ks], cf[ks], dB[c]);
                    }
                }
                cv += __shfl_xor(cv, 32);
                if (kh == 0) CSV[ki] = cv;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = SB_TILE * it + 4 * kh + 8 * r4 + r;
                            if (row < L) {
                                float* const dst = dbc_part + row * (2 * N) + 32 * c + q;
                                *dst = first ? dB[c][4 * r4 + r] : *dst + dB[c][4 * r4 + r];
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
                        const u32x4_t gq = row_frag(lds + SBW_GS, l, c8);
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
        __syncthreads();                                                          // the next head reuses the tables and the scratch
    }
}

template <typename T, int NK>
static int ssd_bwd_wide_launch(const dm_ssd_bwd_args& a, hipStream_t st) {
    if (const int rc = reserve_dynamic_lds<&ssd_bwd_wide_kernel<T, NK>>("dm_ssd_bwd_wide", SBW_LDS_BYTES)) return rc;
    dim3 grid((a.nheads + SBW_HEADS - 1) / SBW_HEADS, a.nseq), block(SB_THREADS);
    hipLaunchKernelGGL((ssd_bwd_wide_kernel<T, NK>), grid, block, SBW_LDS_BYTES, st, a);
    return launch_status("dm_ssd_bwd_wide");
}

template <typename T>
static int ssd_bwd_wide_dispatch(const dm_ssd_bwd_args& a, hipStream_t st) {
    switch (a.dstate) {
        case 32: return ssd_bwd_wide_launch<T, 2>(a, st);
        case 64: return ssd_bwd_wide_launch<T, 4>(a, st);
        default: return ssd_bwd_wide_launch<T, 8>(a, st);
    }
}

}  // namespace dm

extern "C" int dm_ssd_bwd_wide_supported(int seqlen, int headdim, int dstate, int io_dtype) {
    const bool width = dstate == 32 || dstate == 64 || dstate == 128;
    return (seqlen >= 1 && seqlen <= dm::SB_MAXL && headdim == 64 && width && (io_dtype == DM_BF16 || io_dtype == DM_F16)) ? 1 : 0;
}

extern "C" int dm_ssd_bwd_wide(const dm_ssd_bwd_args* args, void* stream) {
    using namespace dm;
    if (const int rc = ssd_bwd_check("dm_ssd_bwd_wide", args, dm_ssd_bwd_wide_supported, /*wide*/ true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return args->io_dtype == DM_BF16 ? ssd_bwd_wide_dispatch<bf16_t>(*args, st) : ssd_bwd_wide_dispatch<f16_t>(*args, st);
}
