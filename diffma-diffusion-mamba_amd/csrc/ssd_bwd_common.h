// What the two SSD backward kernels (ssd_bwd.hip at d_state 16, ssd_bwd_wide.hip at 32 / 64 / 128) share: the tile geometry, the
// per-position table names, the swizzled X / gY row fragments, the one-hot selector fragments and the workgroup prefix sum.
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

}  // namespace dm
