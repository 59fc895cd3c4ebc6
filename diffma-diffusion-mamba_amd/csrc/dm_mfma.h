// The matrix pipe per 16-bit I/O dtype, shared by every MFMA kernel (gemm, gemm_large, dtproj, conv_xproj, ssd, ssd_bwd): the two
// products these kernels use and the 16-bit pair pack / unpack that goes with their operands and results.
#pragma once
#include "dm_common.h"

namespace dm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Operands are u32x4_t: 8 consecutive 16-bit elements of the contraction, as loaded.
//   m16  D(16x16) = A(16x32) B(32x16) + C   v_mfma_f32_16x16x32_*
//   m32  D(32x32) = A(32x16) B(16x32) + C   v_mfma_f32_32x32x16_*
//   pack(lo, hi)              two fp32 -> one word of two T, lo in bits 0..15
//   unpack(w, lo, hi)         the word's two elements as fp32, from ONE view of the word
//   lo(w), hi(w)              the same, each from its own view of the word
// unpack and lo / hi give the same values; they differ in what the register allocator makes of the f16 case (one bit-cast to a
// half pair and two conversions, against two independent bit-casts), and a kernel keeps the form it was tuned with.
template <typename T> struct mfma;
template <> struct mfma<bf16_t> {
    typedef __bf16 x8 __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ f32x4 m16(const u32x4_t& a, const u32x4_t& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 m32(const u32x4_t& a, const u32x4_t& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    // v_cvt_pk_bf16_f32 through the compiler (dm_cvt_pk_bf16), NEVER inline asm: the kernels convert MFMA results directly, and
    // only an instruction the compiler knows gets the wait states an MFMA result needs before a VALU read (the inline-asm form
    // was seen as 1 % garbage in K6b's selector tiles) and a place in the schedule by its latency (-3 % K3x, -5 % K4x).
    static __device__ __forceinline__ uint32_t pack(float lo, float hi) { return dm_cvt_pk_bf16(lo, hi); }
    static __device__ __forceinline__ float lo(uint32_t w) { return __uint_as_float(w << 16); }
    static __device__ __forceinline__ float hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
    static __device__ __forceinline__ void unpack(uint32_t w, float& l, float& h) { l = lo(w); h = hi(w); }
};
template <> struct mfma<f16_t> {
    typedef _Float16 x8 __attribute__((ext_vector_type(8)));
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ f32x4 m16(const u32x4_t& a, const u32x4_t& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 m32(const u32x4_t& a, const u32x4_t& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ uint32_t pack(float lo, float hi) {
        h2 v;
        v.x = (_Float16)lo;
        v.y = (_Float16)hi;
        return __builtin_bit_cast(uint32_t, v);
    }
    static __device__ __forceinline__ float lo(uint32_t w) { return (float)__builtin_bit_cast(h2, w).x; }
    static __device__ __forceinline__ float hi(uint32_t w) { return (float)__builtin_bit_cast(h2, w).y; }
    static __device__ __forceinline__ void unpack(uint32_t w, float& l, float& h) {
        const h2 v = __builtin_bit_cast(h2, w);
        l = (float)v.x;
        h = (float)v.y;
    }
};

}  // namespace dm
