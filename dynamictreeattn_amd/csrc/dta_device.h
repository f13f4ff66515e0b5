// Shared device-side vocabulary of the kernel files (*.hip only): vector types, the storage-type trait, wave reductions, the transposed
// LDS read and the two LDS-image fragment reads of the MFMA 32x32x16 kernels.  Host-side launch bookkeeping is in dta_common.h.
#ifndef DTA_DEVICE_H
#define DTA_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dta.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
// 8 floats = two 16-byte accesses per lane: aligned(16), so the row kernels may take any 16-byte aligned fp32 pointer.  (The log-prob
// entries ask for 32 bytes; their device code is the same with either alignment.)
typedef float f32x8 __attribute__((ext_vector_type(8), aligned(16)));

// Storage type DT (DTA_BF16 / DTA_F16 / DTA_F32): element e, 8-vector v8; the 16-bit types also have the 4-vector v4 and the MFMA
// 32x32x16 with fp32 accumulation.  With e = float the roundings to the storage type `(e)(...)` are the identity.
template <int DT> struct Ty;
template <> struct Ty<DTA_BF16> {
  using e = __bf16; using v8 = bf16x8; using v4 = bf16x4;
  static __device__ __forceinline__ f32x16 mma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Ty<DTA_F16> {
  using e = _Float16; using v8 = f16x8; using v4 = f16x4;
  static __device__ __forceinline__ f32x16 mma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct Ty<DTA_F32> { using e = float; using v8 = f32x8; };

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// tanh(x) from a = 2 log2(e) x in fp32: 1 - 2 / (1 + 2^a), one v_exp_f32 and one v_rcp_f32.  2^a overflows to +inf for large a and the
// reciprocal of inf is 0, so the value saturates to exactly +1 (and to -1 when 2^a underflows to 0): finite for every finite or infinite a
// - a quotient of two exponentials would be inf / inf there.  Absolute error a few 2^-24 (the cancellation for small |x| is absolute, not
// relative: a capped score softcap * tanh is off by the order of softcap * 2^-24, the fp32 floor of the score itself).
__device__ __forceinline__ float cap_tanh(float a) { return __builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(a)), 1.f); }

__device__ __forceinline__ float wave_max(float v) { for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ float wave_sum(float v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }

// ds_read_b64_tr_b16: the transposed LDS read of four 16-bit elements
__device__ __forceinline__ s16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// MFMA 32x32x16 operand fragment of k-step s for the 32-row/column block ob, from an LDS image of 16-bit elements with pitch ld (elements).
// k-fast image [outer][k]: lane (r = lane & 31, h = lane >> 5) gets operand[ob*32 + r][16s + 8h + j], j = 0..7, by one ds_read_b128
template <class V8> __device__ __forceinline__ V8 frag_kfast(const char* img, int ld, int ob, int s, int lane) {
  return *reinterpret_cast<const V8*>(img + ((ob * 32 + (lane & 31)) * ld + 16 * s + 8 * (lane >> 5)) * 2);
}
// the same fragment from an outer-fast image [k][outer] by two transposed reads: in 16-lane group G (column half c = G & 1, k half h = G >> 1),
// lane 4q + p addresses row k = 16s + 8h + q (+4), columns ob*32 + 16c + 4p .. +3; lane i of the group receives column 16c + i
template <class V8> __device__ __forceinline__ V8 frag_ofast(const char* img, int ld, int ob, int s, int lane) {
  const int G = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int col = ob * 32 + 16 * (G & 1) + 4 * p, kr = 16 * s + 8 * (G >> 1) + q;
  const s16x4 lo = tr_read(img + (kr * ld + col) * 2), hi = tr_read(img + ((kr + 4) * ld + col) * 2);
  const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(V8, both);
}

#endif
