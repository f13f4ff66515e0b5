// Quantised frozen base of a LoRA model for gfx950 (include/dta.h "Quantised frozen base") - HBM-bound.
//   dta_quant_blockwise     weight [R, C] (bf16 / f16 / f32, row pitch ld_w) -> block codes + one fp32 scale per block; once per weight
//   dta_dequant_blockwise   codes + scales -> the 16-bit (or fp32) operand of a GEMM, row-major at a row pitch (a member of a fused group
//                           writes its row range of ONE stacked operand) or transposed through an LDS tile; every use of every projection
// Formats: "nf4" - blocks of 64, scale = absmax, code = number of code-book midpoints below x / scale, two codes per byte (even element
// in the high nibble); "fp8" - blocks of 128, scale = absmax / 448, OCP e4m3 of x / scale.  value(code) * scale is ONE fp32 product,
// rounded once to the output type: quant.py mirrors every bit on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dta_common.h"
#include "dta_device.h"
#include "dta_quant_tables.h"

namespace {

// value(code) * scale, rounded to fp32, BEFORE the rounding to the output type.  Left to itself the compiler folds the product and a
// rounding to f16 into one v_fma_mixlo_f16 (x * s + 0, rounded once to f16) - whatever the contraction pragmas say: another result where
// the two roundings differ from the one, and +0 where the product is -0, bits the host mirror's two-step expression does not give.  The
// empty statement makes the fp32 product a value of its own.
__device__ __forceinline__ float scaled(float v, float s) {
  float p = v * s;
  asm("" : "+v"(p));
  return p;
}

constexpr float NF4_CODE[16] = {DTA_NF4_CODEBOOK};
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int FMT> struct Fmt;
template <> struct Fmt<DTA_QUANT_NF4> { static constexpr int block = DTA_NF4_BLOCK; static constexpr int bytes8 = 4; };   // bytes of 8 codes
template <> struct Fmt<DTA_QUANT_FP8> { static constexpr int block = DTA_FP8_BLOCK; static constexpr int bytes8 = 8; };

// Codes are read once per use of a weight and never again inside the call: non-temporal, as the saved activations of the row kernels
template <class T> __device__ __forceinline__ T code_load(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const T*>(p)); }

__device__ __forceinline__ void nf4_pair(uint32_t byte, const float* lut, float* v) { v[0] = lut[(byte >> 4) & 15]; v[1] = lut[byte & 15]; }
__device__ __forceinline__ void fp8_pair(uint32_t word, bool hi, float* v) {
  const f32x2 f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)word, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)word, false);
  v[0] = f[0]; v[1] = f[1];
}
// value(code) of the N (4 or 8) consecutive elements whose codes start at p (aligned to their N-code unit); lut: the NF4 code book in LDS
template <int FMT, int N> __device__ __forceinline__ void decode(const uint8_t* p, const float* lut, float* v) {
  if constexpr (FMT == DTA_QUANT_NF4) {
    const uint32_t wd = N == 8 ? code_load<uint32_t>(p) : (uint32_t)code_load<uint16_t>(p);
#pragma unroll
    for (int j = 0; j < N / 2; ++j) nf4_pair(wd >> (8 * j), lut, v + 2 * j);
  } else if constexpr (N == 8) {
    const u32x2 wd = code_load<u32x2>(p);
    fp8_pair(wd[0], false, v); fp8_pair(wd[0], true, v + 2); fp8_pair(wd[1], false, v + 4); fp8_pair(wd[1], true, v + 6);
  } else {
    const uint32_t wd = code_load<uint32_t>(p);
    fp8_pair(wd, false, v); fp8_pair(wd, true, v + 2);
  }
}

template <int FMT> __device__ __forceinline__ void load_codebook(float* lut) {      // fp8 decodes by conversion: no table, no barrier
  if constexpr (FMT == DTA_QUANT_NF4) {
    if (threadIdx.x < 16) lut[threadIdx.x] = NF4_CODE[threadIdx.x];
    __syncthreads();
  }
}

template <int DT> __device__ __forceinline__ uint32_t bits_of(float f) {           // round_to(DT, f) as its bit pattern
  using e = typename Ty<DT>::e;
  const e r = (e)f;
  if constexpr (DT == DTA_F32) return __builtin_bit_cast(uint32_t, r);
  else return (uint32_t)__builtin_bit_cast(uint16_t, r);
}

// ---------------------------------------------------------------------------------------------
// Quantise: one wave per block (64 lanes x 1 or 2 elements), grid-strided.  Not a hot path: element loads, byte / 2-byte stores.
template <int DT, int FMT>
__global__ __launch_bounds__(256) void quant_kernel(const void* __restrict__ w_, int64_t ld_w, int64_t R, int64_t C, uint8_t* __restrict__ q,
                                                    float* __restrict__ scales) {
  using e = typename Ty<DT>::e;
  constexpr int B = Fmt<FMT>::block, PER = B / 64;
  const e* w = reinterpret_cast<const e*>(w_);
  const int lane = threadIdx.x & 63;
  const int64_t nb = C / B, total = R * nb;
  for (int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < total; blk += (int64_t)gridDim.x * 4) {   // wave-uniform
    const int64_t row = blk / nb, b = blk - row * nb;
    const e* src = w + row * ld_w + b * B + lane * PER;
    float x[PER], m = 0.f;
#pragma unroll
    for (int j = 0; j < PER; ++j) { x[j] = (float)src[j]; m = fmaxf(m, fabsf(x[j])); }
    m = wave_max(m);
    if constexpr (FMT == DTA_QUANT_NF4) {
      int code = 7;
      if (m > 0.f) {
        const float v = __fdiv_rn(x[0], m);
        code = 0;
#pragma unroll
        for (int i = 0; i < 15; ++i) code += v > DTA_NF4_MID(NF4_CODE, i) ? 1 : 0;       // a value on a midpoint takes the lower code
      }
      const int next = __shfl_down(code, 1);
      if (!(lane & 1)) q[row * (C / 2) + b * (B / 2) + (lane >> 1)] = (uint8_t)((code << 4) | next);
      if (lane == 0) scales[blk] = m;
    } else {
      const float s = __fdiv_rn(m, DTA_FP8_MAX);
      uint16_t pk = 0;
      if (s > 0.f) {
        const float a = fminf(fmaxf(__fdiv_rn(x[0], s), -DTA_FP8_MAX), DTA_FP8_MAX), c = fminf(fmaxf(__fdiv_rn(x[1], s), -DTA_FP8_MAX), DTA_FP8_MAX);
        pk = (uint16_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, c, 0, false);                  // element 2l in the low byte
      }
      reinterpret_cast<uint16_t*>(q + row * C + b * B)[lane] = pk;
      if (lane == 0) scales[blk] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Dequantise, row-major.  A lane owns 8 consecutive elements of a row (inside one block: 8 divides both block sizes): one 4- or 8-byte
// code load, its block's scale, one 16-byte store (two for fp32).  A wave covers 512 consecutive elements of one row, the four waves of a
// workgroup four rows, and every lane has U rows' loads in flight before the first decode.
template <int DT, int FMT>
__global__ __launch_bounds__(256) void dequant_rows_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scales, int64_t R, int64_t C,
                                                           void* __restrict__ out_, int64_t ld_out) {
  using e = typename Ty<DT>::e; using V8 = typename Ty<DT>::v8;
  constexpr int U = 4, GB = Fmt<FMT>::bytes8, B = Fmt<FMT>::block;
  __shared__ float lut[16];
  load_codebook<FMT>(lut);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * 64 + lane;
  if (g * 8 >= C) return;
  const int64_t row_bytes = C / 8 * GB, nb = C / B, blk = g * 8 / B;
  e* out = reinterpret_cast<e*>(out_);
  for (int64_t rb = (int64_t)blockIdx.y * (4 * U); rb < R; rb += (int64_t)gridDim.y * (4 * U)) {
    float v[U][8], s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = rb + u * 4 + wave;
      if (row < R) { decode<FMT, 8>(q + row * row_bytes + g * GB, lut, v[u]); s[u] = scales[row * nb + blk]; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = rb + u * 4 + wave;
      if (row < R) {
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (e)scaled(v[u][j], s[u]);
        *reinterpret_cast<V8*>(out + row * ld_out + g * 8) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Dequantise, transposed: out[c][r] = value(code[r][c]) * scale.  The LDS tile of transpose_kernel (elementwise_kernels.hip) - 64 x 64
// elements as 32-bit words at an odd-ish pitch, 16-bit elements packed as (row 2p, row 2p + 1) pairs so that the write phase reads 8
// output elements with one ds_read_b128 - with the decode on the load side.  A tile lies inside one block of every row it covers (64
// divides both block sizes).  `vec`: the output rows start on 16 bytes (ld_out a multiple of 16 bytes); otherwise, and at the ragged edge
// of R, element stores.
template <int DT, int FMT>
__global__ __launch_bounds__(256) void dequant_transposed_kernel(const uint8_t* __restrict__ q, const float* __restrict__ scales, int64_t R, int64_t C,
                                                                 void* __restrict__ out_, int64_t ld_out, int vec) {
  constexpr int ESZ = DT == DTA_F32 ? 4 : 2, TS = 64, WPR = ESZ == 2 ? TS / 2 : TS, PITCH = WPR + 4;
  constexpr int GB = Fmt<FMT>::bytes8, B = Fmt<FMT>::block;
  __shared__ __attribute__((aligned(16))) uint32_t tile[TS * PITCH];
  __shared__ float lut[16];
  load_codebook<FMT>(lut);
  const int64_t r0 = (int64_t)blockIdx.x * TS, c0 = (int64_t)blockIdx.y * TS;
  const int64_t row_bytes = C / 8 * GB, nb = C / B;
  const int tid = threadIdx.x;
  char* out = reinterpret_cast<char*>(out_);
  if constexpr (ESZ == 2) {
    // load: 32 row pairs x 8 groups of 8 columns = 256 items, one per thread
    const int rp = tid >> 3, c = 8 * (tid & 7);
    uint32_t word[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) word[j] = 0;
    if (c0 + c < C) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t row = r0 + 2 * rp + h;
        if (row < R) {
          float v[8];
          decode<FMT, 8>(q + row * row_bytes + (c0 + c) / 8 * GB, lut, v);
          const float s = scales[row * nb + (c0 + c) / B];
#pragma unroll
          for (int j = 0; j < 8; ++j) word[j] |= bits_of<DT>(scaled(v[j], s)) << (16 * h);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[(c + j) * PITCH + rp] = word[j];
    __syncthreads();
    // store: 64 output rows (input columns) x 8 chunks of 8 output elements (4 words)
    for (int i = tid; i < TS * 8; i += 256) {
      const int oc = i >> 3, k = i & 7;
      if (c0 + oc >= C || r0 + 8 * k >= R) continue;
      const uint32_t* src = &tile[oc * PITCH + 4 * k];
      char* dst = out + ((c0 + oc) * ld_out + r0 + 8 * k) * 2;
      if (vec && r0 + 8 * k + 8 <= R) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
      else
        for (int j = 0; j < 8 && r0 + 8 * k + j < R; ++j) reinterpret_cast<uint16_t*>(dst)[j] = (uint16_t)(src[j >> 1] >> (16 * (j & 1)));
    }
  } else {
    for (int i = tid; i < TS * 16; i += 256) {          // 64 rows x 16 groups of 4 columns
      const int r = i >> 4, c = 4 * (i & 15);
      const int64_t row = r0 + r;
      float v[4] = {0.f, 0.f, 0.f, 0.f}, s = 0.f;
      if (row < R && c0 + c < C) {
        decode<FMT, 4>(q + row * row_bytes + (c0 + c) * GB / 8, lut, v);
        s = scales[row * nb + (c0 + c) / B];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(c + j) * PITCH + r] = __builtin_bit_cast(uint32_t, scaled(v[j], s));
    }
    __syncthreads();
    for (int i = tid; i < TS * 16; i += 256) {
      const int oc = i >> 4, k = i & 15;
      if (c0 + oc >= C || r0 + 4 * k >= R) continue;
      const uint32_t* src = &tile[oc * PITCH + 4 * k];
      char* dst = out + ((c0 + oc) * ld_out + r0 + 4 * k) * 4;
      if (vec && r0 + 4 * k + 4 <= R) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
      else
        for (int j = 0; j < 4 && r0 + 4 * k + j < R; ++j) reinterpret_cast<uint32_t*>(dst)[j] = src[j];
    }
  }
}

inline bool fmt_ok(int fmt) { return fmt == DTA_QUANT_NF4 || fmt == DTA_QUANT_FP8; }
inline int block_of(int fmt) { return fmt == DTA_QUANT_NF4 ? DTA_NF4_BLOCK : DTA_FP8_BLOCK; }
template <class F> inline void quant_format(int32_t fmt, F&& f) {
  if (fmt == DTA_QUANT_NF4) f(std::integral_constant<int, DTA_QUANT_NF4>{});
  else f(std::integral_constant<int, DTA_QUANT_FP8>{});
}
constexpr int64_t MAX_COLS = (int64_t)1 << 22;      // 65 535 column tiles of the transposed form

}  // namespace

extern "C" int dta_quant_blockwise(const void* w, int64_t ld_w, int64_t R, int64_t C, int32_t w_dtype, int32_t fmt, void* q, float* scales,
                                   void* stream) {
  if (!w || !q || !scales || R <= 0 || C <= 0 || ld_w < C) return DTA_EINVAL;
  if (!fmt_ok(fmt) || !row_dtype_ok(w_dtype) || C % block_of(fmt) || C >= MAX_COLS) return DTA_EUNSUPPORTED;
  if (!all_aligned16(q, scales) || (reinterpret_cast<uintptr_t>(w) & (w_dtype == DTA_F32 ? 3 : 1))) return DTA_EALIGN;
  const int64_t blocks = R * (C / block_of(fmt));
  return dta_launch(stream, [&](hipStream_t st) {
    dta_storage_type(w_dtype, [&](auto dt) {
      quant_format(fmt, [&](auto f) {
        hipLaunchKernelGGL((quant_kernel<decltype(dt)::value, decltype(f)::value>), dim3(row_blocks(blocks, 4, 8192)), dim3(256), 0, st, w, ld_w, R, C,
                           (uint8_t*)q, scales);
      });
    });
  });
}

extern "C" int dta_dequant_blockwise(const void* q, const float* scales, int64_t R, int64_t C, int32_t fmt, void* out, int64_t ld_out,
                                     int32_t out_dtype, int32_t transposed, void* stream) {
  if (!q || !scales || !out || R <= 0 || C <= 0 || (transposed != 0 && transposed != 1) || ld_out < (transposed ? R : C)) return DTA_EINVAL;
  if (!fmt_ok(fmt) || !row_dtype_ok(out_dtype) || C % block_of(fmt) || C >= MAX_COLS) return DTA_EUNSUPPORTED;
  const int V = out_dtype == DTA_F32 ? 4 : 8;         // elements of 16 bytes
  if (!all_aligned16(q, scales, out) || (!transposed && ld_out % V)) return DTA_EALIGN;
  return dta_launch(stream, [&](hipStream_t st) {
    dta_storage_type(out_dtype, [&](auto dt) {
      quant_format(fmt, [&](auto f) {
        constexpr int DT = decltype(dt)::value, FMT = decltype(f)::value;
        if (transposed)
          hipLaunchKernelGGL((dequant_transposed_kernel<DT, FMT>), dim3(ceil_blocks(R, 64), (unsigned)(C / 64)), dim3(256), 0, st, (const uint8_t*)q,
                             scales, R, C, out, ld_out, ld_out % V == 0 ? 1 : 0);
        else
          hipLaunchKernelGGL((dequant_rows_kernel<DT, FMT>), dim3(ceil_blocks(C / 8, 64), row_blocks(R, 16, 65535)), dim3(256), 0, st, (const uint8_t*)q,
                             scales, R, C, out, ld_out);
      });
    });
  });
}
