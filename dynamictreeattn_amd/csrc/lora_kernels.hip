// Low-rank adapter (LoRA) kernels for gfx950 (MI355X, CDNA4): products a projection y = base(x) + s (x A^T) B^T adds to the base GEMM,
// in the forward and the backward.  Each has one long operand [T, K] (T = packed rows) and one of rank R <= 256, so each is a single pass
// over HBM with almost no arithmetic per byte - for the weight gradient the shape a general GEMM library serves worst (one or two output
// tiles for 256 CUs).  The C ABI is in include/dta.h; ops.py chooses kernel or GEMM expression per shape from the measurement in
// profiles/lora_probe.json (the third product, y += s xa B^T in place, lost to addmm_ at every shape and is not here: DESIGN 4f, scripts/diag/lora_up_add_experiment.hip).
//
//   dta_lora_down    out[T, R]  = (X[T, K] . M[R, K]^T) * rscale[r]          one read of X
//   dta_lora_wgrad   part[s][R, K] = rscale[r] * sum_{t in slab s} L[t, R]^T X[t, K]   one read of X and L; fp32 slabs for dta_sum_slabs
//
// MFMA 32x32x16 (bf16 / f16), fp32 accumulation; scales multiply the fp32 accumulator.  Staging global -> registers -> LDS as in
// moe_kernels.hip: an operand whose contraction index is contiguous is read back by rows (ds_read_b128), one whose contraction index is
// the slow axis (both operands of the weight gradient: the contraction runs over the rows) by ds_read_b64_tr_b16.  The rank is padded with
// zeros IN STAGING (to 32 as an output extent, to 16 as a contraction length), never in HBM: a rank-6 operand is [T, 6] in memory, its rows
// are 12 bytes, and the staging loads fall back from 16-byte vectors to element loads when a row pitch or pointer is not 16-byte aligned.
// Rows beyond T, columns beyond K / N / R read as zero and are never written.
//
// Determinism: no atomics.  The weight gradient cuts T into slabs of whole 64-row steps; every slab is summed by one workgroup in row
// order and the slabs are added in slab order by dta_sum_slabs: the same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dta_common.h"
#include "dta_device.h"

namespace {

constexpr int MAXR = 256;
constexpr int BM = 128, BK = 64;
constexpr int KF_LD = BK + 8;            // k-fast image [rows][BK]: 144-byte rows
constexpr int XF_LD = 128 + 8;           // outer-fast image [BK][128]: 272-byte rows

struct RScale { float s[MAXR]; };         // per rank index, passed by value (kernel argument memory)

// elements c .. c+7 of row `row` (16-bit elements, pitch ld), zero from column clim on; c is a multiple of 8
__device__ __forceinline__ uint4 ld8(const uint16_t* base, int64_t row, int64_t ld, int c, int clim, bool vec) {
  uint4 r = {0, 0, 0, 0};
  if (c >= clim) return r;
  const uint16_t* p = base + row * ld + c;
  if (vec && c + 8 <= clim) return *reinterpret_cast<const uint4*>(p);
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = c + j < clim ? (uint32_t)p[j] : 0u;
  r.x = e[0] | (e[1] << 16); r.y = e[2] | (e[3] << 16); r.z = e[4] | (e[5] << 16); r.w = e[6] | (e[7] << 16);
  return r;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// down: out[T, R] = X[T, K] . M[R, K]^T.  A workgroup owns 128 rows; wave w rows 32w .. 32w+31 and all NCB = ceil(R / 32) column blocks.
// ------------------------------------------------------------------------------------------------------------------------------------
struct DownArgs {
  const uint16_t *x, *m; void* out;
  int64_t ldx, ldm, ldo;
  int T, R, K, vx, vm, has_scale;
  RScale rs;
};

template <int DT, int NCB>
__global__ __launch_bounds__(256) void down_k(DownArgs a) {
  using V8 = typename Ty<DT>::v8;
  __shared__ __attribute__((aligned(16))) char lds_x[BM * KF_LD * 2];
  __shared__ __attribute__((aligned(16))) char lds_m[NCB * 32 * KF_LD * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * BM;
  f32x16 acc[NCB];
#pragma unroll
  for (int j = 0; j < NCB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  uint4 sx[4], sm[NCB];
  auto load = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = tid + 256 * i, o = v >> 3, kc = (v & 7) * 8;
      sx[i] = m0 + o < a.T ? ld8(a.x, m0 + o, a.ldx, kb + kc, a.K, a.vx) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < NCB; ++i) {
      const int v = tid + 256 * i, o = v >> 3, kc = (v & 7) * 8;
      sm[i] = o < a.R ? ld8(a.m, o, a.ldm, kb + kc, a.K, a.vm) : uint4{0, 0, 0, 0};
    }
  };
  load(0);
  for (int kb = 0; kb < a.K; kb += BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int v = tid + 256 * i; *reinterpret_cast<uint4*>(lds_x + ((v >> 3) * KF_LD + (v & 7) * 8) * 2) = sx[i]; }
#pragma unroll
    for (int i = 0; i < NCB; ++i) { const int v = tid + 256 * i; *reinterpret_cast<uint4*>(lds_m + ((v >> 3) * KF_LD + (v & 7) * 8) * 2) = sm[i]; }
    __syncthreads();
    if (kb + BK < a.K) load(kb + BK);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      if (kb + 16 * s >= a.K) break;                         // uniform: K is a multiple of 16
      const V8 fa = frag_kfast<V8>(lds_x, KF_LD, wave, s, lane);
#pragma unroll
      for (int j = 0; j < NCB; ++j) acc[j] = Ty<DT>::mma(fa, frag_kfast<V8>(lds_m, KF_LD, j, s, lane), acc[j]);
    }
  }
  // C block j: register r holds row 8(r>>2) + 4(lane>>5) + (r&3), column lane & 31
  typename Ty<DT>::e* out = reinterpret_cast<typename Ty<DT>::e*>(a.out);
#pragma unroll
  for (int j = 0; j < NCB; ++j) {
    const int n = j * 32 + (lane & 31);
    if (n >= a.R) continue;
    const float sc = a.has_scale ? a.rs.s[n] : 1.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wave * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (m < a.T) out[(int64_t)m * a.ldo + n] = (typename Ty<DT>::e)(acc[j][r] * sc);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// wgrad: part[slab][i][j] = rscale[i] * sum_{t in slab} L[t][i] X[t][j].  Workgroup = (128 columns of K, one slab of rows); wave w owns the
// columns 32w .. 32w+31 and all NCB = ceil(R / 32) row blocks.  Both operands are staged as they lie in memory ([t][outer]) and read
// back transposed.
// ------------------------------------------------------------------------------------------------------------------------------------
struct WgradArgs {
  const uint16_t *l, *x; float* part;
  int64_t ldl, ldx;
  int T, R, K, rows_per, vl, vx, has_scale;
  RScale rs;
};

template <int DT, int NCB>
__global__ __launch_bounds__(256) void wgrad_k(WgradArgs a) {
  using V8 = typename Ty<DT>::v8;
  constexpr int LLD = NCB * 32 + 8, VPR = NCB * 4;          // pitch of the L image; 16-byte vectors per staged L row
  __shared__ __attribute__((aligned(16))) char lds_l[BK * LLD * 2];
  __shared__ __attribute__((aligned(16))) char lds_x[BK * XF_LD * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * 128;
  const int t0 = (int)blockIdx.y * a.rows_per, t1 = min(a.T, t0 + a.rows_per);
  f32x16 acc[NCB];
#pragma unroll
  for (int i = 0; i < NCB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  uint4 sl[NCB], sx[4];
  auto load = [&](int tb) {
#pragma unroll
    for (int i = 0; i < NCB; ++i) {
      const int v = tid + 256 * i, kk = v / VPR, oc = (v % VPR) * 8;
      sl[i] = tb + kk < t1 ? ld8(a.l, tb + kk, a.ldl, oc, a.R, a.vl) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = tid + 256 * i, kk = v >> 4, oc = (v & 15) * 8;
      sx[i] = tb + kk < t1 ? ld8(a.x, tb + kk, a.ldx, k0 + oc, a.K, a.vx) : uint4{0, 0, 0, 0};
    }
  };
  if (t0 < t1) load(t0);
  for (int tb = t0; tb < t1; tb += BK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NCB; ++i) { const int v = tid + 256 * i; *reinterpret_cast<uint4*>(lds_l + ((v / VPR) * LLD + (v % VPR) * 8) * 2) = sl[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int v = tid + 256 * i; *reinterpret_cast<uint4*>(lds_x + ((v >> 4) * XF_LD + (v & 15) * 8) * 2) = sx[i]; }
    __syncthreads();
    if (tb + BK < t1) load(tb + BK);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      if (tb + 16 * s >= t1) break;                          // uniform; rows beyond t1 are zero in the images
      const V8 fb = frag_ofast<V8>(lds_x, XF_LD, wave, s, lane);
#pragma unroll
      for (int i = 0; i < NCB; ++i) acc[i] = Ty<DT>::mma(frag_ofast<V8>(lds_l, LLD, i, s, lane), fb, acc[i]);
    }
  }
  float* out = a.part + (int64_t)blockIdx.y * a.R * a.K;
  const int n = k0 + wave * 32 + (lane & 31);
  if (n >= a.K) return;
#pragma unroll
  for (int i = 0; i < NCB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (m < a.R) out[(int64_t)m * a.K + n] = acc[i][r] * (a.has_scale ? a.rs.s[m] : 1.f);
    }
}

inline int vec_ok(const void* p, int64_t ld) { return aligned16(p) && ld % 8 == 0; }

// The kernel form of a down / wgrad call: f(DT, NCB) with DT the 16-bit storage type and NCB = 1, 2, 4 or 8 the rank class, the number of
// 32-wide blocks that hold the rank R <= 256
template <class F> inline void lora_form(int32_t dtype, int R, F&& f) {
  using std::integral_constant;
  dta_storage_type16(dtype, [&](auto dt) {
    if (R <= 32) f(dt, integral_constant<int, 1>{});
    else if (R <= 64) f(dt, integral_constant<int, 2>{});
    else if (R <= 128) f(dt, integral_constant<int, 4>{});
    else f(dt, integral_constant<int, 8>{});
  });
}

// rows of one slab of the weight gradient: whole 64-row steps, about 512 workgroups over (K tiles) x (slabs), at most 64 slabs
inline int slab_rows(int T, int K) {
  const int ktiles = (K + 127) / 128;
  int want = 512 / ktiles;
  want = want < 1 ? 1 : want > 64 ? 64 : want;
  int per = ((T + want - 1) / want + 63) / 64 * 64;
  return per < 64 ? 64 : per;
}

inline void fill_scale(RScale& rs, const float* h, int R) { for (int i = 0; i < MAXR; ++i) rs.s[i] = (h && i < R) ? h[i] : 1.f; }

}  // namespace

extern "C" {

int dta_lora_down(const void* x, int64_t ldx, const void* m, int64_t ldm, void* out, int64_t ldo, const float* rscale_host,
                  int32_t T, int32_t R, int32_t K, int32_t dtype, void* stream) {
  if (T < 0 || R <= 0 || K <= 0 || !x || !m || !out || ldx < K || ldm < K || ldo < R) return DTA_EINVAL;
  if (R > MAXR || K % 16 || (dtype != DTA_BF16 && dtype != DTA_F16)) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (T == 0) return DTA_OK;
  hipStream_t st = (hipStream_t)stream;
  DownArgs a{(const uint16_t*)x, (const uint16_t*)m, out, ldx, ldm, ldo, T, R, K, vec_ok(x, ldx), vec_ok(m, ldm), rscale_host != nullptr, {}};
  fill_scale(a.rs, rscale_host, R);
  const dim3 g(ceil_blocks(T, BM)), b(256);
  lora_form(dtype, R, [&](auto dt, auto ncb) { down_k<decltype(dt)::value, decltype(ncb)::value><<<g, b, 0, st>>>(a); });
  return DTA_LAUNCH_STATUS();
}

int dta_lora_wgrad_slabs(int32_t T, int32_t K) {
  if (T < 0 || K <= 0) return DTA_EINVAL;
  const int per = slab_rows(T, K);
  const int s = (T + per - 1) / per;
  return s < 1 ? 1 : s;
}

int dta_lora_wgrad(const void* l, int64_t ldl, const void* x, int64_t ldx, float* part, const float* rscale_host,
                   int32_t T, int32_t R, int32_t K, int32_t dtype, void* stream) {
  if (T < 0 || R <= 0 || K <= 0 || !l || !x || !part || ldl < R || ldx < K) return DTA_EINVAL;
  if (R > MAXR || K % 16 || (dtype != DTA_BF16 && dtype != DTA_F16)) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  WgradArgs a{(const uint16_t*)l, (const uint16_t*)x, part, ldl, ldx, T, R, K, slab_rows(T, K), vec_ok(l, ldl), vec_ok(x, ldx), rscale_host != nullptr, {}};
  fill_scale(a.rs, rscale_host, R);
  const dim3 g(ceil_blocks(K, 128), dta_lora_wgrad_slabs(T, K)), b(256);
  lora_form(dtype, R, [&](auto dt, auto ncb) { wgrad_k<decltype(dt)::value, decltype(ncb)::value><<<g, b, 0, st>>>(a); });
  return DTA_LAUNCH_STATUS();
}

}  // extern "C"
