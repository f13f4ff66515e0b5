// Fused row kernels of the decoder layer for gfx950 — HBM-bound, 16-byte accesses, fp32 math.
//   dta_rmsnorm_fwd/bwd        y = w · cast(x · rsqrt(mean(x²)+eps))                 (Qwen3RMSNorm arithmetic; w_offset: Gemma's single rounding)
//   dta_layernorm_fwd/bwd      y = cast(w · (x − mean(x)) · rsqrt(var(x)+eps)), x = x + delta_a + delta_b fused in   (CohereLayerNorm arithmetic)
//   dta_qk_norm_rope_fwd/bwd   per (token, head) of 128 or 64: optional RMSNorm, then RoPE at position = trie depth
//   dta_rope_partial_fwd/bwd   RoPE over the first R of D elements of a head, half-split or interleaved pairs (Phi, GLM)
//   dta_wide_qk_norm_rope_fwd/bwd  per token: RMSNorm over the whole [NH·D] projection row (OLMo), then RoPE per head
//   dta_rmsnorm_add_fwd        out = res + cast(w · y · rsqrt(mean(y²)+eps)): OLMo's post-norm branch end
//   dta_swiglu_fwd/bwd         y = cast(silu(g)) · u
//   dta_geglu_fwd/bwd          y = cast(gelu_tanh(g)) · u                              (Gemma)
//   dta_transpose              2-D transpose of 2- or 4-byte elements
//   dta_sum_slabs              fp32 sum of the per-workgroup weight-gradient partials, rounded to the parameter dtype
// These replace ~40 torch elementwise launches per layer (fp32 up-casts included); together they are ~18 ms of a
// 250 ms step (profiles/r1_bench_kernel_stats.csv).  Reference call sites: the model call of
// tree_training_engine.py:182-186, 248-252, 351-353 (third-party transformers Qwen3 layers).
// The algorithms the kernels share - row pass, norm backward, dw reduction, RoPE exchange, unit decode - stand once each at the top of
// the file; a kernel supplies its per-element arithmetic as functors.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dta_common.h"
#include "dta_device.h"

namespace {

// fp32 models (the reference's --dtype fp32, run.py:122-132): the same kernels with Ty<DTA_F32>

// A saved activation read back in a backward kernel: written a whole forward ago, in no cache, so read non-temporally
// (the 8 elements at p; DT and not the vector type is the template argument: a deduced vector type would drop the 16-byte alignment of f32x8)
template <int DT> __device__ __forceinline__ typename Ty<DT>::v8 saved_load(const typename Ty<DT>::e* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const typename Ty<DT>::v8*>(p));
}

// ---------------------------------------------------------------------------------------------
// The shared row algorithms.  A row of nv 16-byte groups is spread over L lanes: lane l owns the groups i = l + L a, a < NA.
// ---------------------------------------------------------------------------------------------
// f(a, i) for every a < per_lane on every lane, inside the row or not: per_lane is uniform over the L lanes, so f may shuffle.  `a` is a
// constant after unrolling: arrays indexed by it stay in registers.
template <int NA, class F> __device__ __forceinline__ void row_groups_uniform(int lane, int L, int per_lane, F&& f) {
#pragma unroll
  for (int a = 0; a < NA; ++a)
    if (a < per_lane) f(a, lane + L * a);
}
// f(a, i) for the lane's groups inside the row.  per_lane = ceil(nv / L) skips whole groups by a uniform branch; NA where the kernel
// has no use for that.
template <int NA, class F> __device__ __forceinline__ void row_groups(int lane, int L, int nv, int per_lane, F&& f) {
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = lane + L * a;
    if (a < per_lane && i < nv) f(a, i);
  }
}

// RMS forward row pass over a row of n = 8 nv elements held in registers (nv <= L NA): v = load(i) (which may do more: add a delta, store
// x_out), sum of squares, sum(ss) over the row's lanes, r = rsqrt(mean + eps) written once to rstd[row], then finish(i, live, v, r) for
// every a < per_lane - `live` telling whether group i lies inside the row: a finish that shuffles needs the dead lanes, any other
// returns at once.  ONE read of the row.
template <int NA, int DT, class Load, class Sum, class Finish>
__device__ __forceinline__ void rms_row_pass(int lane, int L, int nv, int per_lane, int n, float eps, float* rstd, int row, Load&& load, Sum&& sum,
                                             Finish&& finish) {
  using V8 = typename Ty<DT>::v8;
  V8 keep[NA];
  float ss = 0.f;
  auto squares = [&](const V8& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; ss = __builtin_fmaf(f, f, ss); }
  };
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const int i = lane + L * a;
    if (a < per_lane && i < nv) { const V8 v = load(i); squares(v); keep[a] = v; }
  }
  const float r = __builtin_amdgcn_rsqf(sum(ss) / (float)n + eps);
  if (lane == 0) rstd[row] = r;
#pragma unroll
  for (int a = 0; a < NA; ++a)
    if (a < per_lane) finish(lane + L * a, lane + L * a < nv, keep[a], r);
}

// The 4 waves' weight-gradient accumulators (one wave per row, 64 lanes) summed through LDS, one 16-byte group at a time, into the
// workgroup's row `out` of the partials.  `a < per_lane` is block-uniform: every wave meets the barriers.
template <int NA> __device__ __forceinline__ void dw_reduce(const float (&acc)[NA][8], float (&red)[4 * 64 * 8], float* out, int nv, int per_lane) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    if (a < per_lane) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; ++j) red[(wave * 64 + lane) * 8 + j] = acc[a][j];
      __syncthreads();
      if (wave == 0) {
        const int i = lane + 64 * a;
        if (i < nv) {
#pragma unroll
          for (int j = 0; j < 8; ++j) out[8 * i + j] = red[lane * 8 + j] + red[(64 + lane) * 8 + j] + red[(128 + lane) * 8 + j] + red[(192 + lane) * 8 + j];
        }
      }
    }
  }
}

// Norm backward over rows of H <= 512 NA elements: one wave per row, 4 rows per workgroup, grid-stride; dw partial per workgroup.
// row_of(row) gives the row's state S with
//   S.that(x)           the normalised element t̂
//   S.add(dy, w, t̂)     one element's terms of the row statistics;   S.reduce(H)   the statistics over the row, between the two sweeps
//   S.dx(x, dy, w, dres, at)  the 8 gradients of a group; dres = the [R, H] gradient arriving on the residual stream (it joins dx here: one
//                       pass less) or null, `at` = the group's place in it - what a null dres means to the rounding is the norm's own
//                       business, and the test of the kernel argument itself keeps the branch uniform.  The three vectors go by
//                       value: behind references the fp32 forms compiled to other multiplies and other bits
// and the skeleton does the rest: dw += dy·t̂ per element in acc[NA][8]; x (read as a saved activation) and dy stay in registers between
// the sweeps where that fits (KEEP: <= 64 VGPRs) and are read again where not; a null dw_part (frozen weight) ends the kernel after dx.
template <int DT, int NA, class RowOf>
__device__ __forceinline__ void norm_bwd(const void* x_, const void* w_, const void* dy_, const void* dres_, void* dx_, float* dw_part, int R, int H,
                                         float (&red)[4 * 64 * 8], RowOf&& row_of) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const e* w = reinterpret_cast<const e*>(w_);
  const int nv = H >> 3;
  const int per_lane = (nv + 63) >> 6;                      // <= NA
  constexpr bool KEEP = NA * sizeof(v8) <= 128;
  float acc[NA][8] = {};
  for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
    const e* x = reinterpret_cast<const e*>(x_) + (int64_t)row * H;
    const e* dy = reinterpret_cast<const e*>(dy_) + (int64_t)row * H;
    e* dx = reinterpret_cast<e*>(dx_) + (int64_t)row * H;
    auto st = row_of(row);
    v8 kx[KEEP ? NA : 1], kg[KEEP ? NA : 1];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int i = lane + 64 * a;
      if (!(a < per_lane && i < nv)) continue;
      const v8 v = saved_load<DT>(x + 8 * i); const v8 g = *reinterpret_cast<const v8*>(dy + 8 * i);
      const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float t = st.that((float)v[j]); const float gg = (float)g[j]; st.add(gg, (float)wv[j], t); acc[a][j] = __builtin_fmaf(gg, t, acc[a][j]); }
      if constexpr (KEEP) { kx[a] = v; kg[a] = g; }
    }
    st.reduce(H);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int i = lane + 64 * a;
      if (!(a < per_lane && i < nv)) continue;
      v8 v, g;
      if constexpr (KEEP) { v = kx[a]; g = kg[a]; }
      else { v = *reinterpret_cast<const v8*>(x + 8 * i); g = *reinterpret_cast<const v8*>(dy + 8 * i); }
      const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
      *reinterpret_cast<v8*>(dx + 8 * i) = st.dx(v, g, wv, dres_, (int64_t)row * H + 8 * i);
    }
  }
  if (!dw_part) return;                                       // block-uniform
  dw_reduce<NA>(acc, red, dw_part + (int64_t)blockIdx.x * H, nv, per_lane);
}

// rotate_half RoPE.  LPH = D/8 lanes own one head, 8 elements each (sub = the lane's place in its head): element i pairs with i +- D/2,
// which is lane sub ^ (LPH/2) of the same head.  rope_table: the lane's 8 cos and 8 signed sin values of token tok from
// cs [T, D] = {cos[D/2], sin[D/2]}; sign +1 rotates by the token's angle (forward), -1 by its negative (backward).
template <int D> __device__ __forceinline__ void rope_table(const float* cs, int64_t tok, int sub, float sign, float (&cj)[8], float (&sj)[8]) {
  constexpr int LPH = D / 8;
  const float* c = cs + tok * D + 8 * (sub & (LPH / 2 - 1));
#pragma unroll
  for (int j = 0; j < 8; ++j) { cj[j] = c[j]; sj[j] = sub < LPH / 2 ? -(sign * c[D / 2 + j]) : sign * c[D / 2 + j]; }
}
// out = a rotated; the partner's a arrives by shuffle, so the call is wave-uniform or under a condition a lane shares with its partner
template <int LPH> __device__ __forceinline__ void rotate_half(const float (&a)[8], const float (&cj)[8], const float (&sj)[8], float (&out)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float other = __shfl_xor(a[j], LPH / 2);
    out[j] = a[j] * cj[j] + other * sj[j];
  }
}

// The (token, head group) unit of a lane group in the head kernels: a workgroup pass starting at unit `base` takes 4·64/LPH units, HPL
// heads of one token each.  A lane group past the end is not live and runs along on the last unit, so the shuffles of a grid-stride
// kernel stay uniform and its addresses valid; it stores nothing.  ONE_PASS (the grid covers every unit): such a group leaves at once,
// so nothing is clamped and only `live` of its result means anything.
struct HeadUnit { int64_t tok; int head0; bool live; };
template <int HPL, int D, bool ONE_PASS> __device__ __forceinline__ HeadUnit head_unit(int64_t base, int64_t n_units, int NH) {
  constexpr int LPH = D / 8, LSH = D == 128 ? 4 : 3;              // lanes per head, log2
  const int64_t unit = base + (threadIdx.x >> 6) * (64 / LPH) + ((threadIdx.x & 63) >> LSH);
  const bool live = unit < n_units;
  const int64_t uc = ONE_PASS || live ? unit : n_units - 1;
  const int groups = NH / HPL;
  const int64_t tok = uc / groups;
  return {tok, (int)(uc - tok * groups) * HPL, live};
}

// ---------------------------------------------------------------------------------------------
// RMSNorm over rows of H (H % 8 == 0; forward: any H, backward: H <= 8192).  One wave per row, 4 rows per workgroup, grid-stride.
// ---------------------------------------------------------------------------------------------
// OFF (w_offset != 0, the Gemma form): y = cast(x·r·(w_off + w)) - the weight offset is added in fp32 inside the kernel and the
// product is rounded ONCE (the default form rounds x·r to the storage type first, as Qwen3RMSNorm does).  OFF = false: w_off is unused.
// NA > 0: rows of H <= 512*NA elements, kept in registers (rms_row_pass); NA == 0: any H, second pass re-reads the row (L2-hot).
template <int DT, int NA, bool OFF = false>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const void* __restrict__ x_, const void* __restrict__ delta_, const void* __restrict__ w_,
                                                          void* __restrict__ xout_, void* __restrict__ y_,
                                                          float* __restrict__ rstd, int R, int H, float eps, float w_off = 0.f) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const e* w = reinterpret_cast<const e*>(w_);
  const int nv = H >> 3;
  for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
    const e* x = reinterpret_cast<const e*>(x_) + (int64_t)row * H;
    e* y = reinterpret_cast<e*>(y_) + (int64_t)row * H;
    auto finish = [&](int i, bool live, const v8& v, float r) {
      if (!live) return;
      const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
      v8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if constexpr (OFF) o[j] = (e)((float)v[j] * r * (w_off + (float)wv[j]));
        else { const e t = (e)((float)v[j] * r); o[j] = (e)((float)wv[j] * (float)t); }
      }
      *reinterpret_cast<v8*>(y + 8 * i) = o;
    };
    if constexpr (NA > 0) {
      const e* dl = delta_ ? reinterpret_cast<const e*>(delta_) + (int64_t)row * H : nullptr;
      e* xo = delta_ ? reinterpret_cast<e*>(xout_) + (int64_t)row * H : nullptr;
      rms_row_pass<NA, DT>(
          lane, 64, nv, NA, H, eps, rstd, row,
          [&](int i) {                                     // residual stream update fused in: x_out = x + delta (rounded), then normalised
            v8 v = *reinterpret_cast<const v8*>(x + 8 * i);
            if (dl) {
              const v8 d = *reinterpret_cast<const v8*>(dl + 8 * i);
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = (e)((float)v[j] + (float)d[j]);
              *reinterpret_cast<v8*>(xo + 8 * i) = v;
            }
            return v;
          },
          [](float ss) { return wave_sum(ss); }, finish);
    } else {                                               // any H: the row is read twice, its loops written out
      float ss = 0.f;
      if (delta_) {                                      // residual stream update fused in: x_out = x + delta (rounded), then normalised
        const e* dl = reinterpret_cast<const e*>(delta_) + (int64_t)row * H;
        e* xo = reinterpret_cast<e*>(xout_) + (int64_t)row * H;
        for (int i = lane; i < nv; i += 64) {
          const v8 v = *reinterpret_cast<const v8*>(x + 8 * i); const v8 d = *reinterpret_cast<const v8*>(dl + 8 * i);
          v8 o;
#pragma unroll
          for (int j = 0; j < 8; ++j) { o[j] = (e)((float)v[j] + (float)d[j]); const float f = (float)o[j]; ss = __builtin_fmaf(f, f, ss); }
          *reinterpret_cast<v8*>(xo + 8 * i) = o;
        }
        x = xo;                                          // second pass re-reads the wave's own (L1/L2-hot) row
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      } else {
        for (int i = lane; i < nv; i += 64) {
          const v8 v = *reinterpret_cast<const v8*>(x + 8 * i);
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; ss = __builtin_fmaf(f, f, ss); }
        }
      }
      ss = wave_sum(ss);
      const float r = __builtin_amdgcn_rsqf(ss / (float)H + eps);
      if (lane == 0) rstd[row] = r;
      for (int i = lane; i < nv; i += 64) finish(i, true, *reinterpret_cast<const v8*>(x + 8 * i), r);
    }
  }
}

// dx = r·(dt − t̂·mean(dt·t̂)), dt = dy·w, t̂ = x·r ;  dw partial per workgroup: Σ_rows dy·t̂.
// NA = v8 groups per lane (dw accumulators in registers): 2/4/8 for H <= 1024/2048/4096, 16 for H <= 8192 (Qwen3-14B/32B hidden 5120).
// OFF: dt = dy·(w_off + w); dw is unchanged (d(w_off + w)/dw = 1).  A null dres drops the add: two dx expressions.
template <int DT, bool OFF> struct RmsBwdRow {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  float r, w_off, dot;
  __device__ __forceinline__ float wof(float w) const { if constexpr (OFF) return w_off + w; else return w; }
  __device__ __forceinline__ float that(float x) const { return x * r; }
  __device__ __forceinline__ void add(float gg, float w, float t) { dot = __builtin_fmaf(gg * wof(w), t, dot); }
  __device__ __forceinline__ void reduce(int H) { dot = wave_sum(dot) / (float)H; }
  __device__ __forceinline__ v8 dx(v8 v, v8 g, v8 wv, const void* dres_, int64_t at) const {
    v8 o;
    if (dres_) {
      const v8 dr = *reinterpret_cast<const v8*>(reinterpret_cast<const e*>(dres_) + at);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float t = (float)v[j] * r; o[j] = (e)(r * ((float)g[j] * wof((float)wv[j]) - t * dot) + (float)dr[j]); }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float t = (float)v[j] * r; o[j] = (e)(r * ((float)g[j] * wof((float)wv[j]) - t * dot)); }
    }
    return o;
  }
};
template <int DT, int NA, bool OFF = false>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const void* __restrict__ x_, const void* __restrict__ w_, const void* __restrict__ dy_,
                                                          const void* __restrict__ dres_,
                                                          const float* __restrict__ rstd, void* __restrict__ dx_, float* __restrict__ dw_part,
                                                          int R, int H, float w_off = 0.f) {
  __shared__ float red[4 * 64 * 8];
  norm_bwd<DT, NA>(x_, w_, dy_, dres_, dx_, dw_part, R, H, red, [&](int row) { return RmsBwdRow<DT, OFF>{rstd[row], w_off, 0.f}; });
}

// ---------------------------------------------------------------------------------------------
// LayerNorm without bias over rows of H (CohereLayerNorm; H % 8 == 0, H <= 8192 = 512·NA).  One wave per row, 4 rows per workgroup,
// grid-stride.  The row stays in registers for three passes: Σx -> m, Σ(x-m)² -> r (the centred form: E[x²]-m² in fp32 loses rstd to
// cancellation on rows with a common offset), then y = cast(w·((x-m)·r)) with ONE rounding.  x is read once, y written once.
// da / db: the pending branch outputs of the parallel block, x_out = cast((x + da) + db) summed in fp32 and rounded once; db may be null.
// ---------------------------------------------------------------------------------------------
template <int DT, int NA>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const void* __restrict__ x_, const void* __restrict__ da_, const void* __restrict__ db_,
                                                            const void* __restrict__ w_, void* __restrict__ xout_, void* __restrict__ y_,
                                                            float* __restrict__ mean, float* __restrict__ rstd, int R, int H, float eps) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const e* w = reinterpret_cast<const e*>(w_);
  const int nv = H >> 3;
  const float inv_h = 1.f / (float)H;
  for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
    const e* x = reinterpret_cast<const e*>(x_) + (int64_t)row * H;
    const e* da = da_ ? reinterpret_cast<const e*>(da_) + (int64_t)row * H : nullptr;
    const e* db = db_ ? reinterpret_cast<const e*>(db_) + (int64_t)row * H : nullptr;
    e* xo = da_ ? reinterpret_cast<e*>(xout_) + (int64_t)row * H : nullptr;
    e* y = reinterpret_cast<e*>(y_) + (int64_t)row * H;
    v8 keep[NA];
    float s = 0.f;
    row_groups<NA>(lane, 64, nv, NA, [&](int a, int i) {
      v8 v = *reinterpret_cast<const v8*>(x + 8 * i);
      if (da) {
        const v8 d = *reinterpret_cast<const v8*>(da + 8 * i);
        if (db) {
          const v8 d2 = *reinterpret_cast<const v8*>(db + 8 * i);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (e)(((float)v[j] + (float)d[j]) + (float)d2[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (e)((float)v[j] + (float)d[j]);
        }
        *reinterpret_cast<v8*>(xo + 8 * i) = v;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (float)v[j];
      keep[a] = v;
    });
    const float m = wave_sum(s) * inv_h;
    float q = 0.f;
    row_groups<NA>(lane, 64, nv, NA, [&](int a, int) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float c = (float)keep[a][j] - m; q = __builtin_fmaf(c, c, q); }
    });
    const float r = __builtin_amdgcn_rsqf(wave_sum(q) * inv_h + eps);
    if (lane == 0) { mean[row] = m; rstd[row] = r; }
    row_groups<NA>(lane, 64, nv, NA, [&](int a, int i) {
      const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
      v8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (e)((float)wv[j] * (((float)keep[a][j] - m) * r));
      *reinterpret_cast<v8*>(y + 8 * i) = o;
    });
  }
}

// t = (x-m)·r, g = dy·w:  dx = r·(g − mean(g) − t·mean(g·t)) + dres ;  dw partial per workgroup: Σ_rows dy·t.  NA and KEEP as
// rmsnorm_bwd_kernel (norm_bwd), so the workspace has dta_layernorm_bwd_blocks(R) rows.
template <int DT> struct LnBwdRow {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  float m, r, sg, sgt;
  __device__ __forceinline__ float that(float x) const { return (x - m) * r; }
  __device__ __forceinline__ void add(float gg, float w, float t) { const float gw = gg * w; sg += gw; sgt = __builtin_fmaf(gw, t, sgt); }
  __device__ __forceinline__ void reduce(int H) { const float inv_h = 1.f / (float)H; sg = wave_sum(sg) * inv_h; sgt = wave_sum(sgt) * inv_h; }
  // the gradient on the residual stream joins here; both deltas share this dx.  ONE expression for both forms (dres NULL adds a
  // zero), so that a NULL dres and a dres of zeros give the same bits whatever the compiler fuses
  __device__ __forceinline__ v8 dx(v8 v, v8 g, v8 wv, const void* dres_, int64_t at) const {
    v8 dr, o;
    if (dres_) dr = *reinterpret_cast<const v8*>(reinterpret_cast<const e*>(dres_) + at);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) dr[j] = (e)0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float t = ((float)v[j] - m) * r; o[j] = (e)(r * (((float)g[j] * (float)wv[j] - sg) - t * sgt) + (float)dr[j]); }
    return o;
  }
};
template <int DT, int NA>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const void* __restrict__ x_, const void* __restrict__ w_, const void* __restrict__ dy_,
                                                            const void* __restrict__ dres_, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, void* __restrict__ dx_, float* __restrict__ dw_part,
                                                            int R, int H) {
  __shared__ float red[4 * 64 * 8];
  norm_bwd<DT, NA>(x_, w_, dy_, dres_, dx_, dw_part, R, H, red, [&](int row) { return LnBwdRow<DT>{mean[row], rstd[row], 0.f, 0.f}; });
}

// ---------------------------------------------------------------------------------------------
// q/k head-norm + RoPE.  x: [T, NH, D], D = 128 or 64; LPH = D/8 lanes own one head (8 elements each); a wave = 64/LPH heads (4 or 8).
// cs: [T, D] float = {cos[0..D/2-1], sin[0..D/2-1]} of the token's depth.  w == NULL: RoPE only.
// ---------------------------------------------------------------------------------------------
// HPL = heads of ONE token per LPH-lane group (4 when NH % 4 == 0): the token's cos/sin values - 64 bytes per lane, four times the 16 bytes
// of x - are fetched once and reused, and HPL independent 16-byte loads are in flight per lane.
template <int DT, int HPL, int D>
__global__ __launch_bounds__(256) void qk_norm_rope_fwd_kernel(const void* __restrict__ x_, const void* __restrict__ w_, const float* __restrict__ cs,
                                                               void* __restrict__ y_, float* __restrict__ rstd, int64_t n_units, int NH,
                                                               int64_t x_st, float eps) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  constexpr int LPH = D / 8, UPB = 4 * (64 / LPH);
  const int sub = threadIdx.x & (LPH - 1);
  const HeadUnit u = head_unit<HPL, D, true>((int64_t)blockIdx.x * UPB, n_units, NH);
  if (!u.live) return;                                     // (a lane group is one unit: the partner lanes of a shuffle leave together)
  const e* x = reinterpret_cast<const e*>(x_) + u.tok * x_st + (int64_t)u.head0 * D + 8 * sub;
  const int64_t hid0 = u.tok * NH + u.head0;
  e* y = reinterpret_cast<e*>(y_) + hid0 * D + 8 * sub;
  v8 v[HPL];
#pragma unroll
  for (int h = 0; h < HPL; ++h) v[h] = *reinterpret_cast<const v8*>(x + h * D);
  float cj[8], sj[8];
  rope_table<D>(cs, u.tok, sub, 1.f, cj, sj);
  v8 wv;
  if (w_) wv = *reinterpret_cast<const v8*>(reinterpret_cast<const e*>(w_) + 8 * sub);
#pragma unroll
  for (int h = 0; h < HPL; ++h) {
    float a[8], rot[8];
    if (w_) {
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float f = (float)v[h][j]; ss = __builtin_fmaf(f, f, ss); }
#pragma unroll
      for (int o = LPH / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
      const float r = __builtin_amdgcn_rsqf(ss * (1.f / D) + eps);
      if (sub == 0) rstd[hid0 + h] = r;
#pragma unroll
      for (int j = 0; j < 8; ++j) { const e t = (e)((float)v[h][j] * r); a[j] = (float)(e)((float)wv[j] * (float)t); }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (float)v[h][j];
    }
    rotate_half<LPH>(a, cj, sj, rot);
    v8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (e)rot[j];
    *reinterpret_cast<v8*>(y + h * D) = o;
  }
}

// dx_ may be dy_ (in place): a lane writes exactly the 16-byte groups it read; its partner's values arrive through registers.
template <int DT, int HPL, int D>
__global__ __launch_bounds__(256) void qk_norm_rope_bwd_kernel(const void* __restrict__ x_, const void* __restrict__ w_, const float* __restrict__ cs,
                                                               const void* dy_, const float* __restrict__ rstd,
                                                               void* dx_, float* __restrict__ dw_part, int64_t n_units, int NH,
                                                               int64_t x_st, int64_t dy_st_t, int64_t dy_st_h, int64_t dx_st) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  constexpr int LPH = D / 8, UPB = 4 * (64 / LPH);          // lanes per head, (token, head group) units per workgroup pass
  __shared__ float red[256 * 8];
  const int sub = threadIdx.x & (LPH - 1);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  v8 wv;
  if (w_) wv = *reinterpret_cast<const v8*>(reinterpret_cast<const e*>(w_) + 8 * sub);
  for (int64_t base = (int64_t)blockIdx.x * UPB; base < n_units; base += (int64_t)gridDim.x * UPB) {
    const HeadUnit u = head_unit<HPL, D, false>(base, n_units, NH);
    const e* dy = reinterpret_cast<const e*>(dy_) + u.tok * dy_st_t + (int64_t)u.head0 * dy_st_h + 8 * sub;
    v8 g[HPL], v[HPL];
#pragma unroll
    for (int h = 0; h < HPL; ++h) g[h] = *reinterpret_cast<const v8*>(dy + h * dy_st_h);
    if (w_) {
      const e* x = reinterpret_cast<const e*>(x_) + u.tok * x_st + (int64_t)u.head0 * D + 8 * sub;
#pragma unroll
      for (int h = 0; h < HPL; ++h) v[h] = saved_load<DT>(x + h * D);
    }
    float cj[8], sj[8];
    rope_table<D>(cs, u.tok, sub, -1.f, cj, sj);
    e* dx = reinterpret_cast<e*>(dx_) + u.tok * dx_st + (int64_t)u.head0 * D + 8 * sub;
#pragma unroll
    for (int h = 0; h < HPL; ++h) {
      float gf[8], da[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) gf[j] = (float)g[h][j];
      rotate_half<LPH>(gf, cj, sj, da);
      v8 o;
      if (w_) {
        const float r = rstd[u.tok * NH + u.head0 + h];
        float dot = 0.f, t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { t[j] = (float)v[h][j] * r; dot = __builtin_fmaf(da[j] * (float)wv[j], t[j], dot); if (u.live) acc[j] = __builtin_fmaf(da[j], t[j], acc[j]); }
#pragma unroll
        for (int o2 = LPH / 2; o2 > 0; o2 >>= 1) dot += __shfl_xor(dot, o2);
        dot *= (1.f / D);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (e)(r * (da[j] * (float)wv[j] - t[j] * dot));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (e)da[j];
      }
      if (u.live) *reinterpret_cast<v8*>(dx + h * D) = o;
    }
  }
  if (w_ && dw_part) {                                   // dw partial [gridDim.x, D]; none for a frozen weight (dw_part NULL)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < D) {
      const int s = threadIdx.x >> 3, j = threadIdx.x & 7;                   // element 8*s + j: the lanes sub == s of all 256/LPH heads
      float t = 0.f;
      for (int g2 = 0; g2 < 256 / LPH; ++g2) t += red[(g2 * LPH + s) * 8 + j];
      dw_part[(int64_t)blockIdx.x * D + threadIdx.x] = t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// RoPE over the first R of D elements of a head (Phi-3 / Phi-4-mini, GLM-4), no norm: elements R .. D-1 pass through bit for bit.
// cs: [T, R] float = {cos[R/2], sin[R/2]}.  The lane layout is that of qk_norm_rope_*: LPH = D/8 lanes own one head, 8 elements each, and
// HPL heads of one token share the lane group's table values.  A lane whose 8 elements lie at or past R (sub >= R/8) reads no table entry
// and stores the vector it loaded.
//   PAIR 0 (half-split, R % 16 == 0): element i <-> i + R/2, i.e. lane sub <-> sub +- R/16 of the same head.  R/16 is 3 for R = 48 and 6
//     for R = 96 - no power of two - so the partner's value comes by an indexed shuffle.
//   PAIR 1 (interleaved, R % 8 == 0): element 2i <-> 2i+1, both inside the lane's own 8 elements; the lane reads 4 cos and 4 sin.
// One kernel serves both directions: sgn = +1 rotates by the token's angle (forward), -1 by its negative (the backward).  ONE_PASS (the
// forward): the grid covers every unit and a lane group past the end leaves at once, as in qk_norm_rope_fwd_kernel; otherwise grid-stride
// over (token, head group) units; out_ may be in_ with the same strides (in place): a lane writes exactly the bytes it read, partner
// values travel through registers.  No LDS.
// ---------------------------------------------------------------------------------------------
template <int DT, int HPL, int D, int PAIR, bool ONE_PASS>
__global__ __launch_bounds__(256) void rope_partial_kernel(const void* in_, const float* __restrict__ cs, void* out_, int64_t n_units, int NH, int R,
                                                           int64_t in_st_t, int64_t in_st_h, int64_t out_st_t, float sgn) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  constexpr int LPH = D / 8, UPB = 4 * (64 / LPH);
  const int lane = threadIdx.x & 63, sub = lane & (LPH - 1);
  const bool rot = 8 * sub < R;
  const int half = R >> 4;                                 // PAIR 0: lanes per rotated half
  const bool lo = sub < half;
  const int src = PAIR == 0 && rot ? (lo ? lane + half : lane - half) : lane;
  for (int64_t base = (int64_t)blockIdx.x * UPB; base < n_units; base += (int64_t)gridDim.x * UPB) {
    const HeadUnit u = head_unit<HPL, D, ONE_PASS>(base, n_units, NH);
    if (ONE_PASS && !u.live) return;                       // (a lane group is one unit: the partner lanes of a shuffle leave together)
    const e* in = reinterpret_cast<const e*>(in_) + u.tok * in_st_t + (int64_t)u.head0 * in_st_h + 8 * sub;
    v8 v[HPL];
#pragma unroll
    for (int h = 0; h < HPL; ++h) v[h] = *reinterpret_cast<const v8*>(in + h * in_st_h);
    float cj[8], sj[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cj[j] = 0.f; sj[j] = 0.f; }
    if (rot) {
      if (PAIR == 0) {
        const float* c = cs + u.tok * R + 8 * (lo ? sub : sub - half);
        const float sg = lo ? -sgn : sgn;
#pragma unroll
        for (int j = 0; j < 8; ++j) { cj[j] = c[j]; sj[j] = sg * c[(R >> 1) + j]; }
      } else {
        const float* c = cs + u.tok * R + 4 * sub;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = sgn * c[(R >> 1) + i];
          cj[2 * i] = cj[2 * i + 1] = c[i]; sj[2 * i] = -s; sj[2 * i + 1] = s;
        }
      }
    }
    e* out = reinterpret_cast<e*>(out_) + u.tok * out_st_t + (int64_t)u.head0 * D + 8 * sub;
#pragma unroll
    for (int h = 0; h < HPL; ++h) {
      v8 o = v[h];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float a = (float)v[h][j];
        const float other = PAIR == 0 ? __shfl(a, src) : (float)v[h][j ^ 1];
        if (rot) o[j] = (e)(a * cj[j] + other * sj[j]);
      }
      if (u.live) *reinterpret_cast<v8*>(out + h * D) = o;
    }
    if (ONE_PASS) break;
  }
}

// ---------------------------------------------------------------------------------------------
// OLMo-2 / OLMo-3: q/k RMSNorm over the WHOLE projection row (NH*D <= 8192 elements, weight [NH*D]), then RoPE per head.
// WPT = waves per token.  Rows of up to 2 048 elements: one wave per token, 4 tokens per workgroup (WPT 1); longer rows: the 4 waves of
// a workgroup share one token (WPT 4) - at most 4 groups per lane either way, where one wave holding a row of 8 192 (16 groups per lane)
// ran at 2 waves / SIMD forward and 1 backward and reached 0.36 / 0.23 of 8 TB/s at 5 120.  Grid-stride over tokens.  Lane l of the
// L = 64 WPT lanes of a token owns the 16-byte groups i = l + L a (a < NA) of the row: group i is elements 8i .. 8i+7 of head 8i / D.
// L is a multiple of LPH = D / 8, so a lane's position inside its head (sub = l % LPH) - and with it its 8 cos / 8 sin values - is the
// same for every a: the token's table row is fetched once and reused across its heads; the rotate_half partner of group i is group
// i ^ (LPH/2) = lane l ^ (LPH/2) of the same wave at the same a (an NH*D row is a whole number of heads, so both are live or neither
// is).  The row stays in registers between the sum of squares and the scaling: one read of x.  The row sums are wave shuffles, and
// with WPT 4 one LDS word per wave.
// ---------------------------------------------------------------------------------------------
// sum of v over the lanes of one token: the wave's shuffles, and for WPT 4 the four waves' sums through `slot` (4 floats of LDS; the two
// barriers make the slot reusable by the next call - every wave of the workgroup runs the same token loop, so they are uniform)
template <int WPT> __device__ __forceinline__ float token_sum(float v, float* slot) {
  v = wave_sum(v);
  if constexpr (WPT == 1) return v;
  else {
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = (slot[0] + slot[1]) + (slot[2] + slot[3]);
    __syncthreads();
    return t;
  }
}

template <int DT, int NA, int D, int WPT>
__global__ __launch_bounds__(256) void wide_qk_norm_rope_fwd_kernel(const void* __restrict__ x_, const void* __restrict__ w_, const float* __restrict__ cs,
                                                                    void* __restrict__ y_, float* __restrict__ rstd, int T, int n,
                                                                    int64_t x_st, float eps) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  constexpr int LPH = D / 8, L = 64 * WPT, TPB = 4 / WPT;     // lanes per head, lanes per token, tokens per workgroup pass
  __shared__ float slot[4];
  const int lane = WPT == 1 ? (threadIdx.x & 63) : threadIdx.x, sub = lane & (LPH - 1);
  const e* w = reinterpret_cast<const e*>(w_);
  const int nv = n >> 3;
  const int per_lane = (nv + L - 1) / L;                    // <= NA, workgroup-uniform
  for (int tok = blockIdx.x * TPB + (WPT == 1 ? (threadIdx.x >> 6) : 0); tok < T; tok += gridDim.x * TPB) {
    const e* x = reinterpret_cast<const e*>(x_) + (int64_t)tok * x_st;
    e* y = reinterpret_cast<e*>(y_) + (int64_t)tok * n;
    float cj[8], sj[8];
    rope_table<D>(cs, tok, sub, 1.f, cj, sj);
    auto load = [&](int i) { return *reinterpret_cast<const v8*>(x + 8 * i); };
    rms_row_pass<NA, DT>(lane, L, nv, per_lane, n, eps, rstd, tok, load, [&](float ss) { return token_sum<WPT>(ss, slot); },
                         [&](int i, bool live, const v8& v, float r) {      // every lane takes part in the shuffles
                           float av[8], rot[8];
                           if (live) {
                             const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
#pragma unroll
                             for (int j = 0; j < 8; ++j) av[j] = (float)(e)((float)wv[j] * ((float)v[j] * r));      // Olmo2RMSNorm: w · x · r in fp32, ONE rounding
                           } else {
#pragma unroll
                             for (int j = 0; j < 8; ++j) av[j] = 0.f;
                           }
                           rotate_half<LPH>(av, cj, sj, rot);
                           v8 o;
#pragma unroll
                           for (int j = 0; j < 8; ++j) o[j] = (e)rot[j];
                           if (live) *reinterpret_cast<v8*>(y + 8 * i) = o;
                         });
  }
}

// da = un-rotated dy in fp32 (never rounded); dx = r·(da·w − t̂·mean_n(da·w·t̂)), t̂ = x·r; dw partial per workgroup: Σ_tokens da·t̂.
// dx_ may be dy_ (in place): a lane writes exactly the 16-byte groups it read; its partner's values arrive through registers.  x and dy
// of the row stay in registers between the two passes (NA <= 4 groups per lane: at most 64 VGPRs).  Not norm_bwd: the rows are strided
// by head, the rotation needs the dead lanes of a group, and with WPT 4 neither the row sum nor the dw partials go the one-wave way.
template <int DT, int NA, int D, int WPT>
__global__ __launch_bounds__(256) void wide_qk_norm_rope_bwd_kernel(const void* __restrict__ x_, const void* __restrict__ w_, const float* __restrict__ cs,
                                                                    const void* dy_, const float* __restrict__ rstd, void* dx_,
                                                                    float* __restrict__ dw_part, int T, int n, int64_t x_st, int64_t dy_st_t,
                                                                    int64_t dy_st_h, int64_t dx_st) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  constexpr int LPH = D / 8, LSH = D == 128 ? 4 : 3, L = 64 * WPT, TPB = 4 / WPT;
  __shared__ float red[WPT == 1 ? 4 * 64 * 8 : 4];          // WPT 1: the 4 waves' dw partials; WPT 4: the row sum's slot
  const int lane = WPT == 1 ? (threadIdx.x & 63) : threadIdx.x, wave = threadIdx.x >> 6, sub = lane & (LPH - 1);
  const e* w = reinterpret_cast<const e*>(w_);
  const int nv = n >> 3;
  const int per_lane = (nv + L - 1) / L;                    // <= NA, block-uniform
  float acc[NA][8] = {};
  auto unrotate = [&](const v8& g, const float (&cj)[8], const float (&sj)[8], float (&da)[8]) {
    float gf[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) gf[j] = (float)g[j];
    rotate_half<LPH>(gf, cj, sj, da);
  };
  for (int tok = blockIdx.x * TPB + (WPT == 1 ? wave : 0); tok < T; tok += gridDim.x * TPB) {
    const e* x = reinterpret_cast<const e*>(x_) + (int64_t)tok * x_st;
    const e* dy = reinterpret_cast<const e*>(dy_) + (int64_t)tok * dy_st_t + 8 * sub;
    e* dx = reinterpret_cast<e*>(dx_) + (int64_t)tok * dx_st;
    float cj[8], sj[8];
    rope_table<D>(cs, tok, sub, -1.f, cj, sj);
    const float r = rstd[tok];
    float dot = 0.f;
    v8 kx[NA], kg[NA];
    row_groups_uniform<NA>(lane, L, per_lane, [&](int a, int i) {
      v8 v, g;
      if (i < nv) {                                         // a lane and its partner are both inside the row or both outside
        v = saved_load<DT>(x + 8 * i); g = *reinterpret_cast<const v8*>(dy + (int64_t)(i >> LSH) * dy_st_h);
        const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
        float da[8];
        unrotate(g, cj, sj, da);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float t = (float)v[j] * r; dot = __builtin_fmaf(da[j] * (float)wv[j], t, dot); acc[a][j] = __builtin_fmaf(da[j], t, acc[a][j]); }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[j] = (e)0.f; g[j] = (e)0.f; }
      }
      kx[a] = v; kg[a] = g;
    });
    dot = token_sum<WPT>(dot, red) / (float)n;
    row_groups_uniform<NA>(lane, L, per_lane, [&](int a, int i) {
      const v8 v = kx[a];
      float da[8];
      unrotate(kg[a], cj, sj, da);
      if (i < nv) {
        const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
        v8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float t = (float)v[j] * r; o[j] = (e)(r * (da[j] * (float)wv[j] - t * dot)); }
        *reinterpret_cast<v8*>(dx + 8 * i) = o;
      }
    });
  }
  if (!dw_part) return;                                       // frozen weight: no partials wanted (block-uniform)
  float* out = dw_part + (int64_t)blockIdx.x * n;
  if constexpr (WPT == 4) {                                   // every lane of the workgroup owns its columns alone
    row_groups<NA>(lane, L, nv, per_lane, [&](int a, int i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) out[8 * i + j] = acc[a][j];
    });
  } else dw_reduce<NA>(acc, red, out, nv, per_lane);
}

// ---------------------------------------------------------------------------------------------
// OLMo's post-norm branch end: yn = cast(w · y · rsqrt(mean(y²)+eps)) - Olmo2RMSNorm multiplies by the weight in fp32 and rounds ONCE, unlike
// the Qwen3 / Llama norm above - kept only when yn_ is given; out = cast(res + yn), one pass.
// The forms of rmsnorm_fwd_kernel: NA > 0 keeps the row in registers, NA == 0 (any H) reads it twice.  The two sweeps stand here and not
// in rms_row_pass: behind it the 16-bit NA 4 instances took 66-68 VGPRs instead of 64 and lost the eighth wave.
// ---------------------------------------------------------------------------------------------
template <int DT, int NA>
__global__ __launch_bounds__(256) void rmsnorm_add_fwd_kernel(const void* __restrict__ y_, const void* __restrict__ w_, const void* __restrict__ res_,
                                                              void* __restrict__ out_, void* __restrict__ yn_, float* __restrict__ rstd,
                                                              int R, int H, float eps) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const e* w = reinterpret_cast<const e*>(w_);
  const int nv = H >> 3;
  for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
    const e* y = reinterpret_cast<const e*>(y_) + (int64_t)row * H;
    const e* res = reinterpret_cast<const e*>(res_) + (int64_t)row * H;
    e* out = reinterpret_cast<e*>(out_) + (int64_t)row * H;
    e* yn = yn_ ? reinterpret_cast<e*>(yn_) + (int64_t)row * H : nullptr;
    float ss = 0.f;
    auto finish = [&](int i, const v8& v, float r) {
      const v8 wv = *reinterpret_cast<const v8*>(w + 8 * i);
      const v8 rv = *reinterpret_cast<const v8*>(res + 8 * i);
      v8 n8, o;
#pragma unroll
      for (int j = 0; j < 8; ++j) { n8[j] = (e)((float)wv[j] * ((float)v[j] * r)); o[j] = (e)((float)rv[j] + (float)n8[j]); }
      if (yn) *reinterpret_cast<v8*>(yn + 8 * i) = n8;
      *reinterpret_cast<v8*>(out + 8 * i) = o;
    };
    if constexpr (NA > 0) {
      v8 keep[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int i = lane + 64 * a;
        if (i < nv) {
          const v8 v = *reinterpret_cast<const v8*>(y + 8 * i);
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; ss = __builtin_fmaf(f, f, ss); }
          keep[a] = v;
        }
      }
      ss = wave_sum(ss);
      const float r = __builtin_amdgcn_rsqf(ss / (float)H + eps);
      if (lane == 0) rstd[row] = r;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        const int i = lane + 64 * a;
        if (i < nv) finish(i, keep[a], r);
      }
    } else {
      for (int i = lane; i < nv; i += 64) {
        const v8 v = *reinterpret_cast<const v8*>(y + 8 * i);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; ss = __builtin_fmaf(f, f, ss); }
      }
      ss = wave_sum(ss);
      const float r = __builtin_amdgcn_rsqf(ss / (float)H + eps);
      if (lane == 0) rstd[row] = r;
      for (int i = lane; i < nv; i += 64) finish(i, *reinterpret_cast<const v8*>(y + 8 * i), r);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// SwiGLU and GeGLU on rows of C columns; gate/up (and their gradients) may live side by side in one fused
// [rows, 2C] GEMM output: `ld` = elements between consecutive rows of g/u (dg/du).  One body per direction over the activation A:
// A::act(g) = the activation, rounded to the storage type before the product with u; A::grad(g, u, dy, du, dg) = both gradients in fp32.
struct Silu {
  static __device__ __forceinline__ float act(float x) { return x / (1.f + __expf(-x)); }
  static __device__ __forceinline__ void grad(float x, float u, float d, float& du, float& dg) {
    const float sg = 1.f / (1.f + __expf(-x));
    du = d * x * sg;
    dg = d * u * sg * (1.f + x * (1.f - sg));
  }
};

// GeGLU (Gemma): y = cast(gelu_tanh(g)) · u with gelu_tanh(g) = 0.5 g (1 + tanh(√(2/π)(g + 0.044715 g³))) - HF's gelu_pytorch_tanh.
// 0.5 (1 + tanh(z)) = sigmoid(2z) = 1 / (1 + e^{-2z}): one exponential and one division, saturating to 0 / 1 for
// large |z| without an inf / inf.  s = that factor: gelu = g s, gelu' = s + g s (1 − s) · 2 dz/dg.
__device__ __forceinline__ float gelu_gate(float x, float* dgelu) {
  constexpr float K0 = 0.7978845608028654f, K1 = 0.044715f;
  const float x2 = x * x;
  const float z2 = 2.f * K0 * x * __builtin_fmaf(K1, x2, 1.f);                   // 2z
  const float E = __expf(fminf(-z2, 80.f));                                     // finite: E s below is never inf * 0
  const float s = 1.f / (1.f + E);                                              // sigmoid(2z) = 0.5 (1 + tanh z), no cancellation at either end
  if (dgelu) *dgelu = s + x * s * (E * s) * (2.f * K0 * __builtin_fmaf(3.f * K1, x2, 1.f));      // 1 - s = E s
  return x * s;
}
struct GeluTanh {
  static __device__ __forceinline__ float act(float x) { return gelu_gate(x, nullptr); }
  static __device__ __forceinline__ void grad(float x, float u, float d, float& du, float& dg) {
    float dgl; const float ge = gelu_gate(x, &dgl);
    du = d * ge;
    dg = d * u * dgl;
  }
};

template <int DT, class A>
__device__ __forceinline__ void glu_fwd_body(const void* g_, const void* u_, void* y_, int64_t n8, int c8, int64_t ld) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / c8; const int col = (int)(i - row * c8) * 8;
    const v8 g = *reinterpret_cast<const v8*>(reinterpret_cast<const e*>(g_) + row * ld + col);
    const v8 u = *reinterpret_cast<const v8*>(reinterpret_cast<const e*>(u_) + row * ld + col);
    v8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const e s = (e)A::act((float)g[j]); o[j] = (e)((float)s * (float)u[j]); }
    reinterpret_cast<v8*>(y_)[i] = o;
  }
}
template <int DT, class A>
__device__ __forceinline__ void glu_bwd_body(const void* g_, const void* u_, const void* dy_, void* dg_, void* du_, int64_t n8, int c8, int64_t ld,
                                             int64_t ldg) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / c8; const int col = (int)(i - row * c8) * 8;
    const v8 g = saved_load<DT>(reinterpret_cast<const e*>(g_) + row * ld + col);
    const v8 u = saved_load<DT>(reinterpret_cast<const e*>(u_) + row * ld + col);
    const v8 dy = reinterpret_cast<const v8*>(dy_)[i];
    v8 dg, du;
#pragma unroll
    for (int j = 0; j < 8; ++j) { float fu, fg; A::grad((float)g[j], (float)u[j], (float)dy[j], fu, fg); du[j] = (e)fu; dg[j] = (e)fg; }
    *reinterpret_cast<v8*>(reinterpret_cast<e*>(dg_) + row * ldg + col) = dg;
    *reinterpret_cast<v8*>(reinterpret_cast<e*>(du_) + row * ldg + col) = du;
  }
}

template <int DT>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const void* __restrict__ g_, const void* __restrict__ u_, void* __restrict__ y_,
                                                         int64_t n8, int c8, int64_t ld) { glu_fwd_body<DT, Silu>(g_, u_, y_, n8, c8, ld); }
template <int DT>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const void* __restrict__ g_, const void* __restrict__ u_, const void* __restrict__ dy_,
                                                         void* __restrict__ dg_, void* __restrict__ du_, int64_t n8, int c8, int64_t ld, int64_t ldg) {
  glu_bwd_body<DT, Silu>(g_, u_, dy_, dg_, du_, n8, c8, ld, ldg);
}
template <int DT>
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const void* __restrict__ g_, const void* __restrict__ u_, void* __restrict__ y_,
                                                        int64_t n8, int c8, int64_t ld) { glu_fwd_body<DT, GeluTanh>(g_, u_, y_, n8, c8, ld); }
template <int DT>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const void* __restrict__ g_, const void* __restrict__ u_, const void* __restrict__ dy_,
                                                        void* __restrict__ dg_, void* __restrict__ du_, int64_t n8, int c8, int64_t ld, int64_t ldg) {
  glu_bwd_body<DT, GeluTanh>(g_, u_, dy_, dg_, du_, n8, c8, ld, ldg);
}

// ---------------------------------------------------------------------------------------------
// 2-D transpose through a 64x64 LDS tile of 32-bit words, 16-byte global accesses on both sides.
//   4-byte elements: word[c][r] = in[r][c].
//   2-byte elements: a lane loads the 8-element chunks of TWO consecutive rows and packs (in[r][c], in[r+1][c]) into one word, so the tile
//   is transposed at word granularity ([c][r/2], 32 words per output row) and the write phase reads 4 consecutive words = 8 output
//   elements with one ds_read_b128.  Row pitch = odd number of words (+1 word of padding x alignment): the column-wise writes of the
//   load phase spread over the banks.
template <int ESZ>
__global__ __launch_bounds__(256) void transpose_kernel(const char* __restrict__ in, char* __restrict__ out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out) {
  constexpr int TS = 64;
  constexpr int WPR = ESZ == 2 ? TS / 2 : TS;         // words per transposed tile row
  constexpr int PITCH = WPR + 4;                      // words; +4 keeps 16-byte alignment of the rows for the b128 reads (2-way conflicts at worst)
  __shared__ __attribute__((aligned(16))) uint32_t tile[TS * PITCH];
  const int64_t r0 = (int64_t)blockIdx.y * TS, c0 = (int64_t)blockIdx.x * TS;
  const int tid = threadIdx.x;
  if (ESZ == 2) {
    // load: 32 row pairs x 8 chunks of 8 columns = 256 items, one per thread
    const int rp = tid >> 3, ch = tid & 7, r = 2 * rp, c = 8 * ch;
    uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
    if (c0 + c < cols) {
      if (r0 + r < rows) a = *reinterpret_cast<const uint4*>(in + ((r0 + r) * ld_in + c0 + c) * 2);
      if (r0 + r + 1 < rows) b = *reinterpret_cast<const uint4*>(in + ((r0 + r + 1) * ld_in + c0 + c) * 2);
    }
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {                     // columns c+2j (low halves) and c+2j+1 (high halves)
      tile[(c + 2 * j) * PITCH + rp] = (aw[j] & 0xffffu) | (bw[j] << 16);
      tile[(c + 2 * j + 1) * PITCH + rp] = (aw[j] >> 16) | (bw[j] & 0xffff0000u);
    }
    __syncthreads();
    // store: 64 output rows (input columns) x 8 chunks of 8 output elements (4 words)
    for (int i = tid; i < TS * 8; i += 256) {
      const int oc = i >> 3, k = i & 7;               // output row oc (= input column), output elements 8k .. 8k+7 (= input rows)
      if (c0 + oc < cols && r0 + 8 * k < rows)
        *reinterpret_cast<uint4*>(out + ((c0 + oc) * ld_out + r0 + 8 * k) * 2) = *reinterpret_cast<const uint4*>(&tile[oc * PITCH + 4 * k]);
    }
  } else {
    for (int i = tid; i < TS * 16; i += 256) {        // 64 rows x 16 chunks of 4 columns
      const int r = i >> 4, c = 4 * (i & 15);
      uint4 a = make_uint4(0, 0, 0, 0);
      if (r0 + r < rows && c0 + c < cols) a = *reinterpret_cast<const uint4*>(in + ((r0 + r) * ld_in + c0 + c) * 4);
      tile[(c + 0) * PITCH + r] = a.x; tile[(c + 1) * PITCH + r] = a.y; tile[(c + 2) * PITCH + r] = a.z; tile[(c + 3) * PITCH + r] = a.w;
    }
    __syncthreads();
    for (int i = tid; i < TS * 16; i += 256) {
      const int oc = i >> 4, k = i & 15;
      if (c0 + oc < cols && r0 + 4 * k < rows)
        *reinterpret_cast<uint4*>(out + ((c0 + oc) * ld_out + r0 + 4 * k) * 4) = *reinterpret_cast<const uint4*>(&tile[oc * PITCH + 4 * k]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// out[i] = cast( sum_s part[s * stride + i]  (+ extra[i]) ),  fp32 sums: the reduction of the per-workgroup weight-gradient partials of
// the norm kernels above (many slabs of H values) and of the split-K weight-gradient GEMM (a few slabs of out*in values), fused with the
// rounding to the parameter dtype.
//   tall form: a workgroup of 16 waves owns 64 columns; wave w sums slabs w, w+16, ... (8 loads in flight), LDS combines the 16.
template <int DT>
__global__ __launch_bounds__(1024) void sum_slabs_tall_kernel(const float* __restrict__ part, int64_t slabs, int64_t n, int64_t stride,
                                                              const float* __restrict__ extra, void* __restrict__ out_) {
  using e = typename Ty<DT>::e;
  __shared__ float red[16 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * 64 + lane;
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.f;
  if (col < n) {
    int64_t s = wave;
    for (; s + 16 * 7 < slabs; s += 16 * 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += part[(s + 16 * u) * stride + col];
    }
    for (; s < slabs; s += 16) acc[0] += part[s * stride + col];
  }
  red[wave * 64 + lane] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (wave == 0 && col < n) {
    float t = extra ? extra[col] : 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w * 64 + lane];
    reinterpret_cast<e*>(out_)[col] = (e)t;
  }
}
//   flat form (slabs <= 16): one output element group of 4 per lane, slabs summed in order.
template <int DT>
__global__ __launch_bounds__(256) void sum_slabs_flat_kernel(const float* __restrict__ part, int slabs, int64_t n4, int64_t stride,
                                                             const float* __restrict__ extra, void* __restrict__ out_) {
  using e = typename Ty<DT>::e;
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef e e4 __attribute__((ext_vector_type(4)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f4 t = extra ? *reinterpret_cast<const f4*>(extra + 4 * i) : f4{0.f, 0.f, 0.f, 0.f};
    for (int s2 = 0; s2 < slabs; ++s2) t += *reinterpret_cast<const f4*>(part + s2 * stride + 4 * i);
    e4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (e)t[j];
    *reinterpret_cast<e4*>(reinterpret_cast<e*>(out_) + 4 * i) = o;
  }
}

template <int N> using Int = std::integral_constant<int, N>;

// The NA ladder of the row kernels: f(NA) with NA = 16-byte groups per lane.  Rows of up to 1 024 / 2 048 / 4 096 elements stay in
// registers between the passes (backward: where that fits, see KEEP); WIDE = the NA of longer rows (0: any H, the row is read twice;
// 16: H <= 8192).
template <int WIDE, class F> inline void na_form(int H, F&& f) {
  if (H <= 1024) f(Int<2>{}); else if (H <= 2048) f(Int<4>{}); else if (H <= 4096) f(Int<8>{}); else f(Int<WIDE>{});
}
// The kernel form of an RMSNorm call, chosen once for both directions: f(NA, OFF).  w_offset == 0 selects the kernels compiled without
// the offset.
template <int WIDE, class F> inline void rms_form(int H, float w_offset, F&& f) {
  if (w_offset != 0.f) na_form<WIDE>(H, [&](auto na) { f(na, std::true_type{}); });
  else na_form<WIDE>(H, [&](auto na) { f(na, std::false_type{}); });
}

// The kernel form of a head-norm / RoPE call: f(HPL, D) with HPL = 4 heads per lane group when NH % 4 == 0, and D = head_dim (64 or 128)
template <class F> inline void qk_form(int NH, int head_dim, F&& f) {
  if (head_dim == 64) { if (NH % 4 == 0) f(Int<4>{}, Int<64>{}); else f(Int<1>{}, Int<64>{}); }
  else if (NH % 4 == 0) f(Int<4>{}, Int<128>{}); else f(Int<1>{}, Int<128>{});
}

// The kernel form of a projection-wide q/k norm + RoPE call: f(NA, D, WPT) for the row of n = NH*D <= 8192 elements - one wave per token
// (WPT 1) with NA = 2 / 4 16-byte groups per lane up to 1 024 / 2 048, the workgroup's four waves on one token (WPT 4) with NA = 2 / 4
// up to 4 096 / 8 192 - and D = head_dim (64 or 128)
template <class F> inline void wide_qk_form(int64_t n, int head_dim, F&& f) {
  auto by_n = [&](auto d) {
    if (n <= 1024) f(Int<2>{}, d, Int<1>{});
    else if (n <= 2048) f(Int<4>{}, d, Int<1>{});
    else if (n <= 4096) f(Int<2>{}, d, Int<4>{});
    else f(Int<4>{}, d, Int<4>{});
  };
  if (head_dim == 64) by_n(Int<64>{}); else by_n(Int<128>{});
}

// SwiGLU and GeGLU: one checked body per direction; kernel_of(DT) is the entry's kernel for the storage type DT
template <class K>
int glu_fwd(const void* gate, const void* up, void* y, int64_t rows, int32_t cols, int64_t ld, int32_t dtype, void* stream, K kernel_of) {
  if (!gate || !up || !y || rows <= 0 || cols <= 0 || ld < cols) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || cols % 8 || ld % 8) return DTA_EUNSUPPORTED;
  if (!all_aligned16(gate, up, y)) return DTA_EALIGN;
  const int64_t n8 = rows * (cols / 8);
  return dta_launch(stream, [&](hipStream_t st) {
    dta_storage_type(dtype, [&](auto dt) {
      hipLaunchKernelGGL(kernel_of(dt), dim3(row_blocks(n8, 256, 4096)), dim3(256), 0, st, gate, up, y, n8, cols / 8, ld);
    });
  });
}

template <class K>
int glu_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup, int64_t rows, int32_t cols, int64_t ld, int64_t ld_grad,
            int32_t dtype, void* stream, K kernel_of) {
  if (!gate || !up || !dy || !dgate || !dup || rows <= 0 || cols <= 0 || ld < cols || ld_grad < cols) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || cols % 8 || ld % 8 || ld_grad % 8) return DTA_EUNSUPPORTED;
  if (!all_aligned16(gate, up, dy, dgate, dup)) return DTA_EALIGN;
  const int64_t n8 = rows * (cols / 8);
  return dta_launch(stream, [&](hipStream_t st) {
    dta_storage_type(dtype, [&](auto dt) {
      hipLaunchKernelGGL(kernel_of(dt), dim3(row_blocks(n8, 256, 4096)), dim3(256), 0, st, gate, up, dy, dgate, dup, n8, cols / 8, ld, ld_grad);
    });
  });
}

}  // namespace

extern "C" int dta_rmsnorm_fwd(const void* x, const void* delta, const void* w, void* x_out, void* y, float* rstd,
                               int32_t R, int32_t H, float eps, float w_offset, int32_t dtype, void* stream) {
  if (!x || !w || !y || !rstd || R <= 0 || H <= 0 || ((delta != nullptr) != (x_out != nullptr)) || w_offset != w_offset) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || H % 8) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, w, y, delta, x_out)) return DTA_EALIGN;
  const dim3 grid(row_blocks(R, 4, 8192)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    rms_form<0>(H, w_offset, [&](auto na, auto off) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((rmsnorm_fwd_kernel<decltype(dt)::value, decltype(na)::value, decltype(off)::value>), grid, block, 0, st,
                           x, delta, w, x_out, y, rstd, R, H, eps, w_offset);
      });
    });
  });
}

/* dw_partial: float [dta_rmsnorm_bwd_blocks(R), H]; the caller sums it over dim 0.  NULL: the weight needs no gradient, dx only. */
extern "C" int dta_rmsnorm_bwd_blocks(int32_t R) { return row_blocks(R, 4, 2048); }
extern "C" int dta_rmsnorm_bwd(const void* x, const void* w, const void* dy, const void* dres, const float* rstd, void* dx, float* dw_partial,
                               int32_t R, int32_t H, float w_offset, int32_t dtype, void* stream) {
  if (!x || !w || !dy || !rstd || !dx || R <= 0 || H <= 0 || w_offset != w_offset) return DTA_EINVAL;          // dw_partial NULL: dx only (frozen weight)
  if (!row_dtype_ok(dtype) || H % 8 || H > 8192) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, w, dy, dx, dres)) return DTA_EALIGN;
  const dim3 grid(row_blocks(R, 4, 2048)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    rms_form<16>(H, w_offset, [&](auto na, auto off) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<decltype(dt)::value, decltype(na)::value, decltype(off)::value>), grid, block, 0, st,
                           x, w, dy, dres, rstd, dx, dw_partial, R, H, w_offset);
      });
    });
  });
}

extern "C" int dta_layernorm_fwd(const void* x, const void* delta_a, const void* delta_b, const void* w, void* x_out, void* y,
                                 float* mean, float* rstd, int32_t R, int32_t H, float eps, int32_t dtype, void* stream) {
  if (!x || !w || !y || !mean || !rstd || R <= 0 || H <= 0 || (delta_b && !delta_a) || ((delta_a != nullptr) != (x_out != nullptr)) || eps != eps)
    return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || H % 8 || H > 8192) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, w, y, delta_a, x_out, delta_b)) return DTA_EALIGN;
  const dim3 grid(row_blocks(R, 4, 8192)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    na_form<16>(H, [&](auto na) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((layernorm_fwd_kernel<decltype(dt)::value, decltype(na)::value>), grid, block, 0, st,
                           x, delta_a, delta_b, w, x_out, y, mean, rstd, R, H, eps);
      });
    });
  });
}

/* dw_partial: float [dta_layernorm_bwd_blocks(R), H]; the caller sums it over dim 0.  NULL: the weight needs no gradient, dx only. */
extern "C" int dta_layernorm_bwd_blocks(int32_t R) { return row_blocks(R, 4, 2048); }
extern "C" int dta_layernorm_bwd(const void* x, const void* w, const void* dy, const void* dres, const float* mean, const float* rstd,
                                 void* dx, float* dw_partial, int32_t R, int32_t H, int32_t dtype, void* stream) {
  if (!x || !w || !dy || !mean || !rstd || !dx || R <= 0 || H <= 0) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || H % 8 || H > 8192) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, w, dy, dx, dres)) return DTA_EALIGN;
  const dim3 grid(row_blocks(R, 4, 2048)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    na_form<16>(H, [&](auto na) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((layernorm_bwd_kernel<decltype(dt)::value, decltype(na)::value>), grid, block, 0, st,
                           x, w, dy, dres, mean, rstd, dx, dw_partial, R, H);
      });
    });
  });
}

extern "C" int dta_qk_norm_rope_fwd(const void* x, const void* w, const float* cos_sin, void* y, float* rstd,
                                    int32_t T, int32_t NH, int32_t head_dim, int64_t x_stride_t, float eps, int32_t dtype, void* stream) {
  if (!x || !cos_sin || !y || T <= 0 || NH <= 0 || (w && !rstd)) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || (head_dim != 128 && head_dim != 64)) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, y, w) || x_stride_t % 8) return DTA_EALIGN;
  return dta_launch(stream, [&](hipStream_t st) {
    qk_form(NH, head_dim, [&](auto hpl, auto d) {
      constexpr int HPL = decltype(hpl)::value, D = decltype(d)::value, UPB = 4 * (64 / (D / 8));       // (token, head group) units per workgroup
      const int64_t n = (int64_t)T * (NH / HPL);
      const dim3 grid((unsigned)((n + UPB - 1) / UPB)), block(256);
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((qk_norm_rope_fwd_kernel<decltype(dt)::value, HPL, D>), grid, block, 0, st, x, w, cos_sin, y, rstd, n, NH, x_stride_t, eps);
      });
    });
  });
}

/* dw_partial: float [dta_qk_norm_rope_bwd_blocks(T*NH), head_dim] (ignored when w == NULL); the row count does not depend on head_dim. */
extern "C" int dta_qk_norm_rope_bwd_blocks(int64_t n_heads_total) { return row_blocks(n_heads_total, 16, 1024); }
extern "C" int dta_qk_norm_rope_bwd(const void* x, const void* w, const float* cos_sin, const void* dy, const float* rstd,
                                    void* dx, float* dw_partial, int32_t T, int32_t NH, int32_t head_dim,
                                    int64_t x_stride_t, int64_t dy_stride_t, int64_t dy_stride_h, int64_t dx_stride_t, int32_t dtype, void* stream) {
  if (!cos_sin || !dy || !dx || T <= 0 || NH <= 0 || (w && (!x || !rstd))) return DTA_EINVAL;     // w with dw_partial NULL: dx only
  if (!row_dtype_ok(dtype) || (head_dim != 128 && head_dim != 64)) return DTA_EUNSUPPORTED;
  if (!all_aligned16(dy, dx, w, w ? x : nullptr) || x_stride_t % 8 || dy_stride_t % 8 || dy_stride_h % 8 || dx_stride_t % 8) return DTA_EALIGN;
  if (dx_stride_t < (int64_t)NH * head_dim) return DTA_EINVAL;
  // the grid - and with it the number of dw_partial rows the caller sized from dta_qk_norm_rope_bwd_blocks(T*NH) - depends on neither HPL nor
  // head_dim (the grid-stride loop covers any unit count; a D = 64 workgroup takes 32 units per pass instead of 16)
  const dim3 grid(row_blocks((int64_t)T * NH, 16, 1024)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    qk_form(NH, head_dim, [&](auto hpl, auto d) {
      constexpr int HPL = decltype(hpl)::value, D = decltype(d)::value;
      const int64_t n = (int64_t)T * (NH / HPL);
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((qk_norm_rope_bwd_kernel<decltype(dt)::value, HPL, D>), grid, block, 0, st, x, w, cos_sin, dy, rstd, dx, dw_partial, n, NH,
                           x_stride_t, dy_stride_t, dy_stride_h, dx_stride_t);
      });
    });
  });
}

namespace {
// the checks both dta_rope_partial_* entries share, in the header's order, and the launch: `grid_cap` 0 = one pass over every unit
int rope_partial(const void* in, const float* cos_sin, void* out, int32_t T, int32_t NH, int32_t head_dim, int32_t rotary_dim, int32_t pairing,
                 int64_t in_st_t, int64_t in_st_h, int64_t out_st_t, float sgn, int grid_cap, int32_t dtype, void* stream) {
  if (!in || !cos_sin || !out || T <= 0 || NH <= 0 || rotary_dim <= 0 || (pairing != 0 && pairing != 1)) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || (head_dim != 128 && head_dim != 64) || rotary_dim > head_dim || rotary_dim % (pairing == 0 ? 16 : 8)) return DTA_EUNSUPPORTED;
  if (!all_aligned16(in, out, cos_sin) || in_st_t % 8 || in_st_h % 8 || out_st_t % 8) return DTA_EALIGN;
  if (in_st_t < 0 || in_st_h < head_dim || out_st_t < (int64_t)NH * head_dim) return DTA_EINVAL;
  return dta_launch(stream, [&](hipStream_t st) {
    qk_form(NH, head_dim, [&](auto hpl, auto d) {
      constexpr int HPL = decltype(hpl)::value, D = decltype(d)::value, UPB = 4 * (64 / (D / 8));
      const int64_t n = (int64_t)T * (NH / HPL);
      const dim3 grid(grid_cap ? (unsigned)row_blocks((int64_t)T * NH, 16, grid_cap) : ceil_blocks(n, UPB)), block(256);
      auto launch = [&](auto dt, auto pair, auto one_pass) {
        hipLaunchKernelGGL((rope_partial_kernel<decltype(dt)::value, HPL, D, decltype(pair)::value, decltype(one_pass)::value>), grid, block, 0, st,
                           in, cos_sin, out, n, NH, rotary_dim, in_st_t, in_st_h, out_st_t, sgn);
      };
      dta_storage_type(dtype, [&](auto dt) {
        if (grid_cap) { if (pairing == 0) launch(dt, Int<0>{}, std::false_type{}); else launch(dt, Int<1>{}, std::false_type{}); }
        else if (pairing == 0) launch(dt, Int<0>{}, std::true_type{}); else launch(dt, Int<1>{}, std::true_type{});
      });
    });
  });
}
}  // namespace

extern "C" int dta_rope_partial_fwd(const void* x, const float* cos_sin, void* y, int32_t T, int32_t NH, int32_t head_dim, int32_t rotary_dim,
                                    int32_t pairing, int64_t x_stride_t, int32_t dtype, void* stream) {
  return rope_partial(x, cos_sin, y, T, NH, head_dim, rotary_dim, pairing, x_stride_t, head_dim, (int64_t)NH * head_dim, 1.f, 0, dtype, stream);
}

// the rotation by the negative angle; the grid-stride form of dta_qk_norm_rope_bwd (the same workgroup count)
extern "C" int dta_rope_partial_bwd(const float* cos_sin, const void* dy, void* dx, int32_t T, int32_t NH, int32_t head_dim, int32_t rotary_dim,
                                    int32_t pairing, int64_t dy_stride_t, int64_t dy_stride_h, int64_t dx_stride_t, int32_t dtype, void* stream) {
  return rope_partial(dy, cos_sin, dx, T, NH, head_dim, rotary_dim, pairing, dy_stride_t, dy_stride_h, dx_stride_t, -1.f, 1024, dtype, stream);
}

extern "C" int dta_wide_qk_norm_rope_fwd(const void* x, const void* w, const float* cos_sin, void* y, float* rstd,
                                         int32_t T, int32_t NH, int32_t head_dim, int64_t x_stride_t, float eps, int32_t dtype, void* stream) {
  if (!x || !w || !cos_sin || !y || !rstd || T <= 0 || NH <= 0 || eps != eps) return DTA_EINVAL;
  if (!row_dtype_ok(dtype) || (head_dim != 128 && head_dim != 64) || (int64_t)NH * head_dim > 8192) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, w, y) || x_stride_t % 8) return DTA_EALIGN;
  const int n = NH * head_dim;
  if (x_stride_t < n) return DTA_EINVAL;
  const dim3 grid(row_blocks(T, 4, 8192)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    wide_qk_form(n, head_dim, [&](auto na, auto d, auto wpt) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((wide_qk_norm_rope_fwd_kernel<decltype(dt)::value, decltype(na)::value, decltype(d)::value, decltype(wpt)::value>), grid, block, 0, st,
                           x, w, cos_sin, y, rstd, T, n, x_stride_t, eps);
      });
    });
  });
}

/* dw_partial: float [dta_wide_qk_norm_rope_bwd_blocks(T), NH*head_dim]; the caller sums it over dim 0 (dta_sum_slabs).  NULL: dx only. */
extern "C" int dta_wide_qk_norm_rope_bwd_blocks(int32_t T) { return row_blocks(T, 4, 2048); }
extern "C" int dta_wide_qk_norm_rope_bwd(const void* x, const void* w, const float* cos_sin, const void* dy, const float* rstd,
                                         void* dx, float* dw_partial, int32_t T, int32_t NH, int32_t head_dim,
                                         int64_t x_stride_t, int64_t dy_stride_t, int64_t dy_stride_h, int64_t dx_stride_t, int32_t dtype, void* stream) {
  if (!x || !w || !cos_sin || !dy || !rstd || !dx || T <= 0 || NH <= 0) return DTA_EINVAL;       // dw_partial NULL: dx only (frozen weight)
  if (!row_dtype_ok(dtype) || (head_dim != 128 && head_dim != 64) || (int64_t)NH * head_dim > 8192) return DTA_EUNSUPPORTED;
  if (!all_aligned16(x, w, dy, dx) || x_stride_t % 8 || dy_stride_t % 8 || dy_stride_h % 8 || dx_stride_t % 8) return DTA_EALIGN;
  const int n = NH * head_dim;
  if (x_stride_t < n || dx_stride_t < n) return DTA_EINVAL;
  const dim3 grid(row_blocks(T, 4, 2048)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    wide_qk_form(n, head_dim, [&](auto na, auto d, auto wpt) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((wide_qk_norm_rope_bwd_kernel<decltype(dt)::value, decltype(na)::value, decltype(d)::value, decltype(wpt)::value>), grid, block, 0, st,
                           x, w, cos_sin, dy, rstd, dx, dw_partial, T, n, x_stride_t, dy_stride_t, dy_stride_h, dx_stride_t);
      });
    });
  });
}

extern "C" int dta_rmsnorm_add_fwd(const void* y, const void* w, const void* res, void* out, void* yn, float* rstd,
                                   int32_t R, int32_t H, float eps, int32_t dtype, void* stream) {
  if (!y || !w || !res || !out || !rstd || R <= 0 || H <= 0 || eps != eps) return DTA_EINVAL;           // yn NULL: only out is wanted
  if (!row_dtype_ok(dtype) || H % 8) return DTA_EUNSUPPORTED;
  if (!all_aligned16(y, w, res, out, yn)) return DTA_EALIGN;
  const dim3 grid(row_blocks(R, 4, 8192)), block(256);
  return dta_launch(stream, [&](hipStream_t st) {
    na_form<0>(H, [&](auto na) {
      dta_storage_type(dtype, [&](auto dt) {
        hipLaunchKernelGGL((rmsnorm_add_fwd_kernel<decltype(dt)::value, decltype(na)::value>), grid, block, 0, st, y, w, res, out, yn, rstd, R, H, eps);
      });
    });
  });
}

extern "C" int dta_swiglu_fwd(const void* gate, const void* up, void* y, int64_t rows, int32_t cols, int64_t ld, int32_t dtype, void* stream) {
  return glu_fwd(gate, up, y, rows, cols, ld, dtype, stream, [](auto dt) { return swiglu_fwd_kernel<decltype(dt)::value>; });
}
extern "C" int dta_geglu_fwd(const void* gate, const void* up, void* y, int64_t rows, int32_t cols, int64_t ld, int32_t dtype, void* stream) {
  return glu_fwd(gate, up, y, rows, cols, ld, dtype, stream, [](auto dt) { return geglu_fwd_kernel<decltype(dt)::value>; });
}
extern "C" int dta_geglu_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup,
                             int64_t rows, int32_t cols, int64_t ld, int64_t ld_grad, int32_t dtype, void* stream) {
  return glu_bwd(gate, up, dy, dgate, dup, rows, cols, ld, ld_grad, dtype, stream, [](auto dt) { return geglu_bwd_kernel<decltype(dt)::value>; });
}
extern "C" int dta_swiglu_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup,
                              int64_t rows, int32_t cols, int64_t ld, int64_t ld_grad, int32_t dtype, void* stream) {
  return glu_bwd(gate, up, dy, dgate, dup, rows, cols, ld, ld_grad, dtype, stream, [](auto dt) { return swiglu_bwd_kernel<decltype(dt)::value>; });
}

extern "C" int dta_transpose(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, int32_t elem_size, void* stream) {
  if (!in || !out || rows <= 0 || cols <= 0 || ld_in < cols || ld_out < rows) return DTA_EINVAL;
  if (elem_size != 2 && elem_size != 4) return DTA_EUNSUPPORTED;
  const int V = 16 / elem_size;
  if (rows % V || cols % V || ld_in % V || ld_out % V) return DTA_EUNSUPPORTED;
  if (!aligned16(in) || !aligned16(out)) return DTA_EALIGN;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64)), block(256);
  if (grid.y > 65535) return DTA_EUNSUPPORTED;
  if (elem_size == 2) hipLaunchKernelGGL(transpose_kernel<2>, grid, block, 0, st_, (const char*)in, (char*)out, rows, cols, ld_in, ld_out);
  else hipLaunchKernelGGL(transpose_kernel<4>, grid, block, 0, st_, (const char*)in, (char*)out, rows, cols, ld_in, ld_out);
  return DTA_LAUNCH_STATUS();
}

extern "C" int dta_sum_slabs(const float* part, int64_t slabs, int64_t n, int64_t slab_stride, const float* extra, void* out, int32_t out_dtype,
                             void* stream) {
  if (!part || !out || slabs <= 0 || n <= 0 || slab_stride < n) return DTA_EINVAL;
  if (!row_dtype_ok(out_dtype)) return DTA_EUNSUPPORTED;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  const bool flat = slabs <= 16 && n % 4 == 0 && slab_stride % 4 == 0 && aligned16(part) && aligned16(out) && (!extra || aligned16(extra));
  if (flat) {
    const dim3 grid(row_blocks(n / 4, 256, 8192)), block(256);
    dta_storage_type(out_dtype, [&](auto dt) {
      hipLaunchKernelGGL(sum_slabs_flat_kernel<decltype(dt)::value>, grid, block, 0, st_, part, (int)slabs, n / 4, slab_stride, extra, out);
    });
  } else {
    if ((n + 63) / 64 > 0x7fffffff) return DTA_EUNSUPPORTED;
    const dim3 grid((unsigned)((n + 63) / 64)), block(1024);
    dta_storage_type(out_dtype, [&](auto dt) {
      hipLaunchKernelGGL(sum_slabs_tall_kernel<decltype(dt)::value>, grid, block, 0, st_, part, slabs, n, slab_stride, extra, out);
    });
  }
  return DTA_LAUNCH_STATUS();
}
