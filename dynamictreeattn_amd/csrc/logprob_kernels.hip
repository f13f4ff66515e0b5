// Fused log-softmax statistics over vocabulary rows for gfx950 — HBM-bound, one pass per direction.
//   fwd: per row r of logits[R, V] (bf16 / f16 / f32): lse[r] = ln Σ exp(x/T), ent[r] = lse − Σ p·x/T,
//        lp[r] = x[label[r]]/T − lse[r]                       (vocab_parallel.py:13-27 arithmetic, fp32)
//        and, for every EXTRA label e of the row (CSR extra_ptr/extra_labels: a fork node of the trie predicts one token per
//        child, tree_training_engine.py:205-209, 217-220, 369-372), extra_lp[e] = x[extra_labels[e]]/T − lse[r].
//   bwd: dLoss/dlogits, written to `out` (out == logits: in place):
//        g[r,j] = ( p_j·(−G[r] + ge[r]·(lse[r] − ent[r] − x_j/T)) + Σ_{picked j} g_picked ) / T
//        where G[r] = glp[r] + Σ_e g_extra_lp[e] is the summed gradient of every log-prob picked from row r.
// Masked columns (CAP = false): x = -inf, or x·log2(e)/T below MASKED_Y, has p = 0, adds nothing to (m, s, t) and gets a gradient of exactly 0:
// the factor p is multiplied by - the scaled logit in the forward, the raw one in the backward - is held at MASKED_Y (one v_max per element),
// so that p = 0 always meets a FINITE factor (0·inf was NaN in t = Σ p·y and in p·(c1 + c2·x)); p itself is taken of the raw value, so a NaN
// logit still yields NaN.  A pick of a -inf column is -inf.  A row of masked columns only is undefined.
// One 256-thread workgroup per row, 16-byte loads, online (max, Σexp, Σexp·x) per lane, block reduce.
// Algorithmic HBM bytes: fwd V·sizeof(e) per row (one read); bwd 2·V·sizeof(e) per row (one read, one write).
// Final-logit soft-capping (softcap > 0, CAP = true): every statistic and pick is taken on x' = c·tanh(x/c), formed in registers as the
// raw logit is loaded (no second pass over the logits); the temperature divides x'.  The backward multiplies the gradient with respect to x'
// by 1 − tanh²(x/c) before the store.  The CAP = false kernels keep their arguments and code.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "dta_common.h"
#include "dta_device.h"

// The [rows, V] logits are 8.6 GB at the bench's shape: each byte is read once here (and once more by the gradient GEMMs, long after it
// has left every cache).  Default: non-temporal accesses (no cache allocation) - forward 1.389 -> 1.240 ms (6.9 TB/s), backward 3.36 -> 3.31 ms at
// [28 160, 151 936] bf16; -DDTA_LOGPROB_NT=0: plain.
// The masked-column v_max (one VALU per element, plain form only): scripts/head_stage_probe.py, kept variant at this shape (the whole stage:
// logits GEMM + forward / backward + dgrad + wgrad GEMMs), two runs each: forward 8.887, 9.023 ms before -> 8.830, 8.822 ms after; backward
// 19.954, 20.039 ms before -> 20.057, 19.943 ms after - inside the spread of the two runs before (0.14 / 0.09 ms around 8.955 / 19.996 ms).
#ifndef DTA_LOGPROB_NT
#define DTA_LOGPROB_NT 1
#endif
#if DTA_LOGPROB_NT
#define DTA_LP_LOAD(P) __builtin_nontemporal_load(P)
#define DTA_LP_STORE(P, V) __builtin_nontemporal_store(V, P)
#else
#define DTA_LP_LOAD(P) (*(P))
#define DTA_LP_STORE(P, V) (*(P) = (V))
#endif

namespace {

constexpr float MASKED_Y = -1e30f;   // plain form: the factor that meets p (the scaled logit in fwd, the raw one in bwd) is held at this value
struct Stat { float m, s, t; };   // running max (log2 domain of scaled x), Σ 2^(y−m), Σ 2^(y−m)·y   with y = x·LOG2E/T

__device__ __forceinline__ Stat merge(Stat a, Stat b) {
  const float m = fmaxf(a.m, b.m);
  const float fa = __builtin_amdgcn_exp2f(a.m - m), fb = __builtin_amdgcn_exp2f(b.m - m);
  return Stat{m, a.s * fa + b.s * fb, a.t * fa + b.t * fb};
}

__device__ __forceinline__ Stat block_reduce(Stat v, Stat* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Stat w{__shfl_xor(v.m, o), __shfl_xor(v.s, o), __shfl_xor(v.t, o)};
    v = merge(v, w);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  Stat r = sh[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = merge(r, sh[w]);
  return r;
}

struct FwdArgs {
  const void* logits; const int64_t* labels; const int32_t* extra_ptr; const int64_t* extra_labels;
  float *lse, *ent, *lp, *extra_lp, *stats;
  int R, V; int64_t stride; float inv_temp;
};
struct FwdArgsC : FwdArgs { float softcap; };

template <int DT, bool CAP>
__global__ __launch_bounds__(256) void logprob_entropy_fwd_kernel(typename std::conditional<CAP, FwdArgsC, FwdArgs>::type a) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  __shared__ Stat sh[4];
  const int row = blockIdx.x, V = a.V;
  const e* x = reinterpret_cast<const e*>(a.logits) + (int64_t)row * a.stride;
  float k = LOG2E * a.inv_temp;
  [[maybe_unused]] float kt = 0.f, cs = 1.f;          // CAP: tanh argument factor 2 log2(e) / c; picks are c·t·(1/T)
  if constexpr (CAP) { kt = 2.f * LOG2E / a.softcap; cs = a.softcap; k *= a.softcap; }
  auto capped = [&](float xr) -> float { if constexpr (CAP) return cap_tanh(xr * kt); else return xr; };   // x (no cap) or t = tanh(x/c)
  // the factor of p in t = Σ p·y; plain form: held at MASKED_Y, so that a masked column (y = -inf: p = 0) adds 0·finite = 0, never 0·inf.  p itself
  // is taken of the raw y: a NaN logit still poisons s (fmaxf alone would swallow it)
  auto finite = [&](float y) -> float { if constexpr (CAP) return y; else return fmaxf(y, MASKED_Y); };
  Stat st{-1e30f, 0.f, 0.f};
  const int nv = V >> 3;
  for (int i = threadIdx.x; i < nv; i += 256) {
    const v8 v = DTA_LP_LOAD(reinterpret_cast<const v8*>(x + 8 * i));
    float y[8]; float mx = -1e30f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { y[j] = capped((float)v[j]) * k; mx = fmaxf(mx, y[j]); }
    const float m = fmaxf(st.m, mx);
    const float f = __builtin_amdgcn_exp2f(st.m - m);
    float s = st.s * f, t = st.t * f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float p = __builtin_amdgcn_exp2f(y[j] - m); s += p; t = __builtin_fmaf(p, finite(y[j]), t); }
    st = Stat{m, s, t};
  }
  for (int i = (nv << 3) + threadIdx.x; i < V; i += 256) {            // tail when V % 8 != 0
    const float y = capped((float)x[i]) * k;
    const float m = fmaxf(st.m, y); const float f = __builtin_amdgcn_exp2f(st.m - m); const float p = __builtin_amdgcn_exp2f(y - m);
    st = Stat{m, st.s * f + p, __builtin_fmaf(p, finite(y), st.t * f)};
  }
  st = block_reduce(st, sh);
  const int e0 = a.extra_ptr ? a.extra_ptr[row] : 0, e1 = a.extra_ptr ? a.extra_ptr[row + 1] : 0;
  auto pick = [&](int64_t lab) -> float { if constexpr (CAP) return cs * capped((float)x[lab]) * a.inv_temp; else return (float)x[lab] * a.inv_temp; };
  if (a.stats) {
    // vocab-sharded use: raw per-shard statistics (log2 domain of the scaled logits) for a cross-rank combine; picked
    // values are the raw x/T of the labels this shard owns (0 otherwise)
    if (threadIdx.x == 0) {
      const int64_t lab = a.labels ? a.labels[row] : -1;
      a.stats[4 * row] = st.m; a.stats[4 * row + 1] = st.s; a.stats[4 * row + 2] = st.t;
      a.stats[4 * row + 3] = (lab >= 0 && lab < V) ? pick(lab) : 0.f;
    }
    for (int f = e0 + threadIdx.x; f < e1; f += 256) { const int64_t lab = a.extra_labels[f]; a.extra_lp[f] = (lab >= 0 && lab < V) ? pick(lab) : 0.f; }
  } else {
    const float l = (st.m + __builtin_amdgcn_logf(st.s)) * LN2;          // v_log_f32 = log2
    if (threadIdx.x == 0) {
      a.lse[row] = l;
      if (a.ent) a.ent[row] = l - (st.t / st.s) * LN2;                    // H = lse − E[x/T]
      if (a.lp) { const int64_t lab = a.labels[row]; a.lp[row] = (lab >= 0 && lab < V) ? pick(lab) - l : 0.f; }
    }
    for (int f = e0 + threadIdx.x; f < e1; f += 256) { const int64_t lab = a.extra_labels[f]; a.extra_lp[f] = (lab >= 0 && lab < V) ? pick(lab) - l : 0.f; }
  }
}

struct BwdArgs {
  const void* logits; void* out; const int64_t* labels; const int32_t* extra_ptr; const int64_t* extra_labels;
  const float *lse, *ent, *glp, *gextra, *gent;
  int R, V; int64_t stride, out_stride; float inv_temp;
};
struct BwdArgsC : BwdArgs { float softcap; };
constexpr int CAP_STASH = 2048;      // extra picks of ONE row whose 1 − tanh² factors are held in LDS across the in-place sweep (dta.h)

template <int DT, bool CAP>
__global__ __launch_bounds__(256) void logprob_entropy_bwd_kernel(typename std::conditional<CAP, BwdArgsC, BwdArgs>::type b) {
  using e = typename Ty<DT>::e; using v8 = typename Ty<DT>::v8;
  float* stash = nullptr;
  if constexpr (CAP) { __shared__ float stash_s[CAP_STASH]; stash = stash_s; }
  const int row = blockIdx.x, V = b.V;
  const e* x = reinterpret_cast<const e*>(b.logits) + (int64_t)row * b.stride;
  e* o = reinterpret_cast<e*>(b.out) + (int64_t)row * b.out_stride;
  const float inv_temp = b.inv_temp;
  const float l = b.lse[row];
  const float ge = b.gent ? b.gent[row] : 0.f;
  const float g1 = b.glp ? b.glp[row] : 0.f;
  const int e0 = b.extra_ptr ? b.extra_ptr[row] : 0, e1 = b.extra_ptr ? b.extra_ptr[row + 1] : 0;
  float G = g1;
  for (int f = e0; f < e1; ++f) G += b.gextra[f];                    // a handful per fork row, none elsewhere (uniform loop)
  const float a = -G + ge * (l - (b.ent ? b.ent[row] : 0.f));
  const int64_t lab = b.labels ? b.labels[row] : -1;
  float k = LOG2E * inv_temp; const float l2 = l * LOG2E;
  const int nv = V >> 3;
  [[maybe_unused]] float kt = 0.f, cs = 1.f;
  if constexpr (CAP) {
    kt = 2.f * LOG2E / b.softcap; cs = b.softcap; k *= b.softcap;
    // the one-hot terms of the extra picks need 1 − tanh²(x/c) of their own raw logit, which the in-place sweep below overwrites: taken now
    for (int f = e0 + threadIdx.x; f < e1 && f - e0 < CAP_STASH; f += 256) {
      const int64_t le = b.extra_labels[f];
      float w = 0.f;
      if (le >= 0 && le < V) { const float t = cap_tanh((float)x[le] * kt); w = __builtin_fmaf(-t, t, 1.f); }
      stash[f - e0] = w;
    }
    __syncthreads();
  }
  // d/dx = (p * (a - ge * x/T) + [label] g1) / T  =  p * (c1 + c2 * x) + [label] g1 / T: two instructions per element besides the exponential's two,
  // and the label test once per 16-byte group (it was a compare and a select per element)
  float c2 = -ge * inv_temp * inv_temp;
  if constexpr (CAP) c2 *= cs;                                        // x'/T = c·t/T
  const float c1 = a * inv_temp, gl = g1 * inv_temp;
  const int lab8 = lab >= 0 && lab < ((int64_t)nv << 3) ? (int)(lab >> 3) : -1, labj = (int)(lab & 7);
  for (int i = threadIdx.x; i < nv; i += 256) {
    v8 v = DTA_LP_LOAD(reinterpret_cast<const v8*>(x + 8 * i));
    float g[8];
    [[maybe_unused]] float sech2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xf = (float)v[j];
      if constexpr (CAP) { xf = cap_tanh(xf * kt); sech2[j] = __builtin_fmaf(-xf, xf, 1.f); }      // xf := t; k and c2 carry the cap
      const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(xf, k, -l2));
      if constexpr (!CAP) xf = fmaxf(xf, MASKED_Y);                     // masked column: p = 0 times a FINITE factor = exactly 0
      g[j] = p * __builtin_fmaf(xf, c2, c1);
    }
    if (i == lab8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] += j == labj ? gl : 0.f;
    }
    if constexpr (CAP) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] *= sech2[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (e)g[j];
    DTA_LP_STORE(reinterpret_cast<v8*>(o + 8 * i), v);
  }
  for (int i = (nv << 3) + threadIdx.x; i < V; i += 256) {
    float xr = (float)x[i], s2 = 1.f;
    if constexpr (CAP) { xr = cap_tanh(xr * kt); s2 = __builtin_fmaf(-xr, xr, 1.f); }
    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(xr, k, -l2));
    if constexpr (!CAP) xr = fmaxf(xr, MASKED_Y);
    const float xs = xr * cs * inv_temp;
    float g = p * (a - ge * xs);
    if (i == lab) g += g1;
    if constexpr (CAP) g *= s2;
    o[i] = (e)(g * inv_temp);
  }
  if (e1 > e0) {                                                      // one-hot terms of the extra picks (distinct tokens: children of one node)
    __syncthreads();
    for (int f = e0 + threadIdx.x; f < e1; f += 256) {
      const int64_t le = b.extra_labels[f];
      if constexpr (CAP) {
        // beyond the stash only an out-of-place call still has the raw logit; in place (dta.h: at most CAP_STASH extra picks per row) the
        // pick's gradient element becomes NaN - never a silently dropped term
        float w = __builtin_nanf("");
        if (f - e0 < CAP_STASH) w = stash[f - e0];
        else if (le >= 0 && le < V && (const void*)x != (const void*)o) { const float t = cap_tanh((float)x[le] * kt); w = __builtin_fmaf(-t, t, 1.f); }
        if (le >= 0 && le < V) o[le] = (e)((float)o[le] + b.gextra[f] * inv_temp * w);
      } else
      if (le >= 0 && le < V) o[le] = (e)((float)o[le] + b.gextra[f] * inv_temp);
    }
  }
}

// Final-logit soft-capping: softcap <= 0 selects the kernels compiled without the cap; a cap that is not finite is refused.
bool cap_ok(float c) { return c == c && c < 3.0e38f; }

int fwd_launch(FwdArgsC a, int32_t dtype, float temperature, void* stream) {
  if (!a.logits || a.R <= 0 || a.V <= 0 || (a.lp && !a.labels) || !(temperature > 0.f) || !cap_ok(a.softcap)) return DTA_EINVAL;
  if (a.extra_ptr && (!a.extra_labels || !a.extra_lp)) return DTA_EINVAL;
  if (!row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(a.logits) & (dtype == DTA_F32 ? 31 : 15)) || (a.stride % 8)) return DTA_EALIGN;   // 8-element vector loads
  a.inv_temp = 1.f / temperature;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  auto launch = [&](auto cap) {                              // the CAP = false kernels take the FwdArgs part of `a`
    dta_storage_type(dtype, [&](auto dt) {
      hipLaunchKernelGGL((logprob_entropy_fwd_kernel<decltype(dt)::value, decltype(cap)::value>), dim3(a.R), dim3(256), 0, st, a);
    });
  };
  if (a.softcap > 0.f) launch(std::true_type{}); else launch(std::false_type{});
  return DTA_LAUNCH_STATUS();
}

int bwd_launch(BwdArgsC b, int32_t dtype, float temperature, void* stream) {
  if (!b.logits || !b.out || !b.lse || b.R <= 0 || b.V <= 0 || (b.gent && !b.ent) || (b.glp && !b.labels) || !(temperature > 0.f) ||
      !cap_ok(b.softcap)) return DTA_EINVAL;
  if (b.extra_ptr && (!b.extra_labels || !b.gextra)) return DTA_EINVAL;
  if (!row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  const uintptr_t am = dtype == DTA_F32 ? 31 : 15;
  if ((reinterpret_cast<uintptr_t>(b.logits) & am) || (reinterpret_cast<uintptr_t>(b.out) & am) || (b.stride % 8) || (b.out_stride % 8)) return DTA_EALIGN;
  b.inv_temp = 1.f / temperature;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  auto launch = [&](auto cap) {
    dta_storage_type(dtype, [&](auto dt) {
      hipLaunchKernelGGL((logprob_entropy_bwd_kernel<decltype(dt)::value, decltype(cap)::value>), dim3(b.R), dim3(256), 0, st, b);
    });
  };
  if (b.softcap > 0.f) launch(std::true_type{}); else launch(std::false_type{});
  return DTA_LAUNCH_STATUS();
}

}  // namespace

extern "C" int dta_logprob_entropy_fwd(const void* logits, const int64_t* labels, const int32_t* extra_ptr, const int64_t* extra_labels,
                                       float* lse, float* entropy, float* logprob, float* extra_logprob,
                                       int32_t R, int32_t V, int64_t row_stride, float temperature, int32_t dtype, float softcap, void* stream) {
  if (!lse) return DTA_EINVAL;
  return fwd_launch({{logits, labels, extra_ptr, extra_labels, lse, entropy, logprob, extra_logprob, nullptr, R, V, row_stride, 1.f}, softcap},
                    dtype, temperature, stream);
}

extern "C" int dta_logprob_entropy_shard_stats(const void* logits, const int64_t* labels, const int32_t* extra_ptr, const int64_t* extra_labels,
                                               float* stats, float* extra_picked,
                                               int32_t R, int32_t V, int64_t row_stride, float temperature, int32_t dtype, float softcap, void* stream) {
  if (!stats) return DTA_EINVAL;
  return fwd_launch({{logits, labels, extra_ptr, extra_labels, nullptr, nullptr, nullptr, extra_picked, stats, R, V, row_stride, 1.f}, softcap},
                    dtype, temperature, stream);
}

extern "C" int dta_logprob_entropy_bwd(const void* logits, void* dlogits, const int64_t* labels, const int32_t* extra_ptr, const int64_t* extra_labels,
                                       const float* lse, const float* entropy,
                                       const float* g_logprob, const float* g_extra_logprob, const float* g_entropy,
                                       int32_t R, int32_t V, int64_t row_stride, int64_t out_row_stride, float temperature, int32_t dtype,
                                       float softcap, void* stream) {
  return bwd_launch({{logits, dlogits, labels, extra_ptr, extra_labels, lse, entropy, g_logprob, g_extra_logprob, g_entropy, R, V, row_stride,
                      out_row_stride, 1.f}, softcap}, dtype, temperature, stream);
}
