// fp32 tree attention for gfx950 - the CORRECTNESS path of fp32 models (the reference runs `--dtype fp32` through sdpa,
// run.py:122-132; SURVEY §8d recommends an fp32 tree-vs-dense check at <= 1e-5, far below the bf16 noise floor).
//
// Same visibility rule, same buffers and the same workspace conventions as the MFMA kernels of tree_attn.hip
//   packed trie:  key s visible to query t  <=>  s <= t < subtree_end[s]        stack form: subtree_end == NULL, t = q_offset + row
//   lse [Hq, Tq]   = log2-domain log-sum-exp of the scaled scores (m + log2 l with m = max(c·s), c = scale·log2 e)
//   delta [Hq, Tq] = -rowsum(dO ∘ O)
// but plain fp32 FMAs (157 TFLOP/s vector rate; an fp32 MFMA form would buy 2x at most and this is not a performance path):
// a row (query row in fwd / dQ, key row in dK/dV) is owned by FOUR adjacent lanes with D/4 of the D head dims each (D = 128 or 64), the
// rows of the other side are staged 32 at a time through LDS and broadcast-read; dot products are reduced across the quad with two DPP
// shuffles.  One workgroup = 64 rows x 1 head (fwd, dQ) or 64 keys x 1 kv head over its whole query range and GQA group (dK/dV:
// no atomics, no slabs - the split-Q work units of the MFMA kernel are ignored here).  Deterministic by construction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "dta_common.h"
#include "dta_device.h"

namespace {

constexpr int ROWS = 64;        // rows owned by a workgroup (4 lanes each -> 256 threads)
constexpr int ST = 32;          // rows of the other side staged per LDS tile

struct P32 {
  const float *q, *k, *v, *o, *dout;
  float *out, *dq, *dk, *dv, *lse_w, *delta;
  const float* lse_r;
  const int32_t *subtree_end, *run_ptr, *runs, *ktile_qend;
  int32_t Tq, Tk, q_offset, Hq, Hkv, group;
  int64_t q_st, q_sh, kv_st, kv_sh, v_st, v_sh, o_st, o_sh, dq_st, dq_sh, dkv_st, dkv_sh;
  float scale; int32_t accumulate;
};
// sliding window: key s also needs s >= win_lo[row] (packed form) or q_offset + row - window + 1 (stack form, win_lo == NULL); a type of its
// own so that the kernels without a window keep their arguments and code
struct P32W : P32 { const int32_t* win_lo; int32_t window; };
// soft-capped scores (softcap * tanh(scale q.k / softcap), capped before the mask): parameter types of their own again
struct P32C : P32 { float softcap; };
struct P32WC : P32W { float softcap; };
template <bool WIN, bool CAP = false> using P32T = typename std::conditional<CAP, typename std::conditional<WIN, P32WC, P32C>::type,
                                                                             typename std::conditional<WIN, P32W, P32>::type>::type;
// t = tanh(x) and 1 - t^2 from a = 2 log2(e) x: with E = 2^min(a, 64) and r = 1 / (1 + E), t = 1 - 2r and 1 - t^2 = 4 E r^2 (no cancellation
// in the derivative; E stays finite, so E r^2 is never inf * 0 and both saturate cleanly to +-1 and 0)
__device__ __forceinline__ float cap_tanh32(float a, float* sech2) {
  const float E = __builtin_amdgcn_exp2f(fminf(a, 64.f)), r = __builtin_amdgcn_rcpf(1.f + E);
  *sech2 = 4.f * (E * r) * r;
  return __builtin_fmaf(-2.f, r, 1.f);
}
// kt turns a raw q.k into tanh's argument (2 log2(e) scale / softcap); the log2-domain score factor c becomes softcap log2(e)
template <class P> __device__ __forceinline__ float cap_of(const P& p) {
  if constexpr (std::is_base_of<P32C, P>::value || std::is_base_of<P32WC, P>::value) return p.softcap; else return 0.f;
}
#define DTA_CAP_CONSTANTS                                                                                  \
  const float c = (CAP ? cap_of(p) : p.scale) * LOG2E;                                                     \
  [[maybe_unused]] const float kt = CAP ? 2.f * LOG2E * p.scale / cap_of(p) : 0.f;
template <bool WIN, class P> __device__ __forceinline__ int win_lo_of(const P& p, int row) {
  if constexpr (WIN) { const int lo = p.q_offset + row - p.window + 1; return p.win_lo ? p.win_lo[row] : (lo > 0 ? lo : 0); }
  else return 0;
}

__device__ __forceinline__ float quad_sum(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); return v; }

// 32 rows x D floats of `base` (row stride `st` elements) starting at row r0, rows clamped to [0, rmax), into img
template <int D> __device__ __forceinline__ void stage_rows(float* img, const float* base, int64_t st, int r0, int rmax, int tid) {
  constexpr int SH = D == 128 ? 5 : 4;                 // log2(float4 per row)
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int id = tid + 256 * i, row = id >> SH, c4 = id & (D / 4 - 1);
    int gr = r0 + row; gr = gr < rmax ? gr : rmax - 1; gr = gr < 0 ? 0 : gr;
    reinterpret_cast<float4*>(img)[row * (D / 4) + c4] = *reinterpret_cast<const float4*>(base + (int64_t)gr * st + 4 * c4);
  }
}

// this lane's quarter of a row: D/4 floats
template <int D> __device__ __forceinline__ void load_part(float* dst, const float* src) {
#pragma unroll
  for (int i = 0; i < D / 16; ++i) { const float4 t = reinterpret_cast<const float4*>(src)[i]; dst[4 * i] = t.x; dst[4 * i + 1] = t.y; dst[4 * i + 2] = t.z; dst[4 * i + 3] = t.w; }
}

// key runs of this workgroup's 64 query rows: the run list of their 128-row query tile (a superset; the per-pair test below is
// the complete visibility rule) or, in the stack form, the single run [0, q_offset + last row + 1)
struct Runs {
  const int32_t* runs; int ri, re, k0, kend;
  __device__ __forceinline__ bool next() {
    while (ri < re) {
      if (runs) { k0 = runs[4 * ri]; kend = runs[4 * ri + 1]; }
      ++ri;
      if (k0 < kend) return true;
    }
    return false;
  }
};
template <bool WIN, class P> __device__ __forceinline__ Runs runs_of(const P& p, int q0) {
  Runs r; r.runs = p.runs;
  if (p.runs) { const int qt = q0 / DTA_QTILE; r.ri = p.run_ptr[qt]; r.re = p.run_ptr[qt + 1]; r.k0 = r.kend = 0; }
  else { r.ri = 0; r.re = 1; r.k0 = 0; const int last = p.q_offset + (q0 + ROWS < p.Tq ? q0 + ROWS : p.Tq); r.kend = last < p.Tk ? last : p.Tk; }
  if constexpr (WIN) if (!p.runs && !p.win_lo) r.k0 = win_lo_of<WIN>(p, q0);     // stack form: the first row's bound is the block's lowest
  return r;
}

template <int D, bool WIN, bool CAP>
__global__ __launch_bounds__(256) void tree_attn_fwd_f32_kernel(P32T<WIN, CAP> p) {
  constexpr int PD = D / 4;                                         // head dims per lane
  __shared__ __attribute__((aligned(16))) float Ks[ST * D];
  __shared__ __attribute__((aligned(16))) float Vs[ST * D];
  __shared__ int se_s[ST];
  const int tid = threadIdx.x, row = tid >> 2, part = tid & 3;
  const int hq = blockIdx.y, kvh = hq / p.group;
  const int q0 = blockIdx.x * ROWS, qrow = q0 + row, qrow_c = qrow < p.Tq ? qrow : p.Tq - 1, qidx = p.q_offset + qrow;
  const int wlo = win_lo_of<WIN>(p, qrow_c);
  float q[PD], o[PD];
  load_part<D>(q, p.q + (int64_t)qrow_c * p.q_st + (int64_t)hq * p.q_sh + PD * part);
#pragma unroll
  for (int d = 0; d < PD; ++d) o[d] = 0.f;
  float m = -1e30f, l = 0.f;
  DTA_CAP_CONSTANTS
  const float* kb = p.k + (int64_t)kvh * p.kv_sh; const float* vb = p.v + (int64_t)kvh * p.v_sh;
  Runs rn = runs_of<WIN>(p, q0);
  while (rn.next()) {
    for (int k0 = rn.k0; k0 < rn.kend; k0 += ST) {
      __syncthreads();
      stage_rows<D>(Ks, kb, p.kv_st, k0, p.Tk, tid); stage_rows<D>(Vs, vb, p.v_st, k0, p.Tk, tid);
      if (tid < ST) { const int ki = k0 + tid; se_s[tid] = (p.subtree_end && ki < p.Tk) ? p.subtree_end[ki] : 0x7fffffff; }
      __syncthreads();
      const int n = rn.kend - k0 < ST ? rn.kend - k0 : ST;
      for (int j = 0; j < n; ++j) {
        const float* kr = Ks + j * D + PD * part;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < PD; ++d) s = __builtin_fmaf(q[d], kr[d], s);
        s = quad_sum(s);
        const int key = k0 + j;
        if (key <= qidx && qidx < se_s[j] && key < p.Tk && (!WIN || key >= wlo)) {
          if constexpr (CAP) { float unused; s = cap_tanh32(s * kt, &unused); }
          const float sc = s * c, mn = fmaxf(m, sc);
          const float alpha = __builtin_amdgcn_exp2f(m - mn), pj = __builtin_amdgcn_exp2f(sc - mn);
          const float* vr = Vs + j * D + PD * part;
          l = __builtin_fmaf(l, alpha, pj);
#pragma unroll
          for (int d = 0; d < PD; ++d) o[d] = __builtin_fmaf(pj, vr[d], o[d] * alpha);
          m = mn;
        }
      }
    }
  }
  if (qrow < p.Tq) {
    const float inv = 1.f / l;
    float* op = p.out + (int64_t)qrow * p.o_st + (int64_t)hq * p.o_sh + PD * part;
#pragma unroll
    for (int i = 0; i < PD / 4; ++i) reinterpret_cast<float4*>(op)[i] = make_float4(o[4 * i] * inv, o[4 * i + 1] * inv, o[4 * i + 2] * inv, o[4 * i + 3] * inv);
    if (part == 0) p.lse_w[(int64_t)hq * p.Tq + qrow] = m + __builtin_amdgcn_logf(l);      // v_log_f32 = log2
  }
}

template <int D, bool WIN, bool CAP>
__global__ __launch_bounds__(256) void tree_attn_bwd_dq_f32_kernel(P32T<WIN, CAP> p) {
  constexpr int PD = D / 4;                                         // head dims per lane
  __shared__ __attribute__((aligned(16))) float Ks[ST * D];
  __shared__ __attribute__((aligned(16))) float Vs[ST * D];
  __shared__ int se_s[ST];
  const int tid = threadIdx.x, row = tid >> 2, part = tid & 3;
  const int hq = blockIdx.y, kvh = hq / p.group;
  const int q0 = blockIdx.x * ROWS, qrow = q0 + row, qrow_c = qrow < p.Tq ? qrow : p.Tq - 1, qidx = p.q_offset + qrow;
  const int wlo = win_lo_of<WIN>(p, qrow_c);
  float q[PD], dof[PD], dq[PD];
  load_part<D>(q, p.q + (int64_t)qrow_c * p.q_st + (int64_t)hq * p.q_sh + PD * part);
  load_part<D>(dof, p.dout + (int64_t)qrow_c * p.o_st + (int64_t)hq * p.o_sh + PD * part);
  float delta = 0.f;
  {
    float of[PD];
    load_part<D>(of, p.o + (int64_t)qrow_c * p.o_st + (int64_t)hq * p.o_sh + PD * part);
#pragma unroll
    for (int d = 0; d < PD; ++d) { delta = __builtin_fmaf(dof[d], of[d], delta); dq[d] = 0.f; }
  }
  delta = quad_sum(delta);
  const float lse2 = p.lse_r[(int64_t)hq * p.Tq + qrow_c];
  if (part == 0 && qrow < p.Tq) p.delta[(int64_t)hq * p.Tq + qrow] = -delta;
  DTA_CAP_CONSTANTS
  const float* kb = p.k + (int64_t)kvh * p.kv_sh; const float* vb = p.v + (int64_t)kvh * p.v_sh;
  Runs rn = runs_of<WIN>(p, q0);
  while (rn.next()) {
    for (int k0 = rn.k0; k0 < rn.kend; k0 += ST) {
      __syncthreads();
      stage_rows<D>(Ks, kb, p.kv_st, k0, p.Tk, tid); stage_rows<D>(Vs, vb, p.v_st, k0, p.Tk, tid);
      if (tid < ST) { const int ki = k0 + tid; se_s[tid] = (p.subtree_end && ki < p.Tk) ? p.subtree_end[ki] : 0x7fffffff; }
      __syncthreads();
      const int n = rn.kend - k0 < ST ? rn.kend - k0 : ST;
      for (int j = 0; j < n; ++j) {
        const float* kr = Ks + j * D + PD * part; const float* vr = Vs + j * D + PD * part;
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < PD; ++d) { s = __builtin_fmaf(q[d], kr[d], s); dp = __builtin_fmaf(dof[d], vr[d], dp); }
        s = quad_sum(s); dp = quad_sum(dp);
        const int key = k0 + j;
        if (key <= qidx && qidx < se_s[j] && key < p.Tk && (!WIN || key >= wlo)) {
          float sech2 = 1.f;
          if constexpr (CAP) s = cap_tanh32(s * kt, &sech2);
          float ds = __builtin_amdgcn_exp2f(__builtin_fmaf(s, c, -lse2)) * (dp - delta);
          if constexpr (CAP) ds *= sech2;
#pragma unroll
          for (int d = 0; d < PD; ++d) dq[d] = __builtin_fmaf(ds, kr[d], dq[d]);
        }
      }
    }
  }
  if (qrow < p.Tq) {
    float* dp_ = p.dq + (int64_t)qrow * p.dq_st + (int64_t)hq * p.dq_sh + PD * part;
    const float sc = p.scale;
#pragma unroll
    for (int i = 0; i < PD / 4; ++i) reinterpret_cast<float4*>(dp_)[i] = make_float4(dq[4 * i] * sc, dq[4 * i + 1] * sc, dq[4 * i + 2] * sc, dq[4 * i + 3] * sc);
  }
}

// key-owned sweep: 64 keys of one kv head x every query that can see them x the heads of the GQA group
template <int D, bool WIN, bool CAP>
__global__ __launch_bounds__(256) void tree_attn_bwd_dkv_f32_kernel(P32T<WIN, CAP> p) {
  constexpr int PD = D / 4;                                         // head dims per lane
  __shared__ __attribute__((aligned(16))) float Qs[ST * D];
  __shared__ __attribute__((aligned(16))) float Ds[ST * D];
  __shared__ float lse_s[ST], nd_s[ST];
  const int tid = threadIdx.x, row = tid >> 2, part = tid & 3;
  const int kvh = blockIdx.y;
  const int k0 = blockIdx.x * ROWS, key = k0 + row, key_c = key < p.Tk ? key : p.Tk - 1;
  float kf[PD], vf[PD], dk[PD], dv[PD];
  load_part<D>(kf, p.k + (int64_t)key_c * p.kv_st + (int64_t)kvh * p.kv_sh + PD * part);
  load_part<D>(vf, p.v + (int64_t)key_c * p.v_st + (int64_t)kvh * p.v_sh + PD * part);
#pragma unroll
  for (int d = 0; d < PD; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
  const int se = (p.subtree_end && key < p.Tk) ? p.subtree_end[key_c] : 0x7fffffff;
  DTA_CAP_CONSTANTS
  // global query indices [t_begin, t_end) that may see a key of this block
  int t_begin = k0 > p.q_offset ? k0 : p.q_offset;
  int t_end = p.q_offset + p.Tq;
  if (p.ktile_qend) {                                  // max subtree_end over each DTA_KTILE-key tile (this block lies inside one)
    const int qe = p.ktile_qend[k0 / DTA_KTILE];
    t_end = qe < t_end ? qe : t_end;
  }
  if constexpr (WIN) if (!p.win_lo) {                  // stack form: query t sees this block only while t - window + 1 <= its last key
    const int64_t wl = (int64_t)k0 + ROWS - 1 + p.window; t_end = wl < t_end ? (int)wl : t_end;
  }
  for (int g = 0; g < p.group; ++g) {
    const int hq = kvh * p.group + g;
    const float* qb = p.q + (int64_t)hq * p.q_sh; const float* dob = p.dout + (int64_t)hq * p.o_sh;
    for (int t0 = t_begin; t0 < t_end; t0 += ST) {
      const int r0 = t0 - p.q_offset;
      __syncthreads();
      stage_rows<D>(Qs, qb, p.q_st, r0, p.Tq, tid); stage_rows<D>(Ds, dob, p.o_st, r0, p.Tq, tid);
      if (tid < ST) { int rr = r0 + tid; rr = rr < p.Tq ? rr : p.Tq - 1; lse_s[tid] = p.lse_r[(int64_t)hq * p.Tq + rr]; nd_s[tid] = p.delta[(int64_t)hq * p.Tq + rr]; }
      __syncthreads();
      const int n = t_end - t0 < ST ? t_end - t0 : ST;
      for (int i = 0; i < n; ++i) {
        const float* qr = Qs + i * D + PD * part; const float* dr = Ds + i * D + PD * part;
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < PD; ++d) { s = __builtin_fmaf(kf[d], qr[d], s); dp = __builtin_fmaf(vf[d], dr[d], dp); }
        s = quad_sum(s); dp = quad_sum(dp);
        const int t = t0 + i;
        if (key <= t && t < se && key < p.Tk && (!WIN || key >= win_lo_of<WIN>(p, t - p.q_offset))) {
          float sech2 = 1.f;
          if constexpr (CAP) s = cap_tanh32(s * kt, &sech2);
          const float pj = __builtin_amdgcn_exp2f(__builtin_fmaf(s, c, -lse_s[i]));
          float ds = pj * (dp + nd_s[i]);
          if constexpr (CAP) ds *= sech2;
#pragma unroll
          for (int d = 0; d < PD; ++d) { dv[d] = __builtin_fmaf(pj, dr[d], dv[d]); dk[d] = __builtin_fmaf(ds, qr[d], dk[d]); }
        }
      }
    }
  }
  if (key < p.Tk) {
    float* dkp = p.dk + (int64_t)key * p.dkv_st + (int64_t)kvh * p.dkv_sh + PD * part;
    float* dvp = p.dv + (int64_t)key * p.dkv_st + (int64_t)kvh * p.dkv_sh + PD * part;
    const float sc = p.scale;
#pragma unroll
    for (int i = 0; i < PD / 4; ++i) {
      float4 a = make_float4(dk[4 * i] * sc, dk[4 * i + 1] * sc, dk[4 * i + 2] * sc, dk[4 * i + 3] * sc);
      float4 b = make_float4(dv[4 * i], dv[4 * i + 1], dv[4 * i + 2], dv[4 * i + 3]);
      if (p.accumulate) {                               // 1: add to the caller's gradient, 2: add into the fp32 grad-KV stacks - the same thing in fp32
        const float4 x = reinterpret_cast<const float4*>(dkp)[i], y = reinterpret_cast<const float4*>(dvp)[i];
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w; b.x += y.x; b.y += y.y; b.z += y.z; b.w += y.w;
      }
      reinterpret_cast<float4*>(dkp)[i] = a; reinterpret_cast<float4*>(dvp)[i] = b;
    }
  }
}

}  // namespace

// kernel parameters of the chosen form from the call's arguments (the forward's backward fields are null)
template <bool WIN, bool CAP> static P32T<WIN, CAP> kernel_params(const DtaAttnArgs& a) {
  P32T<WIN, CAP> p{};
  if constexpr (WIN) { p.win_lo = a.win_lo; p.window = a.window; }
  if constexpr (CAP) p.softcap = a.softcap;
  p.q = (const float*)a.q; p.k = (const float*)a.k; p.v = (const float*)a.v; p.o = (const float*)a.o; p.dout = (const float*)a.dout;
  p.out = (float*)a.out; p.dq = (float*)a.dq; p.dk = (float*)a.dk; p.dv = (float*)a.dv; p.lse_w = a.lse_w; p.lse_r = a.lse_r; p.delta = a.delta;
  p.subtree_end = a.subtree_end; p.run_ptr = a.run_ptr; p.runs = a.runs; p.ktile_qend = a.ktile_qend;
  p.Tq = a.Tq; p.Tk = a.Tk; p.q_offset = a.q_offset; p.Hq = a.Hq; p.Hkv = a.Hkv; p.group = a.Hq / a.Hkv;
  p.q_st = a.q_st; p.q_sh = a.q_sh; p.kv_st = a.kv_st; p.kv_sh = a.kv_sh; p.v_st = a.v_st; p.v_sh = a.v_sh; p.o_st = a.o_st; p.o_sh = a.o_sh;
  p.dq_st = a.dq_st; p.dq_sh = a.dq_sh; p.dkv_st = a.dkv_st; p.dkv_sh = a.dkv_sh; p.scale = a.scale; p.accumulate = a.accumulate;
  return p;
}

// f(D) with head_dim as a std::integral_constant
template <class F> static void with_head_dim(const DtaAttnArgs& a, F&& f) {
  if (a.head_dim == 64) f(std::integral_constant<int, 64>{}); else f(std::integral_constant<int, 128>{});
}

int dta_attn_fwd_f32(const DtaAttnArgs& a) {
  dta_attn_form(a, [&](auto win, auto cap) {
    constexpr bool WIN = decltype(win)::value, CAP = decltype(cap)::value;
    const P32T<WIN, CAP> p = kernel_params<WIN, CAP>(a);
    with_head_dim(a, [&](auto d) {
      hipLaunchKernelGGL((tree_attn_fwd_f32_kernel<decltype(d)::value, WIN, CAP>), dim3((a.Tq + ROWS - 1) / ROWS, a.Hq), dim3(256), 0, a.stream, p);
    });
  });
  return DTA_LAUNCH_STATUS();
}

int dta_attn_bwd_f32(const DtaAttnArgs& a) {
  dta_attn_form(a, [&](auto win, auto cap) {
    constexpr bool WIN = decltype(win)::value, CAP = decltype(cap)::value;
    const P32T<WIN, CAP> p = kernel_params<WIN, CAP>(a);
    const dim3 gq((a.Tq + ROWS - 1) / ROWS, a.Hq), gk((a.Tk + ROWS - 1) / ROWS, a.Hkv);
    with_head_dim(a, [&](auto d) {
      constexpr int D = decltype(d)::value;
      if (a.which & 1) hipLaunchKernelGGL((tree_attn_bwd_dq_f32_kernel<D, WIN, CAP>), gq, dim3(256), 0, a.stream, p);      // also writes -delta
      if (a.which & 2) hipLaunchKernelGGL((tree_attn_bwd_dkv_f32_kernel<D, WIN, CAP>), gk, dim3(256), 0, a.stream, p);
    });
  });
  return DTA_LAUNCH_STATUS();                           // (which & 4, the slab finalize of the MFMA path, has nothing to do here)
}
