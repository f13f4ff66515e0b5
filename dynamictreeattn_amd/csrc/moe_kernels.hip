// Mixture-of-experts kernels for gfx950 (MI355X, CDNA4): router top-k, permutation of the (token, slot) pairs by expert, grouped GEMMs
// over the expert-sorted rows and the weighted combine.  They restate HF Qwen3MoeSparseMoeBlock (transformers 5.x, modeling_qwen3_moe.py:
// Qwen3MoeTopKRouter.forward and Qwen3MoeExperts.forward); the C ABI and the HF lines each entry point restates are in include/dta.h.
//
// Determinism: the permutation is a counting sort whose within-expert order is the pair order (token order) - the only atomics are
// integer counts in LDS, which do not decide any order; the combine backward and the scatter-back of the input gradient sum in a fixed
// order; nothing adds floats atomically.  Two identical calls give identical bits, which the layer recomputation relies on (it re-routes
// in the backward).
//
// Grouped GEMM (MFMA 32x32x16, bf16 / f16, fp32 accumulation): a workgroup of 4 waves owns a 128 x 128 output tile, each wave 64 x 64
// (2 x 2 MFMA blocks); k-steps of 64 staged global -> registers -> LDS.  Each operand is staged in its MEMORY layout: an operand whose
// contraction index is contiguous (X rows, W_e rows in the forward) is read back by rows (ds_read_b128), one whose contraction index is the
// slow axis (W_e in the dgrad, dY and X in the wgrad) by the transposed read ds_read_b64_tr_b16 - no transposed copy of any weight exists.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dta_common.h"
#include "dta_device.h"

namespace {

template <int DT> __device__ __forceinline__ float ldf(const void* p, int64_t i) { return (float)reinterpret_cast<const typename Ty<DT>::e*>(p)[i]; }
template <int DT> __device__ __forceinline__ void stf(void* p, int64_t i, float v) { reinterpret_cast<typename Ty<DT>::e*>(p)[i] = (typename Ty<DT>::e)v; }

constexpr int MAXE = 256, MAXK = 16, EPL = MAXE / 64;    // experts per lane in the router kernels

// ------------------------------------------------------------------------------------------------------------------------------------
// Router: one wave per token row; lane l holds experts l, l+64, l+128, l+192.
// ------------------------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void router_fwd_k(const void* logits, int32_t* ids, void* wout, float* lse, int T, int E_, int k, int norm) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;                                  // wave-uniform
  float x[EPL], p[EPL];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < EPL; ++i) { const int e = lane + 64 * i; x[i] = e < E_ ? ldf<DT>(logits, (int64_t)t * E_ + e) : -INFINITY; m = fmaxf(m, x[i]); }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) { p[i] = lane + 64 * i < E_ ? __expf(x[i] - m) : 0.f; s += p[i]; }
  s = wave_sum(s);
  const float inv = 1.f / s;
#pragma unroll
  for (int i = 0; i < EPL; ++i) p[i] = lane + 64 * i < E_ ? p[i] * inv : -1.f;     // -1: never selected
  if (lane == 0) lse[t] = m + __logf(s);
  float mine = 0.f, sum = 0.f;                           // lane j keeps the j-th pick
  int mine_e = 0;
  for (int j = 0; j < k; ++j) {
    // best of this lane (ties: lower expert index, i.e. lower i), then across lanes (ties: lower expert index)
    float bv = -2.f; int be = MAXE;
#pragma unroll
    for (int i = 0; i < EPL; ++i) if (p[i] > bv) { bv = p[i]; be = lane + 64 * i; }
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(bv, o); const int oe = __shfl_xor(be, o);
      if (ov > bv || (ov == bv && oe < be)) { bv = ov; be = oe; }
    }
#pragma unroll
    for (int i = 0; i < EPL; ++i) if (lane + 64 * i == be) p[i] = -1.f;
    sum += bv;
    if (lane == j) { mine = bv; mine_e = be; }
  }
  if (lane < k) {
    ids[(int64_t)t * k + lane] = mine_e;
    stf<DT>(wout, (int64_t)t * k + lane, norm ? mine / sum : mine);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void router_bwd_k(const void* logits, const float* lse, const int32_t* ids, const void* dw, void* dlogits,
                                                    int T, int E_, int k, int norm) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const float L = lse[t];
  int id[MAXK]; float ps[MAXK], dp[MAXK];
  float S = 0.f;
#pragma unroll
  for (int j = 0; j < MAXK; ++j) {
    if (j >= k) break;
    id[j] = ids[(int64_t)t * k + j];
    ps[j] = __expf(ldf<DT>(logits, (int64_t)t * E_ + id[j]) - L);
    dp[j] = ldf<DT>(dw, (int64_t)t * k + j);
    S += ps[j];
  }
  if (norm) {          // w_j = p_j / S:  dL/dp_j = (dw_j - sum_i dw_i w_i) / S
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) { if (j >= k) break; dot += dp[j] * ps[j]; }
    dot /= S;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) { if (j >= k) break; dp[j] = (dp[j] - dot) / S; }
  }
  float g = 0.f;       // softmax: dlogit_e = p_e (dp_e - sum_j dp_j p_j)
#pragma unroll
  for (int j = 0; j < MAXK; ++j) { if (j >= k) break; g += dp[j] * ps[j]; }
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const int e = lane + 64 * i;
    if (e >= E_) break;
    const float pe = __expf(ldf<DT>(logits, (int64_t)t * E_ + e) - L);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) { if (j >= k) break; if (id[j] == e) d = dp[j]; }
    stf<DT>(dlogits, (int64_t)t * E_ + e, pe * (d - g));
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Permutation: counting sort of the P = T*k pairs by expert in chunks of PCH pairs.
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int PCH = 256;

__global__ __launch_bounds__(PCH) void perm_count_k(const int32_t* ids, int P, int E_, int32_t* counts) {
  __shared__ int cnt[MAXE];
  const int tid = threadIdx.x, p = blockIdx.x * PCH + tid;
  cnt[tid] = 0;
  __syncthreads();
  if (p < P) { const int e = ids[p]; if (e >= 0 && e < E_) atomicAdd(&cnt[e], 1); }   // integer counts: order-free
  __syncthreads();
  if (tid < E_) counts[(int64_t)blockIdx.x * E_ + tid] = cnt[tid];
}

// one workgroup: counts[c][e] -> first row of chunk c's pairs of expert e (exclusive scan over chunks plus the expert offset),
// expert offsets, and the tile table {expert, first row} of the GEMMs (unused entries: expert -1)
__global__ __launch_bounds__(MAXE) void perm_scan_k(int32_t* counts, int nch, int E_, int BM, int32_t* offsets, int32_t* tiles, int bound) {
  __shared__ int tot[MAXE], off[MAXE + 1], tstart[MAXE + 1];
  const int e = threadIdx.x;
  int run = 0;
  if (e < E_) for (int c = 0; c < nch; ++c) { const int v = counts[(int64_t)c * E_ + e]; counts[(int64_t)c * E_ + e] = run; run += v; }
  tot[e] = e < E_ ? run : 0;
  __syncthreads();
  if (e == 0) {
    int o = 0, ts = 0;
    for (int i = 0; i < E_; ++i) { off[i] = o; tstart[i] = ts; o += tot[i]; ts += (tot[i] + BM - 1) / BM; }
    off[E_] = o; tstart[E_] = ts;
  }
  __syncthreads();
  if (e < E_) offsets[e] = off[e];
  if (e == 0) offsets[E_] = off[E_];
  if (e < E_) {
    const int n = (tot[e] + BM - 1) / BM;
    for (int i = 0; i < n; ++i) { tiles[2 * (tstart[e] + i)] = e; tiles[2 * (tstart[e] + i) + 1] = off[e] + i * BM; }
  }
  for (int i = tstart[E_] + e; i < bound; i += blockDim.x) { tiles[2 * i] = -1; tiles[2 * i + 1] = 0; }
}

__global__ __launch_bounds__(PCH) void perm_place_k(const int32_t* ids, int P, int k, int E_, const int32_t* counts, const int32_t* offsets,
                                                    int32_t* row_of_pair, int32_t* src_token) {
  __shared__ int eid[PCH];
  const int tid = threadIdx.x, p = blockIdx.x * PCH + tid;
  int e = p < P ? ids[p] : -1;
  if (e >= E_) e = -1;
  eid[tid] = e;
  __syncthreads();
  if (p >= P) return;
  if (e < 0) { row_of_pair[p] = -1; return; }
  int rank = 0;
  for (int j = 0; j < tid; ++j) rank += eid[j] == e;
  const int row = offsets[e] + counts[(int64_t)blockIdx.x * E_ + e] + rank;
  row_of_pair[p] = row;
  src_token[row] = p / k;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Grouped GEMM, MFMA.  C[m][n] = sum_k A[m][k] B[k][n] per 128 x 128 tile.
//   mode 0 (fwd)   A = X[gather(row)][k]     (k fast)   B[k][n] = W_e[n][k]  (k fast)    out Y[row][n]      rows of the tile table
//   mode 1 (dgrad) A = dY[row][k]            (k fast)   B[k][n] = W_e[k][n]  (n fast)    out dX[row][n]     rows of the tile table
//   mode 2 (wgrad) A[i][r] = dY[r][i]        (i fast)   B[r][j] = X[g(r)][j] (j fast)    out dW_e[i][j]     k = the expert's rows
// ------------------------------------------------------------------------------------------------------------------------------------
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int KF_LD = BK + 8;           // k-fast image [128][BK]: 144-B rows (16-B multiple for ds_read_b128)
constexpr int OF_LD = BM + 8;           // outer-fast image [BK][128]: 272-B rows (8-B multiple for ds_read_b64_tr_b16)
constexpr int IMG = (BM * KF_LD > BK * OF_LD ? BM * KF_LD : BK * OF_LD);

struct GemmArgs {
  const void *x, *w, *dy; void* out;
  const int32_t *gather, *offsets, *tiles;
  int N, K;          // W_e is [N][K]
};

// staging of one operand tile: 512 / 256 = 4 16-byte vectors per thread (either image holds 128 x 64 elements)
struct Stage { uint4 v[4]; };

// k-fast operand: element (outer o, k) at base + row(o) * ld + k; rows/cols beyond the limits read as zero
__device__ __forceinline__ void load_kfast(Stage& s, const char* base, int64_t ld, int esz, const int32_t* gather, int o0, int olim, int k0, int klim) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = threadIdx.x + 256 * i, o = v >> 3, kc = (v & 7) * 8;
    uint4 r = {0, 0, 0, 0};
    if (o0 + o < olim && k0 + kc < klim) {
      const int64_t row = gather ? gather[o0 + o] : o0 + o;
      r = *reinterpret_cast<const uint4*>(base + (row * ld + k0 + kc) * esz);
    }
    s.v[i] = r;
  }
}
__device__ __forceinline__ void store_kfast(const Stage& s, char* img) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int v = threadIdx.x + 256 * i, o = v >> 3, kc = (v & 7) * 8; *reinterpret_cast<uint4*>(img + (o * KF_LD + kc) * 2) = s.v[i]; }
}
// outer-fast operand: element (outer o, k) at base + row(k) * ld + o
__device__ __forceinline__ void load_ofast(Stage& s, const char* base, int64_t ld, int esz, const int32_t* gather, int o0, int olim, int k0, int klim) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = threadIdx.x + 256 * i, kk = v >> 4, oc = (v & 15) * 8;
    uint4 r = {0, 0, 0, 0};
    if (k0 + kk < klim && o0 + oc < olim) {
      const int64_t row = gather ? gather[k0 + kk] : k0 + kk;
      r = *reinterpret_cast<const uint4*>(base + (row * ld + o0 + oc) * esz);
    }
    s.v[i] = r;
  }
}
__device__ __forceinline__ void store_ofast(const Stage& s, char* img) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int v = threadIdx.x + 256 * i, kk = v >> 4, oc = (v & 15) * 8; *reinterpret_cast<uint4*>(img + (kk * OF_LD + oc) * 2) = s.v[i]; }
}

template <int DT, int MODE>
__global__ __launch_bounds__(256) void gg_mfma_k(GemmArgs a) {
  using V8 = typename Ty<DT>::v8;
  __shared__ __attribute__((aligned(16))) char lds_a[IMG * 2];
  __shared__ __attribute__((aligned(16))) char lds_b[IMG * 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  int e, m0, mlim, n0, nlim, klim, k0 = 0;
  const char *pa, *pb; int64_t lda, ldb; const int32_t *ga = nullptr, *gb = nullptr;
  if (MODE < 2) {
    e = a.tiles[2 * blockIdx.x];
    if (e < 0) return;                                       // whole workgroup: beyond the tile table
    m0 = a.tiles[2 * blockIdx.x + 1]; mlim = a.offsets[e + 1];
    n0 = blockIdx.y * BN;
    if (MODE == 0) { pa = (const char*)a.x; lda = a.K; ga = a.gather; pb = (const char*)a.w + (int64_t)e * a.N * a.K * 2; ldb = a.K; nlim = a.N; klim = a.K; }
    else           { pa = (const char*)a.dy; lda = a.N; pb = (const char*)a.w + (int64_t)e * a.N * a.K * 2; ldb = a.K; nlim = a.K; klim = a.N; }
  } else {
    e = blockIdx.z; m0 = blockIdx.y * BM; mlim = a.N; n0 = blockIdx.x * BN; nlim = a.K;
    k0 = a.offsets[e]; klim = a.offsets[e + 1];
    pa = (const char*)a.dy; lda = a.N; pb = (const char*)a.x; ldb = a.K; gb = a.gather;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  Stage sa, sb;
  auto load = [&](int kb) {
    if (MODE < 2) load_kfast(sa, pa, lda, 2, ga, m0, mlim, kb, klim); else load_ofast(sa, pa, lda, 2, nullptr, m0, mlim, kb, klim);
    if (MODE == 0) load_kfast(sb, pb, ldb, 2, nullptr, n0, nlim, kb, klim); else load_ofast(sb, pb, ldb, 2, gb, n0, nlim, kb, klim);
  };
  if (k0 < klim) load(k0);
  for (int kb = k0; kb < klim; kb += BK) {
    __syncthreads();
    if (MODE < 2) store_kfast(sa, lds_a); else store_ofast(sa, lds_a);
    if (MODE == 0) store_kfast(sb, lds_b); else store_ofast(sb, lds_b);
    __syncthreads();
    if (kb + BK < klim) load(kb + BK);                       // next tile in flight during this one's MFMAs
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      V8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = MODE < 2 ? frag_kfast<V8>(lds_a, KF_LD, 2 * wm + i, s, lane) : frag_ofast<V8>(lds_a, OF_LD, 2 * wm + i, s, lane);
        fb[i] = MODE == 0 ? frag_kfast<V8>(lds_b, KF_LD, 2 * wn + i, s, lane) : frag_ofast<V8>(lds_b, OF_LD, 2 * wn + i, s, lane);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Ty<DT>::mma(fa[i], fb[j], acc[i][j]);
    }
  }
  // C block (i, j): register r holds row 8(r>>2) + 4(lane>>5) + (r&3), column lane & 31
  typename Ty<DT>::e* out = reinterpret_cast<typename Ty<DT>::e*>(a.out);
  const int64_t ldo = MODE == 0 ? a.N : a.K;
  const int64_t obase = MODE == 2 ? (int64_t)e * a.N * a.K : 0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + i * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (m < mlim && n < nlim) out[obase + (int64_t)m * ldo + n] = (typename Ty<DT>::e)acc[i][j][r];
      }
    }
}

// fp32 grouped GEMM: plain FMAs (the gradient-check path of fp32 models), the same three modes on 64 x 64 tiles, k-steps of 16
constexpr int FB = 64, FK = 16;
template <int MODE>
__global__ __launch_bounds__(256) void gg_f32_k(GemmArgs a) {
  __shared__ float As[FK][FB + 4], Bs[FK][FB + 4];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  int e, m0, mlim, n0, nlim, klim, k0 = 0;
  if (MODE < 2) {
    const int tile = blockIdx.x >> 1;          // the tile table is in BM = 128-row tiles: two 64-row halves each
    e = a.tiles[2 * tile];
    if (e < 0) return;
    m0 = a.tiles[2 * tile + 1] + (blockIdx.x & 1) * FB; mlim = a.offsets[e + 1];
    if (m0 >= mlim) return;
    n0 = blockIdx.y * FB; nlim = MODE == 0 ? a.N : a.K; klim = MODE == 0 ? a.K : a.N;
  } else {
    e = blockIdx.z; m0 = blockIdx.y * FB; mlim = a.N; n0 = blockIdx.x * FB; nlim = a.K; k0 = a.offsets[e]; klim = a.offsets[e + 1];
  }
  const float* X = (const float*)a.x; const float* W = (const float*)a.w + (MODE < 2 ? (int64_t)e * a.N * a.K : 0); const float* DY = (const float*)a.dy;
  float acc[4][4] = {};
  for (int kb = k0; kb < klim; kb += FK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = tid + 256 * i;
      {   // A (m, k)
        int m, kk; float val = 0.f;
        if (MODE < 2) { m = v >> 4; kk = v & 15; } else { kk = v >> 6; m = v & 63; }
        const int gm = m0 + m, gk = kb + kk;
        if (gm < mlim && gk < klim) {
          if (MODE == 0) val = X[(int64_t)(a.gather ? a.gather[gm] : gm) * a.K + gk];
          else if (MODE == 1) val = DY[(int64_t)gm * a.N + gk];
          else val = DY[(int64_t)gk * a.N + gm];
        }
        As[kk][m] = val;
      }
      {   // B (k, n)
        int n, kk; float val = 0.f;
        if (MODE == 0) { n = v >> 4; kk = v & 15; } else { kk = v >> 6; n = v & 63; }
        const int gn = n0 + n, gk = kb + kk;
        if (gn < nlim && gk < klim) {
          if (MODE == 0) val = W[(int64_t)gn * a.K + gk];
          else if (MODE == 1) val = W[(int64_t)gk * a.K + gn];
          else val = X[(int64_t)(a.gather ? a.gather[gk] : gk) * a.K + gn];
        }
        Bs[kk][n] = val;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < FK; ++kk) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { av[i] = As[kk][ty * 4 + i]; bv[i] = Bs[kk][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* out = (float*)a.out;
  const int64_t ldo = MODE == 0 ? a.N : a.K, obase = MODE == 2 ? (int64_t)e * a.N * a.K : 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
      if (m < mlim && n < nlim) out[obase + (int64_t)m * ldo + n] = acc[i][j];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Combine
// ------------------------------------------------------------------------------------------------------------------------------------
// out[t][h] = sum_j w[t][j] * Y[row(t, j)][h]   (w == NULL: weight 1 - the scatter-back of the expert-sorted input gradient)
template <int DT>
__global__ __launch_bounds__(256) void combine_fwd_k(const void* Y, const void* w, const int32_t* row_of_pair, void* out, int T, int k, int H) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)T * H) return;
  const int t = (int)(idx / H), h = (int)(idx % H);
  float acc = 0.f;
  for (int j = 0; j < k; ++j) {
    const int r = row_of_pair[(int64_t)t * k + j];
    if (r < 0) continue;
    const float y = ldf<DT>(Y, (int64_t)r * H + h);
    acc = w ? fmaf(ldf<DT>(w, (int64_t)t * k + j), y, acc) : acc + y;
  }
  stf<DT>(out, idx, acc);
}
// dY[row(t, j)][h] = w[t][j] * dout[t][h]
template <int DT>
__global__ __launch_bounds__(256) void combine_bwd_dy_k(const void* dout, const void* w, const int32_t* row_of_pair, void* dY, int T, int k, int H) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)T * k * H) return;
  const int64_t p = idx / H; const int h = (int)(idx % H);
  const int r = row_of_pair[p];
  if (r < 0) return;
  stf<DT>(dY, (int64_t)r * H + h, ldf<DT>(w, p) * ldf<DT>(dout, (p / k) * H + h));
}
// dw[t][j] = <dout[t], Y[row(t, j)]>: one wave per pair, lane-strided partial sums and a fixed butterfly
template <int DT>
__global__ __launch_bounds__(256) void combine_bwd_dw_k(const void* dout, const void* Y, const int32_t* row_of_pair, void* dw, int T, int k, int H) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= (int64_t)T * k) return;
  const int r = row_of_pair[p];
  float acc = 0.f;
  if (r >= 0)
    for (int h = lane; h < H; h += 64) acc = fmaf(ldf<DT>(dout, (p / k) * H + h), ldf<DT>(Y, (int64_t)r * H + h), acc);
  acc = wave_sum(acc);
  if (lane == 0) stf<DT>(dw, p, acc);
}

}  // namespace

extern "C" {

int dta_moe_router_fwd(const void* logits, int32_t* topk_ids, void* topk_w, float* lse, int32_t T, int32_t E_, int32_t k, int32_t norm_topk,
                       int32_t dtype, void* stream) {
  if (T < 0 || E_ <= 0 || k <= 0 || k > E_ || (T > 0 && (!logits || !topk_ids || !topk_w || !lse))) return DTA_EINVAL;
  if (E_ > MAXE || k > MAXK || !row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (T == 0) return DTA_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 g(ceil_blocks(T, 4)), b(256);
  dta_storage_type(dtype, [&](auto dt) { router_fwd_k<decltype(dt)::value><<<g, b, 0, st>>>(logits, topk_ids, topk_w, lse, T, E_, k, norm_topk); });
  return DTA_LAUNCH_STATUS();
}

int dta_moe_router_bwd(const void* logits, const float* lse, const int32_t* topk_ids, const void* dtopk_w, void* dlogits,
                       int32_t T, int32_t E_, int32_t k, int32_t norm_topk, int32_t dtype, void* stream) {
  if (T < 0 || E_ <= 0 || k <= 0 || k > E_ || (T > 0 && (!logits || !lse || !topk_ids || !dtopk_w || !dlogits))) return DTA_EINVAL;
  if (E_ > MAXE || k > MAXK || !row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (T == 0) return DTA_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 g(ceil_blocks(T, 4)), b(256);
  dta_storage_type(dtype, [&](auto dt) {
    router_bwd_k<decltype(dt)::value><<<g, b, 0, st>>>(logits, lse, topk_ids, dtopk_w, dlogits, T, E_, k, norm_topk);
  });
  return DTA_LAUNCH_STATUS();
}

int dta_moe_permute_workspace(int32_t n_pairs, int32_t E_) {
  if (n_pairs < 0 || E_ <= 0) return DTA_EINVAL;
  const int64_t n = (int64_t)((n_pairs + PCH - 1) / PCH) * E_;
  return n > INT32_MAX ? DTA_EUNSUPPORTED : (int)n;
}

int dta_moe_tile_bound(int32_t n_pairs, int32_t E_) {
  if (n_pairs < 0 || E_ <= 0) return DTA_EINVAL;
  return (n_pairs + BM - 1) / BM + E_;
}

int dta_moe_permute(const int32_t* topk_ids, int32_t T, int32_t k, int32_t E_, int32_t* workspace,
                    int32_t* expert_offsets, int32_t* row_of_pair, int32_t* src_token, int32_t* tiles, void* stream) {
  if (T < 0 || k <= 0 || E_ <= 0 || !expert_offsets || !tiles || (T > 0 && (!topk_ids || !workspace || !row_of_pair || !src_token))) return DTA_EINVAL;
  if (E_ > MAXE || (int64_t)T * k > INT32_MAX - BM) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  const int P = T * k, nch = (P + PCH - 1) / PCH, bound = (P + BM - 1) / BM + E_;
  if (nch > 0) perm_count_k<<<nch, PCH, 0, st>>>(topk_ids, P, E_, workspace);
  perm_scan_k<<<1, MAXE, 0, st>>>(workspace, nch, E_, BM, expert_offsets, tiles, bound);
  if (nch > 0) perm_place_k<<<nch, PCH, 0, st>>>(topk_ids, P, k, E_, workspace, expert_offsets, row_of_pair, src_token);
  return DTA_LAUNCH_STATUS();
}

int dta_moe_grouped_gemm(int32_t mode, const void* x, const void* w, const void* dy, void* out, const int32_t* gather,
                         const int32_t* expert_offsets, const int32_t* tiles, int32_t n_rows, int32_t E_, int32_t N, int32_t K,
                         int32_t dtype, void* stream) {
  if (mode < DTA_MOE_FWD || mode > DTA_MOE_WGRAD || n_rows < 0 || E_ <= 0 || N <= 0 || K <= 0 || !out || !expert_offsets) return DTA_EINVAL;
  if ((mode == DTA_MOE_FWD && (!x || !w)) || (mode == DTA_MOE_DGRAD && (!dy || !w)) || (mode == DTA_MOE_WGRAD && (!dy || !x))) return DTA_EINVAL;
  if (mode != DTA_MOE_WGRAD && !tiles) return DTA_EINVAL;
  if (N % 16 || K % 16 || !row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  if ((x && !aligned16(x)) || (w && !aligned16(w)) || (dy && !aligned16(dy)) || !aligned16(out)) return DTA_EALIGN;   // the operand a mode does not read may be null
  DTA_REFUSE_IF_PRIOR_ERROR();
  hipStream_t st = (hipStream_t)stream;
  GemmArgs a{x, w, dy, out, gather, expert_offsets, tiles, N, K};
  const int bound = (n_rows + BM - 1) / BM + E_;
  if (mode != DTA_MOE_WGRAD && n_rows == 0) return DTA_OK;
  const int nout = mode == DTA_MOE_FWD ? N : K;
  const dim3 b(256);
  if (dtype == DTA_F32) {
    if (mode == DTA_MOE_FWD) gg_f32_k<0><<<dim3(2 * bound, ceil_blocks(nout, FB)), b, 0, st>>>(a);
    else if (mode == DTA_MOE_DGRAD) gg_f32_k<1><<<dim3(2 * bound, ceil_blocks(nout, FB)), b, 0, st>>>(a);
    else gg_f32_k<2><<<dim3(ceil_blocks(K, FB), ceil_blocks(N, FB), E_), b, 0, st>>>(a);
    return DTA_LAUNCH_STATUS();
  }
  dta_storage_type16(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (mode == DTA_MOE_FWD) gg_mfma_k<DT, 0><<<dim3(bound, ceil_blocks(nout, BN)), b, 0, st>>>(a);
    else if (mode == DTA_MOE_DGRAD) gg_mfma_k<DT, 1><<<dim3(bound, ceil_blocks(nout, BN)), b, 0, st>>>(a);
    else gg_mfma_k<DT, 2><<<dim3(ceil_blocks(K, BN), ceil_blocks(N, BM), E_), b, 0, st>>>(a);
  });
  return DTA_LAUNCH_STATUS();
}

int dta_moe_combine_fwd(const void* y, const void* topk_w, const int32_t* row_of_pair, void* out, int32_t T, int32_t k, int32_t H,
                        int32_t dtype, void* stream) {
  if (T < 0 || k <= 0 || H <= 0 || (T > 0 && (!y || !row_of_pair || !out))) return DTA_EINVAL;
  if (!row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (T == 0) return DTA_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = ceil_blocks((int64_t)T * H, 256);
  dta_storage_type(dtype, [&](auto dt) { combine_fwd_k<decltype(dt)::value><<<g, 256, 0, st>>>(y, topk_w, row_of_pair, out, T, k, H); });
  return DTA_LAUNCH_STATUS();
}

int dta_moe_combine_bwd(const void* dout, const void* y, const void* topk_w, const int32_t* row_of_pair, void* dy, void* dtopk_w,
                        int32_t T, int32_t k, int32_t H, int32_t dtype, void* stream) {
  if (T < 0 || k <= 0 || H <= 0 || (T > 0 && (!dout || !y || !topk_w || !row_of_pair || !dy || !dtopk_w))) return DTA_EINVAL;
  if (!row_dtype_ok(dtype)) return DTA_EUNSUPPORTED;
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (T == 0) return DTA_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g1 = ceil_blocks((int64_t)T * k * H, 256), g2 = ceil_blocks((int64_t)T * k, 4);
  dta_storage_type(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    combine_bwd_dy_k<DT><<<g1, 256, 0, st>>>(dout, topk_w, row_of_pair, dy, T, k, H);
    combine_bwd_dw_k<DT><<<g2, 256, 0, st>>>(dout, y, row_of_pair, dtopk_w, T, k, H);
  });
  return DTA_LAUNCH_STATUS();
}

}  // extern "C"
