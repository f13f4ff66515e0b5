// Policy objective over the packed trie (include/dta.h, dta_policy_loss): the clipped PPO / GRPO surrogate, KL penalty, entropy bonus
// and loss mask of losses.PolicyLoss evaluated where the data lives - every packed row once, dlp[T] and dent[T] written directly.
//
// Row-major work.  Row t at depth d is on the path of the sequences s of ONE contiguous range [row_seq_lo[t], row_seq_hi[t]) (callback
// order) with n_s = len_s - 1 >= d.  For each of them it owns the log-prob term (s, j = d - 1) when d >= 1 and the entropy term
// (s, j = d) when d < n_s: every (s, j) is owned by exactly one row in each role, so nothing is scattered and nothing is atomic.
// A thread takes a row; a row whose range is longer than PL_SERIAL sequences is summed by its whole wave, lane-strided over s and
// joined by the xor butterfly - a fixed order either way, so equal inputs give equal bits.
//
// Sequence-level ratios (dta_policy_loss_seq, GSPO): every token of sequence s is clipped on r_s = exp(sum_j m_j x_j / n^), so the
// surrogate's gradient at token t of s is c_s m_t with one scalar c_s per sequence.  A sequence pass (one workgroup per sequence)
// walks the sequence's root path - a few contiguous row runs - for r_s, w_s, c_s and the surrogate's share of the statistics; the row
// pass is the one above with c_s m in place of the token's own surrogate gradient; one reduction joins the partials of both.
//
// Preference objectives (dta_preference_loss: DPO / cDPO / SimPO, SLiC, IPO): a pair couples two sequences, so a pair pass stands
// between the sequence pass (u_s, one number per sequence, over the same path walk) and a row pass that sums g_s m with the pair's
// coefficient g_s; the statistics are per pair and come from the pair pass alone.
#include "dta_common.h"
#include "dta_device.h"
#include <math.h>

namespace {

constexpr int PL_BLOCK = 256;       // rows per workgroup step
constexpr int PL_SERIAL = 16;       // longest sequence range a single thread sums
constexpr int PL_MAX_BLOCKS = 1024; // grid cap: the rest is grid-strided, the partial-sum workspace has at most this many rows
constexpr int PL_NSTAT = 8;         // {loss, sum m pg, sum m kl, sum m entropy, clipped tokens, sum m, 0, 0}
constexpr int PL_SEQ_BLOCKS = 2048; // grid cap of the sequence pass: one workgroup per sequence, the rest grid-strided

struct PolicyParams {
  const float *lp, *ent;
  const int32_t *depth, *row_lo, *row_hi, *seq_ptr;
  const float *old_lp, *ref_lp, *mask, *adv, *w;
  const float* c = nullptr;                  // sequence-level ratios only: the surrogate's gradient scalar per sequence
  float *dlp, *dent, *partial;
  int32_t T, S, adv_per_seq;
  float lo, hi, dual, kl_coef, ent_coef;     // lo = 1 - clip_low, hi = 1 + clip_high, dual = 0: none
};

struct Acc { float glp, gent, st[6]; };

// the terms row (depth d, log-prob lp_t, entropy ent_t) owns for sequence s
template <int KL>
__device__ __forceinline__ void seq_terms(const PolicyParams& p, int s, int d, float lp_t, float ent_t, Acc& a) {
  const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
  if (n < d) return;                                       // the sequence ends above this row
  const float w = p.w[s];
  if (d >= 1) {
    const int i = b + d - 1;
    const float m = p.mask[i];
    const float A = p.adv[p.adv_per_seq ? s : i];
    const float r = p.old_lp ? expf(lp_t - p.old_lp[i]) : 1.f;
    const float s1 = -r * A, s2 = -fminf(fmaxf(r, p.lo), p.hi) * A;
    float pg = fmaxf(s1, s2);
    bool clipped = s2 > s1;                                // the clamp is the active branch: d pg / d lp = 0
    if (p.dual > 0.f && A < 0.f) {
      const float cap = -p.dual * A;
      if (cap < pg) { pg = cap; clipped = true; }
    }
    float g = clipped ? 0.f : s1;                          // d(-r A)/d lp = -r A
    float kl = 0.f;
    if (KL >= 0) {
      const float dd = p.ref_lp[i] - lp_t;
      float dk;
      if (KL == 0) { kl = -dd; dk = 1.f; }
      else if (KL == 1) { kl = 0.5f * dd * dd; dk = -dd; }
      else { const float e = expf(dd); kl = e - dd - 1.f; dk = 1.f - e; }
      g += p.kl_coef * dk;
      a.st[2] += m * kl;
    }
    const float wm = w * m;
    a.glp += wm * g;
    a.st[0] += wm * (pg + p.kl_coef * kl);
    a.st[1] += m * pg;
    a.st[4] += clipped ? m : 0.f;
    a.st[5] += m;
  }
  if (d < n) {
    const float m = p.mask[b + d];
    const float wm = w * m;
    a.gent -= wm * p.ent_coef;
    a.st[0] -= wm * p.ent_coef * ent_t;
    a.st[3] += m * ent_t;
  }
}

// the same for sequence-level ratios: the surrogate's value and statistics are the sequence pass's, its gradient here is c_s m
template <int KL>
__device__ __forceinline__ void seq_terms_sl(const PolicyParams& p, int s, int d, float lp_t, float ent_t, Acc& a) {
  const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
  if (n < d) return;
  const float w = p.w[s];
  if (d >= 1) {
    const int i = b + d - 1;
    const float m = p.mask[i];
    float g = p.c[s] * m;
    if (KL >= 0) {
      const float dd = p.ref_lp[i] - lp_t;
      float kl, dk;
      if (KL == 0) { kl = -dd; dk = 1.f; }
      else if (KL == 1) { kl = 0.5f * dd * dd; dk = -dd; }
      else { const float e = expf(dd); kl = e - dd - 1.f; dk = 1.f - e; }
      const float wm = w * m;
      g += wm * (p.kl_coef * dk);
      a.st[0] += wm * (p.kl_coef * kl);
      a.st[2] += m * kl;
    }
    a.glp += g;
    a.st[5] += m;
  }
  if (d < n) {
    const float m = p.mask[b + d];
    const float wm = w * m;
    a.gent -= wm * p.ent_coef;
    a.st[0] -= wm * p.ent_coef * ent_t;
    a.st[3] += m * ent_t;
  }
}

template <int KL, bool SEQ>
__device__ __forceinline__ void row_terms(const PolicyParams& p, int s, int d, float lp_t, float ent_t, Acc& a) {
  if (SEQ) seq_terms_sl<KL>(p, s, d, lp_t, ent_t, a);
  else seq_terms<KL>(p, s, d, lp_t, ent_t, a);
}

template <int KL, bool SEQ = false>
__global__ __launch_bounds__(PL_BLOCK) void policy_loss_kernel(const PolicyParams p) {
  __shared__ float red[PL_BLOCK / 64][PL_NSTAT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Acc a;
  for (int i = 0; i < 6; ++i) a.st[i] = 0.f;
  for (int base = blockIdx.x * PL_BLOCK; base < p.T; base += gridDim.x * PL_BLOCK) {   // `base` is the same in every lane of the workgroup
    const int t = base + threadIdx.x;
    const bool live = t < p.T;
    int d = 0, s0 = 0, s1 = 0;
    float lp_t = 0.f, ent_t = 0.f;
    if (live) {
      d = p.depth[t]; lp_t = p.lp[t]; ent_t = p.ent[t];
      s0 = max(p.row_lo[t], 0); s1 = min(p.row_hi[t], p.S);
    }
    a.glp = 0.f; a.gent = 0.f;
    const bool wide = s1 - s0 > PL_SERIAL;
    if (!wide)
      for (int s = s0; s < s1; ++s) row_terms<KL, SEQ>(p, s, d, lp_t, ent_t, a);
    // rows with a long range: the wave takes them one after the other, in lane order
    unsigned long long todo = __ballot(wide);
    float glp_w = 0.f, gent_w = 0.f;
    while (todo) {
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int dk = __shfl(d, k), b0 = __shfl(s0, k), b1 = __shfl(s1, k);
      const float lpk = __shfl(lp_t, k), entk = __shfl(ent_t, k);
      Acc r = a;
      r.glp = 0.f; r.gent = 0.f;
      for (int s = b0 + lane; s < b1; s += 64) row_terms<KL, SEQ>(p, s, dk, lpk, entk, r);
      for (int i = 0; i < 6; ++i) a.st[i] = r.st[i];
      const float gl = wave_sum(r.glp), ge = wave_sum(r.gent);
      if (lane == k) { glp_w = gl; gent_w = ge; }
    }
    if (live) {
      p.dlp[t] = wide ? glp_w : a.glp;
      p.dent[t] = wide ? gent_w : a.gent;
    }
  }
  // the workgroup's partial sums: lanes by butterfly, then the four waves in order
  for (int i = 0; i < 6; ++i) {
    const float v = wave_sum(a.st[i]);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < PL_NSTAT) {
    float v = 0.f;
    if (threadIdx.x < 6)
      for (int wv = 0; wv < PL_BLOCK / 64; ++wv) v += red[wv][threadIdx.x];
    p.partial[blockIdx.x * PL_NSTAT + threadIdx.x] = v;
  }
}

// stats[c] = sum over the workgroups' partials, in a fixed order: 32 strided chains per column, then the 32 in order
__global__ __launch_bounds__(256) void policy_loss_reduce_kernel(const float* __restrict__ partial, int nb, float* __restrict__ stats) {
  __shared__ float red[32][PL_NSTAT];
  const int c = threadIdx.x & 7, g = threadIdx.x >> 3;
  float v = 0.f;
  for (int b = g; b < nb; b += 32) v += partial[b * PL_NSTAT + c];
  red[g][c] = v;
  __syncthreads();
  if (threadIdx.x < PL_NSTAT) {
    float s = 0.f;
    for (int i = 0; i < 32; ++i) s += red[i][threadIdx.x];
    stats[threadIdx.x] = s;
  }
}

// w[s] = scale / max(sum of the sequence's mask, 1): one workgroup per sequence, lanes strided, butterfly, the four waves in order
__global__ __launch_bounds__(256) void policy_seq_weight_kernel(const float* __restrict__ mask, const int32_t* __restrict__ seq_ptr, int S,
                                                               float scale, float* __restrict__ w) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = blockIdx.x; s < S; s += gridDim.x) {
    const int b = seq_ptr[s], e = seq_ptr[s + 1];
    float v = 0.f;
    for (int i = b + (int)threadIdx.x; i < e; i += 256) v += mask[i];
    v = wave_sum(v);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) w[s] = scale / fmaxf(((red[0] + red[1]) + red[2]) + red[3], 1.f);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void policy_fill_weight_kernel(int S, float scale, float* __restrict__ w) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < S) w[s] = scale;
}

// The sequence pass of the sequence-level objective.  Sequence s follows the root path of leaf seq_leaf[s]: runs
// [leaf_run_ptr[leaf], leaf_run_ptr[leaf + 1]) of contiguous packed rows, run k starting at row run_row0[k] with depth run_depth0[k].
// Prediction j of s (element seq_ptr[s] + j of the per-token inputs) is the row of depth j + 1.
struct SeqPassParams {
  const float* lp;
  const int32_t *seq_ptr, *leaf_run_ptr, *run_row0, *run_depth0, *seq_leaf;
  const float *old_lp, *mask, *adv;
  float *w, *c, *partial;
  int32_t T, S, M, R, adv_per_seq, seq_mean;
  float lo, hi, dual, scale;
};

// the workgroup's sum of v in a fixed order (lanes by butterfly, the four waves in order), in every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                         // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void policy_seq_pass_kernel(const SeqPassParams p) {
  __shared__ float red[4];
  float st_loss = 0.f, st_pg = 0.f, st_clip = 0.f;         // thread 0: this workgroup's sequences, in order
  for (int s = blockIdx.x; s < p.S; s += gridDim.x) {      // `s` is the same in every thread of the workgroup
    const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
    float sm = 0.f, sx = 0.f;
    if (p.old_lp) {
      const int leaf = min(max(p.seq_leaf[s], 0), p.M - 1);
      const int k0 = max(p.leaf_run_ptr[leaf], 0), k1 = min(p.leaf_run_ptr[leaf + 1], p.R);
      for (int k = k0; k < k1; ++k) {
        const int row0 = p.run_row0[k], d0 = p.run_depth0[k];
        const int da = max(d0, 1), db = min(k + 1 < k1 ? p.run_depth0[k + 1] : n + 1, n + 1);     // depths [da, db) of this run
        for (int d = da + (int)threadIdx.x; d < db; d += 256) {
          const int t = row0 + (d - d0), i = b + d - 1;
          if (t < 0 || t >= p.T) continue;
          const float m = p.mask[i];
          sm += m;
          sx += m * (p.lp[t] - p.old_lp[i]);
        }
      }
    } else {
      for (int j = threadIdx.x; j < n; j += 256) sm += p.mask[b + j];
    }
    const float nh = fmaxf(block_sum(sm, red), 1.f);
    const float r = p.old_lp ? expf(block_sum(sx, red) / nh) : 1.f;
    const float w = p.seq_mean ? p.scale / nh : p.scale;
    // every token of the sequence sees the same r: its branch depends on the sign of its advantage alone
    const float rc = fminf(fmaxf(r, p.lo), p.hi);
    float spg = 0.f, sg = 0.f, sc = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) {
      const float m = p.mask[b + j];
      const float A = p.adv[p.adv_per_seq ? s : b + j];
      const float s1 = -r * A, s2 = -rc * A;
      float pg = fmaxf(s1, s2);
      bool clipped = s2 > s1;
      if (p.dual > 0.f && A < 0.f) {
        const float cap = -p.dual * A;
        if (cap < pg) { pg = cap; clipped = true; }
      }
      spg += m * pg;
      sg += clipped ? 0.f : m * -A;
      sc += clipped ? m : 0.f;
    }
    spg = block_sum(spg, red); sg = block_sum(sg, red); sc = block_sum(sc, red);
    if (threadIdx.x == 0) {
      p.w[s] = w;
      p.c[s] = w * r / nh * sg;
      st_loss += w * spg; st_pg += spg; st_clip += sc;
    }
  }
  if (threadIdx.x == 0) {                                  // this workgroup's row of the partial sums: the surrogate's columns
    float* out = p.partial + (size_t)blockIdx.x * PL_NSTAT;
    out[0] = st_loss; out[1] = st_pg; out[2] = 0.f; out[3] = 0.f; out[4] = st_clip; out[5] = 0.f; out[6] = 0.f; out[7] = 0.f;
  }
}

// ---- preference objectives (dta_preference_loss): DPO / cDPO / SimPO, SLiC, IPO --------------------------------------------------
// A pair couples two sequences, so there is a pair stage between a sequence pass and a row pass: the sequence pass leaves one
// number u_s per sequence, the pair pass turns the two numbers of a pair into one coefficient g_s per member, and the row pass sums
// g_s m over the sequences through a row - the same row-major ownership as above, with nothing but the mask to read per term.

constexpr int PF_MAX_BLOCKS = 1024; // grid cap of the pair pass: one thread per pair, the rest grid-strided; one partial row per workgroup

struct PrefSeqParams {
  const float* lp;
  const int32_t *seq_ptr, *leaf_run_ptr, *run_row0, *run_depth0, *seq_leaf;
  const float *ref_lp, *ref_sum, *mask;
  float *nhat, *u, *sft, *g;
  int32_t T, S, M, R, length_normalize;
};

// n^_s, u_s and P_s / n^_s of every sequence, and g_s = 0 (the pair pass overwrites the members of a pair)
__global__ __launch_bounds__(256) void preference_seq_pass_kernel(const PrefSeqParams p) {
  __shared__ float red[4];
  for (int s = blockIdx.x; s < p.S; s += gridDim.x) {      // `s` is the same in every thread of the workgroup
    const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
    const int leaf = min(max(p.seq_leaf[s], 0), p.M - 1);
    const int k0 = max(p.leaf_run_ptr[leaf], 0), k1 = min(p.leaf_run_ptr[leaf + 1], p.R);
    float sm = 0.f, sp = 0.f, sf = 0.f;
    for (int k = k0; k < k1; ++k) {
      const int row0 = p.run_row0[k], d0 = p.run_depth0[k];
      const int da = max(d0, 1), db = min(k + 1 < k1 ? p.run_depth0[k + 1] : n + 1, n + 1);       // depths [da, db) of this run
      for (int d = da + (int)threadIdx.x; d < db; d += 256) {
        const int t = row0 + (d - d0), i = b + d - 1;
        if (t < 0 || t >= p.T) continue;
        const float m = p.mask[i];
        sm += m;
        sp += m * p.lp[t];
        if (p.ref_lp) sf += m * p.ref_lp[i];
      }
    }
    const float nh = fmaxf(block_sum(sm, red), 1.f);
    const float P = block_sum(sp, red);
    const float F = p.ref_lp ? block_sum(sf, red) : p.ref_sum ? p.ref_sum[s] : 0.f;
    if (threadIdx.x == 0) {
      p.nhat[s] = nh;
      p.u[s] = p.length_normalize ? (P - F) / nh : P - F;
      p.sft[s] = P / nh;
      p.g[s] = 0.f;
    }
  }
}

struct PrefPairParams {
  const int32_t *pair_c, *pair_r;
  const float *nhat, *u, *sft;
  float *g, *partial;
  int32_t S, P, kind, length_normalize;
  float beta, eps, gamma, half_inv_beta, sft_coef, scale;   // half_inv_beta = 1 / (2 beta): the target of "ipo"
};

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// one thread per pair: z, L, the two coefficients and the pair's share of the statistics
__global__ __launch_bounds__(PL_BLOCK) void preference_pair_kernel(const PrefPairParams p) {
  __shared__ float red[PL_BLOCK / 64][PL_NSTAT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float st[PL_NSTAT];
  for (int i = 0; i < PL_NSTAT; ++i) st[i] = 0.f;
  for (int q = blockIdx.x * PL_BLOCK + threadIdx.x; q < p.P; q += gridDim.x * PL_BLOCK) {
    const int c = p.pair_c[q], r = p.pair_r[q];
    if (c < 0 || c >= p.S || r < 0 || r >= p.S) continue;
    const float uc = p.u[c], ur = p.u[r], du = uc - ur;
    float L, dLdu;                                         // the pair's loss and its derivative by u_c (by u_r: the negative)
    if (p.kind == 2) {
      const float h = du - p.half_inv_beta;
      L = h * h; dLdu = 2.f * h;
    } else {
      const float z = p.beta * du - p.gamma;
      float dz;
      if (p.kind == 0) {
        const float e = expf(-fabsf(z));                   // in (0, 1]: neither branch can overflow
        const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        L = (1.f - p.eps) * softplus_f(-z) + p.eps * softplus_f(z);
        dz = sig - (1.f - p.eps);
      } else {
        L = fmaxf(0.f, 1.f - z);
        dz = z < 1.f ? -1.f : 0.f;
      }
      dLdu = p.beta * dz;
    }
    const float nc = p.nhat[c], sc = p.sft[c];
    const float a = p.scale * dLdu;
    p.g[c] = (p.length_normalize ? a / nc : a) - p.scale * p.sft_coef / nc;
    p.g[r] = -(p.length_normalize ? a / p.nhat[r] : a);
    st[0] += p.scale * L - p.scale * p.sft_coef * sc;
    st[1] += L; st[2] += sc;
    st[3] += p.beta * du; st[4] += p.beta * uc; st[5] += p.beta * ur;
    st[6] += uc > ur ? 1.f : 0.f; st[7] += 1.f;
  }
  for (int i = 0; i < PL_NSTAT; ++i) {
    const float v = wave_sum(st[i]);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < PL_NSTAT) {
    float v = 0.f;
    for (int wv = 0; wv < PL_BLOCK / 64; ++wv) v += red[wv][threadIdx.x];
    p.partial[blockIdx.x * PL_NSTAT + threadIdx.x] = v;
  }
}

struct PrefRowParams {
  const int32_t *depth, *row_lo, *row_hi, *seq_ptr;
  const float *mask, *g;
  float* dlp;
  int32_t T, S;
};

// the term row (depth d >= 1) owns for sequence s: g_s m at prediction d - 1
__device__ __forceinline__ float pref_term(const PrefRowParams& p, int s, int d) {
  const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
  return n < d ? 0.f : p.g[s] * p.mask[b + d - 1];
}

// dlp for every row: the row kernel of the policy objective with g_s m as the only term
__global__ __launch_bounds__(PL_BLOCK) void preference_row_kernel(const PrefRowParams p) {
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * PL_BLOCK; base < p.T; base += gridDim.x * PL_BLOCK) {   // `base` is the same in every lane of the workgroup
    const int t = base + threadIdx.x;
    const bool live = t < p.T;
    int d = 0, s0 = 0, s1 = 0;
    if (live) {
      d = p.depth[t];
      if (d >= 1) { s0 = max(p.row_lo[t], 0); s1 = min(p.row_hi[t], p.S); }
    }
    const bool wide = s1 - s0 > PL_SERIAL;
    float v = 0.f;
    if (!wide)
      for (int s = s0; s < s1; ++s) v += pref_term(p, s, d);
    unsigned long long todo = __ballot(wide);
    while (todo) {                                         // rows with a long range: the wave takes them one after the other
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int dk = __shfl(d, k), b0 = __shfl(s0, k), b1 = __shfl(s1, k);
      float r = 0.f;
      for (int s = b0 + lane; s < b1; s += 64) r += pref_term(p, s, dk);
      r = wave_sum(r);
      if (lane == k) v = r;
    }
    if (live) p.dlp[t] = v;
  }
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int dta_policy_loss_blocks(int32_t T) { return T <= 0 ? DTA_EINVAL : row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS); }

extern "C" int dta_policy_loss(const float* lp, const float* ent, const int32_t* depth, const int32_t* row_seq_lo, const int32_t* row_seq_hi,
                               const int32_t* seq_ptr, const float* old_lp, const float* ref_lp, const float* mask, const float* adv,
                               int32_t adv_per_seq, float* w, float* dlp, float* dent, float* partial, float* stats, int32_t T, int32_t S,
                               float clip_low, float clip_high, float dual_clip, float kl_coef, int32_t kl_estimator, float entropy_coef,
                               int32_t agg, float scale, void* stream) {
  if (!lp || !ent || !depth || !row_seq_lo || !row_seq_hi || !seq_ptr || !mask || !adv || !w || !dlp || !dent || !partial || !stats ||
      T <= 0 || S <= 0)
    return DTA_EINVAL;
  if (!finite_f(clip_low) || !finite_f(clip_high) || clip_low < 0.f || clip_high < 0.f) return DTA_EINVAL;
  if (dual_clip != 0.f && !(finite_f(dual_clip) && dual_clip > 1.f)) return DTA_EINVAL;
  if (kl_estimator < 0 || kl_estimator > 2 || agg < 0 || agg > 1) return DTA_EINVAL;
  if (!finite_f(kl_coef) || !finite_f(entropy_coef) || !finite_f(scale)) return DTA_EINVAL;
  if (kl_coef != 0.f && !ref_lp) return DTA_EINVAL;
  if (!aligned16(lp) || !aligned16(ent) || !aligned16(depth) || !aligned16(row_seq_lo) || !aligned16(row_seq_hi) || !aligned16(seq_ptr) ||
      !aligned16(mask) || !aligned16(adv) || !aligned16(w) || !aligned16(dlp) || !aligned16(dent) || !aligned16(partial) || !aligned16(stats) ||
      (old_lp && !aligned16(old_lp)) || (ref_lp && !aligned16(ref_lp)))
    return DTA_EALIGN;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  if (agg == 0)
    hipLaunchKernelGGL(policy_seq_weight_kernel, dim3(S < 2048 ? S : 2048), dim3(256), 0, st_, mask, seq_ptr, S, scale, w);
  else
    hipLaunchKernelGGL(policy_fill_weight_kernel, dim3(ceil_blocks(S, 256)), dim3(256), 0, st_, S, scale, w);
  PolicyParams p;
  p.lp = lp; p.ent = ent; p.depth = depth; p.row_lo = row_seq_lo; p.row_hi = row_seq_hi; p.seq_ptr = seq_ptr;
  p.old_lp = old_lp; p.ref_lp = kl_coef != 0.f ? ref_lp : nullptr; p.mask = mask; p.adv = adv; p.w = w;
  p.dlp = dlp; p.dent = dent; p.partial = partial;
  p.T = T; p.S = S; p.adv_per_seq = adv_per_seq != 0;
  p.lo = 1.f - clip_low; p.hi = 1.f + clip_high; p.dual = dual_clip; p.kl_coef = kl_coef; p.ent_coef = entropy_coef;
  const int nb = row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS);
  const dim3 grid(nb), block(PL_BLOCK);
  if (kl_coef == 0.f) hipLaunchKernelGGL(policy_loss_kernel<-1>, grid, block, 0, st_, p);
  else if (kl_estimator == 0) hipLaunchKernelGGL(policy_loss_kernel<0>, grid, block, 0, st_, p);
  else if (kl_estimator == 1) hipLaunchKernelGGL(policy_loss_kernel<1>, grid, block, 0, st_, p);
  else hipLaunchKernelGGL(policy_loss_kernel<2>, grid, block, 0, st_, p);
  hipLaunchKernelGGL(policy_loss_reduce_kernel, dim3(1), dim3(256), 0, st_, partial, nb, stats);
  return DTA_LAUNCH_STATUS();
}

extern "C" int dta_policy_loss_seq_blocks(int32_t T, int32_t S) {
  return T <= 0 || S <= 0 ? DTA_EINVAL : row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS) + (S < PL_SEQ_BLOCKS ? S : PL_SEQ_BLOCKS);
}

extern "C" int dta_policy_loss_seq(const float* lp, const float* ent, const int32_t* depth, const int32_t* row_seq_lo, const int32_t* row_seq_hi,
                                   const int32_t* seq_ptr, const int32_t* leaf_run_ptr, const int32_t* run_row0, const int32_t* run_depth0,
                                   const int32_t* seq_leaf, const float* old_lp, const float* ref_lp, const float* mask, const float* adv,
                                   int32_t adv_per_seq, float* w, float* c, float* dlp, float* dent, float* partial, float* stats, int32_t T,
                                   int32_t S, int32_t M, int32_t R, float clip_low, float clip_high, float dual_clip, float kl_coef,
                                   int32_t kl_estimator, float entropy_coef, int32_t agg, float scale, void* stream) {
  if (!lp || !ent || !depth || !row_seq_lo || !row_seq_hi || !seq_ptr || !leaf_run_ptr || !run_row0 || !run_depth0 || !seq_leaf || !mask ||
      !adv || !w || !c || !dlp || !dent || !partial || !stats || T <= 0 || S <= 0 || M <= 0 || R <= 0)
    return DTA_EINVAL;
  if (!finite_f(clip_low) || !finite_f(clip_high) || clip_low < 0.f || clip_high < 0.f) return DTA_EINVAL;
  if (dual_clip != 0.f && !(finite_f(dual_clip) && dual_clip > 1.f)) return DTA_EINVAL;
  if (kl_estimator < 0 || kl_estimator > 2 || agg < 0 || agg > 1) return DTA_EINVAL;
  if (!finite_f(kl_coef) || !finite_f(entropy_coef) || !finite_f(scale)) return DTA_EINVAL;
  if (kl_coef != 0.f && !ref_lp) return DTA_EINVAL;
  if (!aligned16(lp) || !aligned16(ent) || !aligned16(depth) || !aligned16(row_seq_lo) || !aligned16(row_seq_hi) || !aligned16(seq_ptr) ||
      !aligned16(leaf_run_ptr) || !aligned16(run_row0) || !aligned16(run_depth0) || !aligned16(seq_leaf) || !aligned16(mask) ||
      !aligned16(adv) || !aligned16(w) || !aligned16(c) || !aligned16(dlp) || !aligned16(dent) || !aligned16(partial) || !aligned16(stats) ||
      (old_lp && !aligned16(old_lp)) || (ref_lp && !aligned16(ref_lp)))
    return DTA_EALIGN;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  const int nb = row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS), nsb = S < PL_SEQ_BLOCKS ? S : PL_SEQ_BLOCKS;
  SeqPassParams q;
  q.lp = lp; q.seq_ptr = seq_ptr; q.leaf_run_ptr = leaf_run_ptr; q.run_row0 = run_row0; q.run_depth0 = run_depth0; q.seq_leaf = seq_leaf;
  q.old_lp = old_lp; q.mask = mask; q.adv = adv; q.w = w; q.c = c; q.partial = partial + (size_t)nb * PL_NSTAT;
  q.T = T; q.S = S; q.M = M; q.R = R; q.adv_per_seq = adv_per_seq != 0; q.seq_mean = agg == 0;
  q.lo = 1.f - clip_low; q.hi = 1.f + clip_high; q.dual = dual_clip; q.scale = scale;
  hipLaunchKernelGGL(policy_seq_pass_kernel, dim3(nsb), dim3(256), 0, st_, q);
  PolicyParams p;
  p.lp = lp; p.ent = ent; p.depth = depth; p.row_lo = row_seq_lo; p.row_hi = row_seq_hi; p.seq_ptr = seq_ptr;
  p.old_lp = nullptr; p.ref_lp = kl_coef != 0.f ? ref_lp : nullptr; p.mask = mask; p.adv = adv; p.w = w; p.c = c;
  p.dlp = dlp; p.dent = dent; p.partial = partial;
  p.T = T; p.S = S; p.adv_per_seq = adv_per_seq != 0;
  p.lo = q.lo; p.hi = q.hi; p.dual = dual_clip; p.kl_coef = kl_coef; p.ent_coef = entropy_coef;
  const dim3 grid(nb), block(PL_BLOCK);
  if (kl_coef == 0.f) hipLaunchKernelGGL((policy_loss_kernel<-1, true>), grid, block, 0, st_, p);
  else if (kl_estimator == 0) hipLaunchKernelGGL((policy_loss_kernel<0, true>), grid, block, 0, st_, p);
  else if (kl_estimator == 1) hipLaunchKernelGGL((policy_loss_kernel<1, true>), grid, block, 0, st_, p);
  else hipLaunchKernelGGL((policy_loss_kernel<2, true>), grid, block, 0, st_, p);
  hipLaunchKernelGGL(policy_loss_reduce_kernel, dim3(1), dim3(256), 0, st_, partial, nb + nsb, stats);
  return DTA_LAUNCH_STATUS();
}

extern "C" int dta_preference_loss_blocks(int32_t T, int32_t S, int32_t P) {
  return T <= 0 || S <= 0 || P <= 0 ? DTA_EINVAL : row_blocks(P, PL_BLOCK, PF_MAX_BLOCKS);
}

extern "C" int dta_preference_loss(const float* lp, const int32_t* depth, const int32_t* row_seq_lo, const int32_t* row_seq_hi,
                                   const int32_t* seq_ptr, const int32_t* leaf_run_ptr, const int32_t* run_row0, const int32_t* run_depth0,
                                   const int32_t* seq_leaf, const int32_t* pair_c, const int32_t* pair_r, const float* ref_lp,
                                   const float* ref_sum, const float* mask, float* nhat, float* u, float* sft, float* g, float* dlp,
                                   float* partial, float* stats, int32_t T, int32_t S, int32_t M, int32_t R, int32_t P, int32_t kind,
                                   float beta, float label_smoothing, float gamma, int32_t length_normalize, int32_t reference_free,
                                   float sft_coef, float scale, void* stream) {
  if (!lp || !depth || !row_seq_lo || !row_seq_hi || !seq_ptr || !leaf_run_ptr || !run_row0 || !run_depth0 || !seq_leaf || !pair_c ||
      !pair_r || !mask || !nhat || !u || !sft || !g || !dlp || !partial || !stats || T <= 0 || S <= 0 || M <= 0 || R <= 0 || P <= 0)
    return DTA_EINVAL;
  if (kind < 0 || kind > 2) return DTA_EINVAL;
  if (!finite_f(beta) || !finite_f(label_smoothing) || !finite_f(gamma) || !finite_f(sft_coef) || !finite_f(scale)) return DTA_EINVAL;
  if (!(beta > 0.f) || label_smoothing < 0.f || !(label_smoothing < 0.5f) || (label_smoothing != 0.f && kind != 0)) return DTA_EINVAL;
  if ((kind == 2 && gamma != 0.f) || sft_coef < 0.f) return DTA_EINVAL;
  if (!reference_free && (ref_lp != nullptr) == (ref_sum != nullptr)) return DTA_EINVAL;      // exactly one form of the reference
  if (reference_free) ref_lp = ref_sum = nullptr;                                             // neither is read
  if (!aligned16(lp) || !aligned16(depth) || !aligned16(row_seq_lo) || !aligned16(row_seq_hi) || !aligned16(seq_ptr) ||
      !aligned16(leaf_run_ptr) || !aligned16(run_row0) || !aligned16(run_depth0) || !aligned16(seq_leaf) || !aligned16(pair_c) ||
      !aligned16(pair_r) || !aligned16(mask) || !aligned16(nhat) || !aligned16(u) || !aligned16(sft) || !aligned16(g) || !aligned16(dlp) ||
      !aligned16(partial) || !aligned16(stats) || (ref_lp && !aligned16(ref_lp)) || (ref_sum && !aligned16(ref_sum)))
    return DTA_EALIGN;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  PrefSeqParams q;
  q.lp = lp; q.seq_ptr = seq_ptr; q.leaf_run_ptr = leaf_run_ptr; q.run_row0 = run_row0; q.run_depth0 = run_depth0; q.seq_leaf = seq_leaf;
  q.ref_lp = ref_lp; q.ref_sum = ref_sum; q.mask = mask; q.nhat = nhat; q.u = u; q.sft = sft; q.g = g;
  q.T = T; q.S = S; q.M = M; q.R = R; q.length_normalize = length_normalize != 0;
  hipLaunchKernelGGL(preference_seq_pass_kernel, dim3(S < PL_SEQ_BLOCKS ? S : PL_SEQ_BLOCKS), dim3(256), 0, st_, q);
  PrefPairParams c;
  c.pair_c = pair_c; c.pair_r = pair_r; c.nhat = nhat; c.u = u; c.sft = sft; c.g = g; c.partial = partial;
  c.S = S; c.P = P; c.kind = kind; c.length_normalize = q.length_normalize;
  c.beta = beta; c.eps = label_smoothing; c.gamma = gamma; c.half_inv_beta = 1.f / (2.f * beta); c.sft_coef = sft_coef; c.scale = scale;
  const int npb = row_blocks(P, PL_BLOCK, PF_MAX_BLOCKS);
  hipLaunchKernelGGL(preference_pair_kernel, dim3(npb), dim3(PL_BLOCK), 0, st_, c);
  PrefRowParams r;
  r.depth = depth; r.row_lo = row_seq_lo; r.row_hi = row_seq_hi; r.seq_ptr = seq_ptr; r.mask = mask; r.g = g; r.dlp = dlp; r.T = T; r.S = S;
  hipLaunchKernelGGL(preference_row_kernel, dim3(row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS)), dim3(PL_BLOCK), 0, st_, r);
  hipLaunchKernelGGL(policy_loss_reduce_kernel, dim3(1), dim3(256), 0, st_, partial, npb, stats);
  return DTA_LAUNCH_STATUS();
}
