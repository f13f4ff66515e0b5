// Policy objective over the packed trie (include/dta.h, dta_policy_loss): the clipped PPO / GRPO surrogate, KL penalty, entropy bonus
// and loss mask of losses.PolicyLoss evaluated where the data lives - every packed row once, dlp[T] and dent[T] written directly.
//
// Row-major work.  Row t at depth d is on the path of the sequences s of ONE contiguous range [row_seq_lo[t], row_seq_hi[t]) (callback
// order) with n_s = len_s - 1 >= d.  For each of them it owns the log-prob term (s, j = d - 1) when d >= 1 and the entropy term
// (s, j = d) when d < n_s: every (s, j) is owned by exactly one row in each role, so nothing is scattered and nothing is atomic.
// A thread takes a row; a row whose range is longer than PL_SERIAL sequences is summed by its whole wave, lane-strided over s and
// joined by the xor butterfly - a fixed order either way, so equal inputs give equal bits.
//
// A sequence pass (one workgroup per sequence) goes first and leaves what is one number per sequence; one reduction joins the partials
// of both passes.  The objective's options are forms of the one row term and branches of the one sequence pass:
//   sequence-level ratios (GSPO): every token of sequence s is clipped on r_s = exp(sum_j m_j x_j / n^), so the surrogate's gradient at
//     token t of s is c_s m_t with one scalar c_s per sequence.  The sequence pass walks the sequence's root path - a few contiguous row
//     runs - for r_s, c_s and the surrogate's share of the statistics; the row term takes c_s m for the token's own surrogate gradient;
//   off-policy corrections: a detached rollout importance weight omega, truncated or masked, per token (formed in the row term, from the
//     row's own lp when old_lp is absent) or per sequence (left by the sequence pass, which walks the path only when old_lp is absent),
//     multiplies the surrogate; with a sequence-level ratio it enters c_s;
//   CISPO: a second token-level form of the row term.
//
// Preference objectives (dta_preference_loss: DPO / cDPO / SimPO, SLiC, IPO): a pair couples two sequences, so a pair pass stands
// between the sequence pass (u_s, one number per sequence, over the same path walk) and a row pass that sums g_s m with the pair's
// coefficient g_s; the statistics are per pair and come from the pair pass alone.
//
// The three algorithms the objectives share are written once, with the objective's own terms handed in as functors: the row sweep
// (row_sweep), the root-path walk (path_walk) and the workgroup's row of statistic partials (stat_partials).
#include "dta_common.h"
#include "dta_device.h"
#include <math.h>

namespace {

constexpr int PL_BLOCK = 256;       // rows per workgroup step
constexpr int PL_SERIAL = 16;       // longest sequence range a single thread sums
constexpr int PL_MAX_BLOCKS = 1024; // grid cap: the rest is grid-strided, the partial-sum workspace has at most this many rows
constexpr int PL_NSTAT = 8;         // {loss, sum m pg, sum m kl, sum m entropy, clipped tokens, sum m, 0 | sum m omega, 0 | altered weights}
constexpr int PL_SEQ_BLOCKS = 2048; // grid cap of the sequence pass: one workgroup per sequence, the rest grid-strided

// ---- the shared algorithms -----------------------------------------------------------------------------------------------------

// Row sweep: every row t < T once, a thread per row, the grid striding over steps of PL_BLOCK rows.  load(t) gives the row's own
// values (a Row, its depth d first), term(s, row, sum) adds what the row owns for sequence s to a Sum, store(t, sum) takes the row's
// total over its sequence range [row_lo[t], row_hi[t]), clamped to [0, S).  Row::from_lane(k) is lane k's Row and Sum::wave_total()
// the butterfly sum, for the rows with a range longer than PL_SERIAL: their wave takes them over one after the other, in lane order,
// with every lane - also one whose own row is short or past T - running along, so no lane may leave before the ballot.
// ROOT: the rows of depth 0 own terms too.
template <class Row, class Sum, bool ROOT, class Load, class Term, class Store>
__device__ __forceinline__ void row_sweep(int T, int S, const int32_t* row_lo, const int32_t* row_hi, Load load, Term term, Store store) {
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * PL_BLOCK; base < T; base += gridDim.x * PL_BLOCK) {   // `base` is the same in every lane of the workgroup
    const int t = base + threadIdx.x;
    const bool live = t < T;
    Row row{};
    int s0 = 0, s1 = 0;
    if (live) {
      row = load(t);
      if (ROOT || row.d >= 1) { s0 = max(row_lo[t], 0); s1 = min(row_hi[t], S); }
    }
    const bool wide = s1 - s0 > PL_SERIAL;
    Sum sum{};
    if (!wide)
      for (int s = s0; s < s1; ++s) term(s, row, sum);
    unsigned long long todo = __ballot(wide);
    Sum wsum{};                                            // lane k: the total of its wide row
    while (todo) {
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const Row rk = row.from_lane(k);
      const int b0 = __shfl(s0, k), b1 = __shfl(s1, k);
      Sum r{};
      for (int s = b0 + lane; s < b1; s += 64) term(s, rk, r);
      r = r.wave_total();
      if (lane == k) wsum = r;
    }
    if (live) store(t, wide ? wsum : sum);
  }
}

// the workgroup's sum of v in a fixed order (lanes by butterfly, the four waves in order), in every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                         // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Root-path walk.  Sequence s (predictions [b, b + n) of the per-token inputs) follows the root path of leaf seq_leaf[s]: runs
// [leaf_run_ptr[leaf], leaf_run_ptr[leaf + 1]) of contiguous packed rows, run k starting at row run_row0[k] with depth run_depth0[k].
// Prediction j of s is the row of depth j + 1: f(t, i) is called for every row t < T of depth >= 1 on the path, with i = b + depth - 1,
// the workgroup's threads striding over each run.
struct PathParams {
  const float* lp;
  const int32_t *seq_ptr, *leaf_run_ptr, *run_row0, *run_depth0, *seq_leaf;
  int32_t T, S, M, R;
};

template <class F>
__device__ __forceinline__ void path_walk(const PathParams& p, int s, int b, int n, F f) {
  const int leaf = min(max(p.seq_leaf[s], 0), p.M - 1);
  const int k0 = max(p.leaf_run_ptr[leaf], 0), k1 = min(p.leaf_run_ptr[leaf + 1], p.R);
  for (int k = k0; k < k1; ++k) {
    const int row0 = p.run_row0[k], d0 = p.run_depth0[k];
    const int da = max(d0, 1), db = min(k + 1 < k1 ? p.run_depth0[k + 1] : n + 1, n + 1);         // depths [da, db) of this run
    for (int d = da + (int)threadIdx.x; d < db; d += 256) {
      const int t = row0 + (d - d0);
      if (t < 0 || t >= p.T) continue;
      f(t, b + d - 1);
    }
  }
}

// The workgroup's row of statistic partials from every thread's st[N]: lanes by butterfly, then the four waves in order from 0.f;
// all PL_NSTAT columns of the row are written, the ones from N on with 0.
template <int N>
__device__ __forceinline__ void stat_partials(const float (&st)[N], float* partial) {
  __shared__ float red[PL_BLOCK / 64][PL_NSTAT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < N; ++i) {
    const float v = wave_sum(st[i]);
    if (lane == 0) red[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < PL_NSTAT) {
    float v = 0.f;
    if (threadIdx.x < N)
      for (int wv = 0; wv < PL_BLOCK / 64; ++wv) v += red[wv][threadIdx.x];
    partial[blockIdx.x * PL_NSTAT + threadIdx.x] = v;
  }
}

// ---- policy objective (dta_policy_loss) --------------------------------------------------------------------------------------------

struct PolicyParams {
  const float *lp, *ent;
  const int32_t *depth, *row_lo, *row_hi, *seq_ptr;
  const float *old_lp, *ref_lp, *rollout, *mask, *adv;
  const float *w, *c, *omega;                // per sequence, left by the sequence pass: the weight, the sequence-level surrogate's gradient
                                             // scalar, the sequence-level rollout weight
  float *dlp, *dent, *partial;
  int32_t T, S, adv_per_seq, is_mode;
  float lo, hi, dual, kl_coef, ent_coef, is_cap, is_floor;     // lo = 1 - clip_low, hi = 1 + clip_high, dual = 0: none
};

// a row's own values, and what it receives: dlp and dent
struct PolicyRow {
  int d; float lp, ent;
  __device__ PolicyRow from_lane(int k) const { return {__shfl(d, k), __shfl(lp, k), __shfl(ent, k)}; }
};
// a thread's share of the statistics.  (A struct: a bare private array that loops index becomes one vector value before the loops are
// unrolled, and the columns an instantiation never touches then no longer fold to constants.)
struct PolicyStats { float v[PL_NSTAT]; };
struct PolicySum {
  float glp, gent;
  __device__ PolicySum wave_total() const { return {wave_sum(glp), wave_sum(gent)}; }
};

// the clipped surrogate of one token from its ratio r and advantage A; `clipped`: a clamp is the active branch, d pg / d lp = 0
struct Pg { float pg; bool clipped; };
__device__ __forceinline__ Pg clipped_pg(float r, float lo, float hi, float A, float dual) {
  const float s1 = -r * A, s2 = -fminf(fmaxf(r, lo), hi) * A;
  float pg = fmaxf(s1, s2);
  bool clipped = s2 > s1;
  if (dual > 0.f && A < 0.f) {
    const float cap = -dual * A;
    if (cap < pg) { pg = cap; clipped = true; }
  }
  return {pg, clipped};
}

// the KL estimate from dd = ref - lp, and dk = d kl / d lp
template <int KL>
__device__ __forceinline__ float kl_term(float dd, float& dk) {
  if (KL == 0) { dk = 1.f; return -dd; }
  if (KL == 1) { dk = -dd; return 0.5f * dd * dd; }
  const float e = expf(dd);
  dk = 1.f - e;
  return e - dd - 1.f;
}

// the rollout weight omega from rho: mode 0 truncates at cap, mode 1 drops what lies outside [floor, cap].  No arithmetic on rho: an
// overflowed expf (inf) gives cap or 0 and never NaN.  `altered`: omega != rho.
struct IsWeight { float omega; bool altered; };
__device__ __forceinline__ IsWeight is_weight(float rho, int mode, float cap, float floor) {
  if (mode == 0) {
    const bool over = rho > cap;
    return {over ? cap : rho, over};
  }
  const bool keep = rho >= floor && rho <= cap;
  return {keep ? rho : 0.f, !keep};
}

// the surrogate's form in the row term
constexpr int PL_CLIPPED = 0;       // the clipped surrogate on the token's own ratio
constexpr int PL_CISPO = 1;         // pg = -clamp(r) A lp with the clamp detached: the gradient -clamp(r) A is never zeroed, "clipped"
                                    // counts r outside [lo, hi]
constexpr int PL_SEQ_RATIO = 2;     // a sequence-level ratio: the gradient is c_s m, value and statistics are the sequence pass's

// The terms a row owns for sequence s.  ISL (the token-level forms): 0 no rollout weight, 1 a weight per token formed here, 2 the
// sequence's weight omega[s]; columns 6 and 7 of the statistics are the sequence pass's under ISL 2 and under PL_SEQ_RATIO.
template <int KL, int FORM, int ISL>
__device__ __forceinline__ void policy_terms(const PolicyParams& p, int s, const PolicyRow& row, PolicySum& a, PolicyStats& st) {
  const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b, d = row.d;
  if (n < d) return;                                       // the sequence ends above this row
  const float w = p.w[s];
  if (d >= 1) {                                            // the log-prob term (s, j = d - 1)
    const int i = b + d - 1;
    const float m = p.mask[i];
    if (FORM == PL_SEQ_RATIO) {
      float g = p.c[s] * m;
      if (KL >= 0) {
        float dk;
        const float kl = kl_term<KL>(p.ref_lp[i] - row.lp, dk);
        const float wm = w * m;
        g += wm * (p.kl_coef * dk);
        st.v[0] += wm * (p.kl_coef * kl);
        st.v[2] += m * kl;
      }
      a.glp += g;
    } else {
      const float A = p.adv[p.adv_per_seq ? s : i];
      const float r = p.old_lp ? expf(row.lp - p.old_lp[i]) : 1.f;
      float pg, g;
      bool clipped;
      if (FORM == PL_CLIPPED) {
        const Pg q = clipped_pg(r, p.lo, p.hi, A, p.dual);
        pg = q.pg; clipped = q.clipped;
        g = clipped ? 0.f : -r * A;                        // d(-r A)/d lp = -r A
      } else {
        g = -fminf(fmaxf(r, p.lo), p.hi) * A;
        pg = g * row.lp;
        clipped = r < p.lo || r > p.hi;
      }
      if (ISL == 1) {
        const float y = (p.old_lp ? p.old_lp[i] : row.lp) - p.rollout[i];
        const auto [omega, altered] = is_weight(expf(y), p.is_mode, p.is_cap, p.is_floor);
        pg *= omega; g *= omega;
        st.v[6] += m * omega;
        st.v[7] += altered ? m : 0.f;
      } else if (ISL == 2) {
        const float omega = p.omega[s];
        pg *= omega; g *= omega;
      } else if (FORM == PL_CISPO) {
        st.v[6] += m;                                      // omega == 1 (the clipped form: column 5, copied after the sweep)
      }
      float kl = 0.f;
      if (KL >= 0) {
        float dk;
        kl = kl_term<KL>(p.ref_lp[i] - row.lp, dk);
        g += p.kl_coef * dk;
        st.v[2] += m * kl;
      }
      const float wm = w * m;
      a.glp += wm * g;
      st.v[0] += wm * (pg + p.kl_coef * kl);
      st.v[1] += m * pg;
      st.v[4] += clipped ? m : 0.f;
    }
    st.v[5] += m;
  }
  if (d < n) {                                             // the entropy term (s, j = d)
    const float m = p.mask[b + d];
    const float wm = w * m;
    a.gent -= wm * p.ent_coef;
    st.v[0] -= wm * p.ent_coef * row.ent;
    st.v[3] += m * row.ent;
  }
}

template <int KL, int FORM, int ISL>
__global__ __launch_bounds__(PL_BLOCK) void policy_loss_kernel(const PolicyParams p) {
  PolicyStats st = {};                                     // this thread's share of the statistics, over all its rows
  row_sweep<PolicyRow, PolicySum, true>(
      p.T, p.S, p.row_lo, p.row_hi, [&](int t) { return PolicyRow{p.depth[t], p.lp[t], p.ent[t]}; },
      [&](int s, const PolicyRow& row, PolicySum& a) { policy_terms<KL, FORM, ISL>(p, s, row, a, st); },
      [&](int t, const PolicySum& a) { p.dlp[t] = a.glp; p.dent[t] = a.gent; });
  // omega == 1: sum m omega has the addends of sum m, in their order.  Copied here, not added per term: a seventh accumulator in the loop
  // changes how the compiler contracts the clipped form's neighbouring products, and with it the last bits of dlp.
  if (FORM == PL_CLIPPED && ISL == 0) st.v[6] = st.v[5];
  stat_partials(st.v, p.partial);
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

// The sequence pass: w[s], omega[s] and c[s] of every sequence, and its workgroup's row of partials - the surrogate's columns under a
// sequence-level ratio, columns 6 and 7 under a sequence-level ratio or a sequence-level weight, 0 everywhere else.
struct SeqPassParams : PathParams {
  const float *old_lp, *rollout, *mask, *adv;
  float *w, *c, *omega, *partial;
  int32_t adv_per_seq, seq_mean, ratio_seq, is_level, is_mode;     // is_level: 0 none, 1 token, 2 sequence, 3 sequence_mean
  float lo, hi, dual, scale, is_cap, is_floor;
};

__global__ __launch_bounds__(256) void policy_seq_pass_kernel(const SeqPassParams p) {
  __shared__ float red[4];
  float st_loss = 0.f, st_pg = 0.f, st_clip = 0.f, st_om = 0.f, st_alt = 0.f;     // thread 0: this workgroup's sequences, in order
  const bool need_x = p.ratio_seq && p.old_lp, need_y = p.is_level >= 2;
  const bool need_m = p.seq_mean || p.ratio_seq || need_y;                        // something reads the sequence's sum of the mask
  for (int s = blockIdx.x; s < p.S; s += gridDim.x) {      // `s` is the same in every thread of the workgroup
    const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
    float sm = 0.f, sx = 0.f, sy = 0.f;
    if (need_x || (need_y && !p.old_lp)) {                 // something reads the rows' lp: the path is walked
      path_walk(p, s, b, n, [&](int t, int i) {
        const float m = p.mask[i], lpt = p.lp[t];
        sm += m;
        if (need_x) sx += m * (lpt - p.old_lp[i]);
        if (need_y) sy += m * ((p.old_lp ? p.old_lp[i] : lpt) - p.rollout[i]);
      });
    } else if (need_m) {                                   // kernel arguments alone decide: the whole grid takes one side
      for (int j = threadIdx.x; j < n; j += 256) {
        const float m = p.mask[b + j];
        sm += m;
        if (need_y) sy += m * (p.old_lp[b + j] - p.rollout[b + j]);
      }
    }
    const float nm = block_sum(sm, red), nh = fmaxf(nm, 1.f);
    const float r = need_x ? expf(block_sum(sx, red) / nh) : 1.f;
    const float w = p.seq_mean ? p.scale / nh : p.scale;
    IsWeight ws = {1.f, false};
    if (need_y) {
      const float e = block_sum(sy, red);
      ws = is_weight(expf(p.is_level == 3 ? e / nh : e), p.is_mode, p.is_cap, p.is_floor);
    }
    float spg = 0.f, sg = 0.f, sc = 0.f, so = 0.f, sa = 0.f;
    if (p.ratio_seq) {
      // every token of the sequence sees the same r: its branch depends on the sign of its advantage alone
      auto token = [&](float lpt, int i) {
        const float m = p.mask[i];
        const float A = p.adv[p.adv_per_seq ? s : i];
        const auto [pg, clipped] = clipped_pg(r, p.lo, p.hi, A, p.dual);
        IsWeight wt = ws;
        if (p.is_level == 1) wt = is_weight(expf((p.old_lp ? p.old_lp[i] : lpt) - p.rollout[i]), p.is_mode, p.is_cap, p.is_floor);
        spg += m * (wt.omega * pg);
        sg += clipped ? 0.f : m * (wt.omega * -A);
        sc += clipped ? m : 0.f;
        so += m * wt.omega;
        sa += wt.altered ? m : 0.f;
      };
      if (p.is_level == 1 && !p.old_lp) path_walk(p, s, b, n, [&](int t, int i) { token(p.lp[t], i); });
      else for (int j = threadIdx.x; j < n; j += 256) token(0.f, b + j);
      spg = block_sum(spg, red); sg = block_sum(sg, red); sc = block_sum(sc, red);
      so = block_sum(so, red); sa = block_sum(sa, red);
    } else if (need_y) {
      so = nm * ws.omega; sa = ws.altered ? nm : 0.f;
    }
    if (threadIdx.x == 0) {
      p.w[s] = w;
      p.omega[s] = ws.omega;
      p.c[s] = p.ratio_seq ? w * r / nh * sg : 0.f;
      st_loss += w * spg; st_pg += spg; st_clip += sc; st_om += so; st_alt += sa;
    }
  }
  if (threadIdx.x == 0) {                                  // this workgroup's row of the partial sums
    float* out = p.partial + (size_t)blockIdx.x * PL_NSTAT;
    out[0] = st_loss; out[1] = st_pg; out[2] = 0.f; out[3] = 0.f; out[4] = st_clip; out[5] = 0.f; out[6] = st_om; out[7] = st_alt;
  }
}

// ---- preference objectives (dta_preference_loss): DPO / cDPO / SimPO, SLiC, IPO --------------------------------------------------
// A pair couples two sequences, so there is a pair stage between a sequence pass and a row pass: the sequence pass leaves one
// number u_s per sequence, the pair pass turns the two numbers of a pair into one coefficient g_s per member, and the row pass sums
// g_s m over the sequences through a row - the same row-major ownership as above, with nothing but the mask to read per term.

constexpr int PF_MAX_BLOCKS = 1024; // grid cap of the pair pass: one thread per pair, the rest grid-strided; one partial row per workgroup

struct PrefSeqParams : PathParams {
  const float *ref_lp, *ref_sum, *mask;
  float *nhat, *u, *sft, *g;
  int32_t length_normalize;
};

// n^_s, u_s and P_s / n^_s of every sequence, and g_s = 0 (the pair pass overwrites the members of a pair)
__global__ __launch_bounds__(256) void preference_seq_pass_kernel(const PrefSeqParams p) {
  __shared__ float red[4];
  for (int s = blockIdx.x; s < p.S; s += gridDim.x) {      // `s` is the same in every thread of the workgroup
    const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
    float sm = 0.f, sp = 0.f, sf = 0.f;
    path_walk(p, s, b, n, [&](int t, int i) {
      const float m = p.mask[i];
      sm += m;
      sp += m * p.lp[t];
      if (p.ref_lp) sf += m * p.ref_lp[i];
    });
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
  float st[PL_NSTAT] = {};
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
  stat_partials(st, p.partial);
}

struct PrefRowParams {
  const int32_t *depth, *row_lo, *row_hi, *seq_ptr;
  const float *mask, *g;
  float* dlp;
  int32_t T, S;
};

struct PrefRow {
  int d;
  __device__ PrefRow from_lane(int k) const { return {__shfl(d, k)}; }
};
struct PrefSum {
  float v;
  __device__ PrefSum wave_total() const { return {wave_sum(v)}; }
};

// dlp for every row: the term a row of depth d >= 1 owns for sequence s is g_s m at prediction d - 1; a row of depth 0 owns none
__global__ __launch_bounds__(PL_BLOCK) void preference_row_kernel(const PrefRowParams p) {
  row_sweep<PrefRow, PrefSum, false>(
      p.T, p.S, p.row_lo, p.row_hi, [&](int t) { return PrefRow{p.depth[t]}; },
      [&](int s, const PrefRow& row, PrefSum& a) {
        const int b = p.seq_ptr[s], n = p.seq_ptr[s + 1] - b;
        a.v += n < row.d ? 0.f : p.g[s] * p.mask[b + row.d - 1];
      },
      [&](int t, const PrefSum& a) { p.dlp[t] = a.v; });
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

// the row kernels of one (surrogate form, weight level), by KL estimator: none, k1, k2, k3
typedef void (*PolicyRowKernel)(const PolicyParams);
template <int FORM, int ISL>
constexpr PolicyRowKernel policy_row_kernels[4] = {policy_loss_kernel<-1, FORM, ISL>, policy_loss_kernel<0, FORM, ISL>,
                                                   policy_loss_kernel<1, FORM, ISL>, policy_loss_kernel<2, FORM, ISL>};

}  // namespace

extern "C" int dta_policy_loss_blocks(int32_t T, int32_t S) {
  return T <= 0 || S <= 0 ? DTA_EINVAL : row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS) + (S < PL_SEQ_BLOCKS ? S : PL_SEQ_BLOCKS);
}

extern "C" int dta_policy_loss(const float* lp, const float* ent, const int32_t* depth, const int32_t* row_seq_lo, const int32_t* row_seq_hi,
                               const int32_t* seq_ptr, const int32_t* leaf_run_ptr, const int32_t* run_row0, const int32_t* run_depth0,
                               const int32_t* seq_leaf, const float* old_lp, const float* ref_lp, const float* rollout_lp, const float* mask,
                               const float* adv, int32_t adv_per_seq, float* w, float* c, float* omega, float* dlp, float* dent,
                               float* partial, float* stats, int32_t T, int32_t S, int32_t M, int32_t R, float clip_low, float clip_high,
                               float dual_clip, float kl_coef, int32_t kl_estimator, float entropy_coef, int32_t agg, float scale,
                               int32_t ratio_level, int32_t surrogate, int32_t is_level, int32_t is_mode, float is_cap, float is_floor,
                               void* stream) {
  if (!lp || !ent || !depth || !row_seq_lo || !row_seq_hi || !seq_ptr || !mask || !adv || !w || !c || !omega || !dlp || !dent || !partial ||
      !stats || T <= 0 || S <= 0)
    return DTA_EINVAL;
  if (!finite_f(clip_low) || !finite_f(clip_high) || clip_low < 0.f || clip_high < 0.f) return DTA_EINVAL;
  if (dual_clip != 0.f && !(finite_f(dual_clip) && dual_clip > 1.f)) return DTA_EINVAL;
  if (kl_estimator < 0 || kl_estimator > 2 || agg < 0 || agg > 1) return DTA_EINVAL;
  if (!finite_f(kl_coef) || !finite_f(entropy_coef) || !finite_f(scale)) return DTA_EINVAL;
  if (kl_coef != 0.f && !ref_lp) return DTA_EINVAL;
  if (ratio_level < 0 || ratio_level > 1 || surrogate < 0 || surrogate > 1 || is_level < 0 || is_level > 3 || is_mode < 0 || is_mode > 1)
    return DTA_EINVAL;
  if (!finite_f(is_cap) || !(is_cap > 0.f) || !finite_f(is_floor) || is_floor < 0.f || !(is_floor < is_cap)) return DTA_EINVAL;
  if (is_mode == 0 && is_floor != 0.f) return DTA_EINVAL;
  if (surrogate == 1 && (ratio_level == 1 || dual_clip != 0.f)) return DTA_EINVAL;
  if (is_level != 0 && !rollout_lp) return DTA_EINVAL;
  const bool walks = ratio_level == 1 || (is_level >= 2 && !old_lp);       // something follows a root path
  if (walks && (!leaf_run_ptr || !run_row0 || !run_depth0 || !seq_leaf || M <= 0 || R <= 0)) return DTA_EINVAL;
  if (!all_aligned16(lp, ent, depth, row_seq_lo, row_seq_hi, seq_ptr, leaf_run_ptr, run_row0, run_depth0, seq_leaf, old_lp, ref_lp, rollout_lp,
                     mask, adv, w, c, omega, dlp, dent, partial, stats))
    return DTA_EALIGN;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  const int nb = row_blocks(T, PL_BLOCK, PL_MAX_BLOCKS), nsb = S < PL_SEQ_BLOCKS ? S : PL_SEQ_BLOCKS;
  if (is_level == 0) rollout_lp = nullptr;                                  // not read
  SeqPassParams q;
  static_cast<PathParams&>(q) = {lp, seq_ptr, leaf_run_ptr, run_row0, run_depth0, seq_leaf, T, S, walks ? M : 0, walks ? R : 0};
  q.old_lp = old_lp; q.rollout = rollout_lp; q.mask = mask; q.adv = adv; q.w = w; q.c = c; q.omega = omega;
  q.partial = partial + (size_t)nb * PL_NSTAT;                              // its partial rows stand behind the row pass's
  q.adv_per_seq = adv_per_seq != 0; q.seq_mean = agg == 0; q.ratio_seq = ratio_level; q.is_level = is_level; q.is_mode = is_mode;
  q.lo = 1.f - clip_low; q.hi = 1.f + clip_high; q.dual = dual_clip; q.scale = scale; q.is_cap = is_cap; q.is_floor = is_floor;
  hipLaunchKernelGGL(policy_seq_pass_kernel, dim3(nsb), dim3(256), 0, st_, q);
  PolicyParams p;
  p.lp = lp; p.ent = ent; p.depth = depth; p.row_lo = row_seq_lo; p.row_hi = row_seq_hi; p.seq_ptr = seq_ptr;
  p.old_lp = ratio_level ? nullptr : old_lp; p.ref_lp = kl_coef != 0.f ? ref_lp : nullptr; p.rollout = rollout_lp; p.mask = mask; p.adv = adv;
  p.w = w; p.c = c; p.omega = omega; p.dlp = dlp; p.dent = dent; p.partial = partial;
  p.T = T; p.S = S; p.adv_per_seq = q.adv_per_seq; p.is_mode = is_mode;
  p.lo = q.lo; p.hi = q.hi; p.dual = dual_clip; p.kl_coef = kl_coef; p.ent_coef = entropy_coef; p.is_cap = is_cap; p.is_floor = is_floor;
  // one instantiation per (KL, surrogate form, weight level); under a sequence-level ratio c_s holds the weight
  static constexpr const PolicyRowKernel* rows[3][3] = {
      {policy_row_kernels<PL_CLIPPED, 0>, policy_row_kernels<PL_CLIPPED, 1>, policy_row_kernels<PL_CLIPPED, 2>},
      {policy_row_kernels<PL_CISPO, 0>, policy_row_kernels<PL_CISPO, 1>, policy_row_kernels<PL_CISPO, 2>},
      {policy_row_kernels<PL_SEQ_RATIO, 0>, policy_row_kernels<PL_SEQ_RATIO, 0>, policy_row_kernels<PL_SEQ_RATIO, 0>}};
  const PolicyRowKernel row_kernel = rows[ratio_level ? PL_SEQ_RATIO : surrogate][is_level >= 2 ? 2 : is_level][kl_coef == 0.f ? 0 : kl_estimator + 1];
  hipLaunchKernelGGL(row_kernel, dim3(nb), dim3(PL_BLOCK), 0, st_, p);
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
  if (!all_aligned16(lp, depth, row_seq_lo, row_seq_hi, seq_ptr, leaf_run_ptr, run_row0, run_depth0, seq_leaf, pair_c, pair_r, mask, nhat, u,
                     sft, g, dlp, partial, stats, ref_lp, ref_sum))
    return DTA_EALIGN;
  hipStream_t st_ = static_cast<hipStream_t>(stream);
  DTA_REFUSE_IF_PRIOR_ERROR();
  PrefSeqParams q;
  static_cast<PathParams&>(q) = {lp, seq_ptr, leaf_run_ptr, run_row0, run_depth0, seq_leaf, T, S, M, R};
  q.ref_lp = ref_lp; q.ref_sum = ref_sum; q.mask = mask; q.nhat = nhat; q.u = u; q.sft = sft; q.g = g;
  q.length_normalize = length_normalize != 0;
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
