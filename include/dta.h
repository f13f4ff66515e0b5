/*
 * dta.h — C ABI of libdta_mi355x.so: the MI355X (gfx950) tree-attention hot path of DynamicTreeAttn.
 *
 * The reference (/root/reference, 17 Python files) has NO native code and therefore no FFI; these
 * entry points are what a binding for its hot path would call.  Each one names the reference
 * interface it replaces (file:line into /root/reference).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions: raw device pointers + sizes + a hipStream_t passed as void*;
 * returns 0 on success, a negative DTA_E* code on invalid arguments (nothing is launched then);
 * no allocation, no ownership transfer, no global state, re-entrant across streams.  All
 * launches are asynchronous on `stream`.  Device code exists for gfx950 only.
 *
 * Packed-trie vocabulary: the T tokens of a trie are laid out in DFS pre-order of its leaves
 * ("packed order"): leaf i contributes the segment of its tokens at depths [lcp[i-1], len[i]).
 * For packed token s, subtree_end[s] is one past its last descendant, so
 *     s is an ancestor-or-self of t   <=>   s <= t < subtree_end[s].
 */
#ifndef DTA_H
#define DTA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTA_OK 0
#define DTA_EINVAL (-1)      /* null pointer / negative size / inconsistent sizes */
#define DTA_EUNSUPPORTED (-2)/* head_dim not 64 / 128, dtype not bf16/f16/f32, Hq % Hkv != 0, accumulate not 0..2 ... */
#define DTA_EALIGN (-3)      /* pointer or stride not 16-byte aligned */
#define DTA_ELAUNCH (-4)     /* hipGetLastError() after the launch was not hipSuccess */
#define DTA_EPRIOR (-5)      /* a HIP error was ALREADY pending on this thread when the entry point was called (an earlier
                              * asynchronous kernel fault or an unchecked runtime call): nothing was launched and the error
                              * is left in place; dta_take_pending_error() names and clears it */

#define DTA_BF16 0
#define DTA_F16 1
#define DTA_F32 2            /* fp32 models (reference --dtype fp32, run.py:122-132): plain-FMA attention kernels (a gradient-check path, not a
                              * performance path), fp32 row kernels; and fp32 logits of the log-prob / entropy kernels (vocab_parallel.py:16,24) */

#define DTA_QTILE 128        /* query rows per workgroup (fwd / dQ kernels)  */
#define DTA_KTILE 128        /* key rows per workgroup (dK/dV kernel): 8 waves = 2 groups x (4 waves x 32 keys) sharing the keys */

int dta_version(void);

/* Name (into msg[cap], NUL-terminated) and CLEAR the HIP error pending on the calling thread; returns its hipError_t value
 * (0 = none).  After an asynchronous kernel fault the context stays unusable - clearing only lets the caller report it. */
int dta_take_pending_error(char* msg, int32_t cap);

/* ---------------------------------------------------------------------------------------------
 * Trie build kernels (integer, bit-exact, HBM-bound)
 * ------------------------------------------------------------------------------------------- */

/* Adjacent longest-common-prefix of S sequences held in one int64 `tokens` buffer: sequence i (in
 * the order to be compared) is tokens[starts[i] .. starts[i]+lens[i]).  out_lcp[i] = lcp(seq i,
 * seq i+1); *out_unsorted += number of adjacent pairs that violate lexicographic order
 * (seq_i[lcp] > seq_{i+1}[lcp]).  The caller zeroes out_unsorted.  S = 0 or 1: nothing to compare, DTA_OK.
 * Replaces token_trie.py:6-10 (_lcp_torch), the order check token_trie.py:24-30 and the
 * recomputation after a permutation, token_trie.py:94.  */
int dta_lcp_adjacent(const int64_t* tokens, const int64_t* starts, const int32_t* lens, int32_t S,
                     int32_t* out_lcp, int32_t* out_unsorted, void* stream);

/* Leafization as a stream compaction over the S sorted sequences: keep[i] = (i == S-1) ||
 * lcp[i] < min(len[i], len[i+1]).  Writes the kept positions (ascending) to out_leaf_pos, the
 * leaf's LCP with the next leaf to out_leaf_lcp, for every sequence the leaf it folds onto to
 * out_seq_leaf[S] (lens[S] = sequence lengths in sorted order), and the leaf count to *out_M.  One workgroup (S <= 2^20).
 * The caller sizes out_leaf_pos for S and out_leaf_lcp for S-1 entries; M and M-1 of them are written, the rest is left untouched.
 * Replaces token_trie.py:32-49 (_leafization, second half).  */
int dta_leafize(const int32_t* lens, const int32_t* lcp, int32_t S,
                int32_t* out_leaf_pos, int32_t* out_leaf_lcp, int32_t* out_seq_leaf, int32_t* out_M,
                void* stream);

/* Packed pre-order metadata for M leaves visited in the given DFS order.  Inputs per leaf i:
 * seg_off[i] (packed offset of its segment; seg_off[M] = T), seg_depth0[i] = lcp[i-1] (0 for i=0),
 * leaf_tok_off[i] = offset of the leaf's tokens in `tokens`; and the per-segment "closing" table
 * brk_ptr[M+1], brk_depth[], brk_end[]: tokens of segment i at depth d in
 * [brk_depth[j], brk_depth[j+1]) have subtree_end = brk_end[j].  parent_of_seg[i] = packed index of
 * the token at depth seg_depth0[i]-1 on leaf i's path (-1 when seg_depth0[i] == 0).
 * Outputs per packed token: token id, depth (= RoPE position, the stack position of
 * tree_training_engine.py:166,293), parent index, subtree_end.
 * Replaces the per-leaf H2D copy + stack bookkeeping of tree_training_engine.py:536-548, 582-611. */
int dta_preorder_meta(const int64_t* tokens, const int64_t* leaf_tok_off,
                      const int32_t* seg_off, const int32_t* seg_depth0, const int32_t* parent_of_seg,
                      const int32_t* brk_ptr, const int32_t* brk_depth, const int32_t* brk_end,
                      int32_t M, int32_t T,
                      int64_t* out_token, int32_t* out_depth, int32_t* out_parent, int32_t* out_subtree_end,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tree attention (MFMA-bound).  One forward / backward pair serves packed tries and the stack form, with or without a sliding window
 * and a soft-cap: window <= 0 and softcap <= 0 select the kernels compiled without those terms.
 * head_dim 128 or 64; dtype DTA_BF16 or DTA_F16 (MFMA kernels), or DTA_F32 (every buffer fp32; plain fp32 FMAs, one workgroup per
 * 64 rows, split-Q work units ignored - the correctness path of fp32 models).
 *
 * Layout.  q/out/dout/dq: [Tq, Hq, head_dim], k/v/dk/dv: [Tk, Hkv, head_dim], rows of head_dim contiguous elements; every token and
 * head stride is explicit (elements), so that head-major layouts such as the reference's [1, H, S, D] KV stack
 * (tree_training_engine.py:108-131) work in place.  Alignment: every base pointer 16 bytes, every stride a multiple of 8 elements
 * (DTA_EALIGN otherwise) - a head row is 256 B (D = 128) or 128 B (D = 64), i.e. whole 16-byte chunks either way.  Token strides of k
 * and v (forward) and of q and dout (backward) must be in [0, 2^24] elements on the MFMA path: a 64-row tile is addressed as scalar
 * base + 32-bit lane offset by the tile DMA (DTA_EUNSUPPORTED otherwise).
 *
 * Visibility.  Query row i has packed index t = q_offset + i.  It attends key s iff
 *   packed trie:  s <= t  &&  t < subtree_end[s]  (the ancestor test)
 *   stack form (subtree_end == NULL): s <= t, no upper bound - the rectangular-causal form of tree_training_engine.py:171-186 with
 *                 q_offset = start
 * and, with window > 0 (the "sliding_attention" layers of Qwen2 / Qwen3 configurations), one lower bound more:
 *   packed trie:  s >= win_lo[i],  win_lo[i] = packed index of t's ancestor at depth max(0, depth[t] - window + 1) (dta_window_lo), i.e.
 *                 depth[t] - depth[s] < window along the path: the mask of HF's sliding_window_overlay for every sequence through t.
 *   stack form (win_lo == NULL):  t - s < window.
 * window <= 0: no window, and win_lo must be NULL.  DTA_EINVAL: win_lo given with window <= 0, or subtree_end given (packed trie)
 * with window > 0 and no win_lo.
 *
 * Query tiles are DTA_QTILE rows.  Tile j visits the key runs runs[run_ptr[j] .. run_ptr[j+1]),
 * each run = 4 int32 {key_begin, key_end, needs_mask, 0}; runs == NULL: one run [0, last row + 1).
 * A run with needs_mask == 0 promises that every key in it is visible to every row of the tile.  With a window, run_ptr / runs of a
 * packed trie must be planned for the window: needs_mask == 0 then promises that the run's keys are ancestors of every row of the tile
 * AND >= every row's win_lo (the windowed plan of packing.plan_qtile_runs_window); ktile_qend and dkv_units may be the windowed,
 * tighter ones.
 *
 * Soft-cap (Gemma-2's attn_logit_softcapping), softcap > 0.  With z_ij = scale * (q_i . k_j), c = softcap and t_ij = tanh(z_ij / c):
 *   forward   s_ij = c * t_ij.  The cap comes FIRST, then the visibility mask (ancestor test, window), then the softmax - the order of
 *             HF's eager_attention_forward.
 *   backward  t is recomputed from Q.K^T as S is; p = exp(s - lse) and dS = p * (dP - delta) as without a cap;
 *             dz = dS * (1 - t^2);  dq = scale * dz K,  dk = scale * dz^T Q;  dV and delta are unchanged.
 * tanh is computed in fp32 as 1 - 2 / (1 + 2^(2 log2(e) z / c)): it saturates to +-1 for large |z / c| (no inf / inf) and its absolute
 * error is a few 2^-24, i.e. the capped score is off by the order of c * 2^-24.  softcap <= 0: no cap.  DTA_EINVAL: a softcap that is
 * NaN or infinite.
 *
 * lse: [Hq, Tq] float (head-major), log2-domain log-sum-exp of the scaled scores - of the CAPPED scores under a soft-cap
 * (natural lse = lse * ln 2).
 *
 * Refusals of both entries come in this order: DTA_EINVAL for the soft-cap, then for the window rules, then for a null pointer, a size
 * <= 0 or q_offset < 0, runs without run_ptr (or the reverse) and, in the backward, inconsistent dkv_units arguments or a `which`
 * without any of bits 0-2; DTA_EUNSUPPORTED for head_dim, Hq % Hkv != 0, dtype or accumulate; DTA_EALIGN; DTA_EUNSUPPORTED for the
 * 2^24 token-stride limit; DTA_EPRIOR.
 * Replaces the attention the reference reaches through the model call,
 * tree_training_engine.py:182-186, 248-252, 351-353 (third-party attention backend).  */
int dta_tree_attn_fwd(const void* q, const void* k, const void* v, void* out, float* lse,
                      const int32_t* subtree_end, const int32_t* run_ptr, const int32_t* runs,
                      int32_t Tq, int32_t Tk, int32_t q_offset, int32_t Hq, int32_t Hkv, int32_t head_dim,
                      int64_t q_stride_t, int64_t q_stride_h, int64_t k_stride_t, int64_t k_stride_h,
                      int64_t v_stride_t, int64_t v_stride_h,
                      int64_t o_stride_t, int64_t o_stride_h, float scale, int32_t dtype,
                      const int32_t* win_lo, int32_t window, float softcap, void* stream);

/* Backward.  Two launches on `stream`: (1) per query tile: delta = rowsum(dout*out), dq;
 * (2) per key tile of DTA_KTILE keys: dk, dv summed over the query range
 * [max(key0, q_offset), ktile_qend[tile]) and over the Hq/Hkv query heads of the group — no
 * cross-workgroup reduction, no atomics, bitwise reproducible (with a window and a soft-cap too).  ktile_qend[j] = max subtree_end
 * over the tile's keys (NULL: q_offset + Tq).  `accumulate`: 0 overwrites dk/dv; 1 adds into them (the grad-KV
 * stack of tree_training_engine.py:447-451; model dtype, rounded after every add as the reference's `+=`); 2 adds into
 * FP32 buffers (dk/dv are float*, strides in floats) so that the hundreds of adds a root-side row receives in the
 * block-wise engine are not rounded to 16 bits each time.  delta: [Hq, Tq] float workspace.
 * Visibility, window, soft-cap, layout and alignment are the forward's.
 * Replaces torch.autograd.backward through the attention backend, tree_training_engine.py:440.  */
int dta_tree_attn_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                      const float* lse, float* delta, void* dq, void* dk, void* dv,
                      const int32_t* subtree_end, const int32_t* run_ptr, const int32_t* runs,
                      const int32_t* ktile_qend,
                      int32_t Tq, int32_t Tk, int32_t q_offset, int32_t Hq, int32_t Hkv, int32_t head_dim,
                      int64_t q_stride_t, int64_t q_stride_h, int64_t k_stride_t, int64_t k_stride_h,
                      int64_t v_stride_t, int64_t v_stride_h,
                      int64_t o_stride_t, int64_t o_stride_h, int64_t dq_stride_t, int64_t dq_stride_h,
                      int64_t dkv_stride_t, int64_t dkv_stride_h,
                      float scale, int32_t dtype, int32_t accumulate,
                      int32_t which /* bit0: delta+dq launch, bit1: dk/dv launch (needs delta) followed by the slab finalize
                                       unless bit3; bit2: slab finalize alone (lets a profiler bracket each launch);
                                       none of bits 0-2: DTA_EINVAL */,
                      /* optional split of the dK/dV sweep into balanced work units (NULL: one per key tile):
                       * dkv_units[u] = {key tile, q_begin, q_end (packed), slab or -1}; units of a split key tile
                       * write fp32 slabs [2][DTA_KTILE][head_dim] into dkv_ws (slab-major, then kv head) which a finalize
                       * launch sums in order: dkv_splits[s] = {key tile, first slab, n slabs, 0}. */
                      const int32_t* dkv_units, int32_t n_units, const int32_t* dkv_splits, int32_t n_splits, float* dkv_ws,
                      const int32_t* win_lo, int32_t window, float softcap, void* stream);

/* out_win_lo[t] for the T packed tokens of a trie: the packed index of t's ancestor at depth max(0, depth[t] - window + 1).  depth[T] as
 * written by dta_preorder_meta; seg_off[M+1], seg_depth0[M], parent_of_seg[M] as passed to it.  Walks up segments (binary search over
 * seg_off per hop), not tokens.  window > 0 (DTA_EINVAL otherwise). */
int dta_window_lo(const int32_t* depth, const int32_t* seg_off, const int32_t* seg_depth0, const int32_t* parent_of_seg,
                  int32_t M, int32_t T, int32_t window, int32_t* out_win_lo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Log-prob / entropy over vocabulary rows (HBM-bound).  logits: [R, V] bf16 / f16 / f32 with row_stride elements
 * between rows (multiple of 8; base 16-byte aligned, 32-byte for f32).  All statistics are fp32.
 * fwd writes lse[r] = ln sum_j exp(x_j/T), entropy[r] (may be NULL) and logprob[r] = x[labels[r]]/T - lse[r] (may be
 * NULL; a label outside [0, V) yields 0).  EXTRA picks: a trie node with several children predicts one token per child
 * (the fork-position logits of tree_training_engine.py:205-209, 217-220, 369-372).  They come as a CSR over the rows:
 * extra_ptr[R+1] (int32, absolute indices into the extra arrays; NULL = none), extra_labels[F]; the forward writes
 * extra_logprob[f] = x[extra_labels[f]]/T - lse[row of f].
 * bwd writes dLoss/dlogits to `dlogits` (== logits: in place) given g_logprob[r], g_extra_logprob[F] and g_entropy[r]
 * (each may be NULL), including the one-hot terms of every pick.
 * Masked columns (no soft-cap): a logit of -inf, or a finite one whose scaled value x * log2(e) / T is below -1e30 (it would overflow
 * fp32: the storage type's lowest value at T = 1), has probability 0.  It adds nothing to lse, to entropy (the limit p log p -> 0) or to
 * any shard statistic, and its element of dlogits is exactly 0 (unless it is itself a picked label: then the pick's one-hot term alone);
 * everything else on the row is what the row without that column gives.  A label on a -inf column yields logprob = -inf.  A row made
 * only of such columns is undefined.  A NaN logit still yields NaN.  Under a soft-cap a -inf logit is x' = -c like any very negative one, and 1 - tanh^2 = 0 makes its
 * gradient exactly 0.
 * Final-logit soft-capping (Gemma-2's final_logit_softcapping), softcap > 0: the three entries work on x' = c * tanh(x / c), c = softcap.
 * The cap is applied to the raw logit as it is loaded (no second pass over the [R, V] logits); lse, entropy, the label pick and the extra
 * picks are all statistics of x', and the temperature divides x'.  The backward reads each raw x once (in place: dlogits == logits) and
 * multiplies the gradient with respect to x' by 1 - tanh^2(x / c) before the store.  The cap is elementwise and comes before the
 * shard statistics, so the cross-rank combine is unchanged.  softcap <= 0 selects the kernels compiled without the cap; NaN / infinite:
 * DTA_EINVAL.
 * In-place backward under a cap: at most 2048 extra picks per row (their 1 - tanh^2 factors are taken before the row is
 * overwritten and held in LDS); the gradient element of a pick beyond that is written as NaN, so the overrun cannot pass for a
 * result.  An out-of-place call has no such limit.
 * Refusals come in this order: DTA_EINVAL (a null pointer, a size <= 0, a temperature that is not > 0, the soft-cap), DTA_EUNSUPPORTED
 * (dtype), DTA_EALIGN, DTA_EPRIOR.
 * Replaces vocab_parallel.py:13-27 (_gather_logprobs[_entropy]) with its autograd backward, and the torch indexing of
 * the fork rows.  */
int dta_logprob_entropy_fwd(const void* logits, const int64_t* labels, const int32_t* extra_ptr, const int64_t* extra_labels,
                            float* lse, float* entropy, float* logprob, float* extra_logprob,
                            int32_t R, int32_t V, int64_t row_stride, float temperature, int32_t dtype, float softcap, void* stream);
/* Vocab-sharded forward: raw per-shard statistics stats[R][4] = {m, s, t, picked} (log2 domain of x*log2(e)/T;
 * labels shard-local, -1 = owned by another rank; extra_picked[F] likewise raw x/T or 0) for the cross-rank combine of
 * vocab_parallel.py:125-160, 258-300. */
int dta_logprob_entropy_shard_stats(const void* logits, const int64_t* labels, const int32_t* extra_ptr, const int64_t* extra_labels,
                                    float* stats, float* extra_picked,
                                    int32_t R, int32_t V, int64_t row_stride, float temperature, int32_t dtype, float softcap, void* stream);
int dta_logprob_entropy_bwd(const void* logits, void* dlogits, const int64_t* labels, const int32_t* extra_ptr, const int64_t* extra_labels,
                            const float* lse, const float* entropy,
                            const float* g_logprob, const float* g_extra_logprob, const float* g_entropy,
                            int32_t R, int32_t V, int64_t row_stride, int64_t out_row_stride, float temperature, int32_t dtype,
                            float softcap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused row kernels of the decoder layer (HBM-bound; bf16/f16 storage, fp32 math).  They restate the
 * arithmetic of the third-party Qwen3 layers the reference calls (tree_training_engine.py:182-186,
 * 248-252, 351-353): RMSNorm = w * cast(x * rsqrt(mean(x^2)+eps)); rotate-half RoPE at position =
 * trie depth; SwiGLU = cast(silu(g)) * u.
 * ------------------------------------------------------------------------------------------- */
/* delta/x_out both NULL: y = norm(x).  Both given: x_out = x + delta (the residual-stream update of the decoder
 * layer, rounded to the storage dtype) and y = norm(x_out), in one pass.  bwd: `x` is the normalised input
 * (x_out of the forward), `dres` (may be NULL) the gradient arriving on the residual stream, added to dx.
 * Weight offset (Gemma: offset 1), w_offset != 0: y = cast(x * rsqrt(mean(x^2)+eps) * (w_offset + w)) - the offset is added to w in fp32
 * inside the kernel and the product is rounded ONCE (a 1 + w formed in bf16 would lose the low bits of w).  The fused residual add and
 * every other argument are unchanged, and so is dw_partial (d(w_offset + w)/dw = 1).  w_offset == 0 selects the kernels compiled
 * without the offset; NaN: DTA_EINVAL.
 * Refusals come in this order: DTA_EINVAL (a null pointer, a size <= 0, delta without x_out or the reverse, the offset),
 * DTA_EUNSUPPORTED (dtype, H % 8, bwd: H > 8192), DTA_EALIGN, DTA_EPRIOR. */
int dta_rmsnorm_fwd(const void* x, const void* delta, const void* w, void* x_out, void* y, float* rstd,
                    int32_t R, int32_t H, float eps, float w_offset, int32_t dtype, void* stream);
int dta_rmsnorm_bwd_blocks(int32_t R);   /* rows of the dw_partial workspace [blocks, H] (float); caller sums dim 0.  H % 8 == 0; bwd: H <= 8192.
                                          * dw_partial NULL (here and in dta_qk_norm_rope_bwd): a frozen weight - dx only, no partials written */
int dta_rmsnorm_bwd(const void* x, const void* w, const void* dy, const void* dres, const float* rstd, void* dx, float* dw_partial,
                    int32_t R, int32_t H, float w_offset, int32_t dtype, void* stream);
/* LayerNorm without bias (CohereLayerNorm, transformers' modeling_cohere.py) with the residual join of the parallel attention || MLP
 * block.  Rows of H, H % 8 == 0 and H <= 8192 in both directions; bf16 / f16 / fp32 storage, fp32 arithmetic; mean, rstd: float [R].
 *   m = mean(x),  r = rsqrt(mean((x - m)^2) + eps),  y = cast(w ((x - m) r)):  the weight multiplies in fp32 and the result is rounded
 *   ONCE.  The statistics are two passes over the row held in registers (the centred form, never E[x^2] - m^2), so a row with a large
 *   common offset keeps its rstd.
 * delta_a, delta_b, x_out all NULL: y = LN(x).  x_out with delta_a, or with delta_a and delta_b: x_out = cast((x + delta_a) + delta_b),
 * summed in fp32 and rounded once, and y = LN(x_out), in one pass over the row (the two branch outputs of the previous layer join the
 * stream here).  No operand may alias an output.
 * bwd: `x` is the normalised input (the forward's x_out).  With t = (x - m) r and g = dy w:
 *   dx = r (g - mean(g) - t mean(g t)) + dres  (dres may be NULL: the gradient arriving on the residual stream); x, delta_a and delta_b
 *   all take this one dx.  dw_partial: float [dta_layernorm_bwd_blocks(R), H] = per-workgroup sums over rows of dy t, summed over dim 0
 *   by dta_sum_slabs; NULL: a frozen weight, dx only.  No float atomics: identical calls give identical bits.
 * Refusals come in this order: DTA_EINVAL (a null pointer, a size <= 0, delta_b without delta_a, a delta without x_out or the reverse,
 * a NaN eps), DTA_EUNSUPPORTED (dtype, H % 8, H > 8192), DTA_EALIGN (a pointer off 16 bytes), DTA_EPRIOR. */
int dta_layernorm_fwd(const void* x, const void* delta_a, const void* delta_b, const void* w, void* x_out, void* y,
                      float* mean, float* rstd, int32_t R, int32_t H, float eps, int32_t dtype, void* stream);
int dta_layernorm_bwd_blocks(int32_t R);   /* rows of the dw_partial workspace [blocks, H] (float) */
int dta_layernorm_bwd(const void* x, const void* w, const void* dy, const void* dres, const float* mean, const float* rstd,
                      void* dx, float* dw_partial, int32_t R, int32_t H, int32_t dtype, void* stream);
/* head_dim D = 128 or 64.  x: [T, NH, D] with token stride x_stride_t; cos_sin: float [T, D] = {cos[D/2], sin[D/2]} of the token's
 * depth (rotate-half pairs element i with i + D/2); y: [T, NH, D] contiguous; w (head-norm weight [D]) may be NULL = RoPE only. */
int dta_qk_norm_rope_fwd(const void* x, const void* w, const float* cos_sin, void* y, float* rstd,
                         int32_t T, int32_t NH, int32_t head_dim, int64_t x_stride_t, float eps, int32_t dtype, void* stream);
int dta_qk_norm_rope_bwd_blocks(int64_t n_heads_total);   /* rows of dw_partial [blocks, head_dim] (the same count for D = 64 and 128) */
int dta_qk_norm_rope_bwd(const void* x, const void* w, const float* cos_sin, const void* dy, const float* rstd,
                         void* dx, float* dw_partial, int32_t T, int32_t NH, int32_t head_dim,
                         int64_t x_stride_t, int64_t dy_stride_t, int64_t dy_stride_h, int64_t dx_stride_t,
                         int32_t dtype, void* stream);   /* dx: [T, NH, D] with dx_stride_t elements between tokens (>= NH*D); dx == dy (same strides) is allowed: in place */
/* RoPE over the first R = rotary_dim elements of every head, no norm (Phi-3 / Phi-4-mini: partial_rotary_factor; GLM-4: interleaved
 * pairs).  x: [T, NH, D], D = 128 or 64, rows of D contiguous, token stride x_stride_t; cos_sin: float [T, R] = {cos[R/2], sin[R/2]} of
 * the token's depth; y: [T, NH, D] contiguous.  0 < R <= D.
 *   pairing 0 (half-split, R % 16 == 0), i < R/2:  y[i] = x[i] c[i] - x[i+R/2] s[i],   y[i+R/2] = x[i+R/2] c[i] + x[i] s[i]
 *   pairing 1 (interleaved, R % 8 == 0), i < R/2:  y[2i] = x[2i] c[i] - x[2i+1] s[i],  y[2i+1] = x[2i+1] c[i] + x[2i] s[i]
 * in fp32 with one rounding to the storage type; elements R .. D-1 are copied bit for bit, and their lanes read no table entry.
 * bwd: the rotation by the negative angle.  dy: token stride dy_stride_t, head stride dy_stride_h; dx: token stride dx_stride_t
 * (>= NH*D); dx == dy (same strides) is allowed: a lane writes exactly the bytes it read.
 * Refusals come in this order: DTA_EINVAL (a null pointer, T, NH or rotary_dim <= 0, pairing not 0 / 1), DTA_EUNSUPPORTED (dtype,
 * head_dim, rotary_dim > head_dim, rotary_dim % 16 for pairing 0 / % 8 for pairing 1), DTA_EALIGN (a pointer off 16 bytes, a stride off 8
 * elements), DTA_EINVAL (a negative token stride, dy_stride_h < head_dim, dx_stride_t < NH*D), DTA_EPRIOR. */
int dta_rope_partial_fwd(const void* x, const float* cos_sin, void* y, int32_t T, int32_t NH, int32_t head_dim, int32_t rotary_dim,
                         int32_t pairing, int64_t x_stride_t, int32_t dtype, void* stream);
int dta_rope_partial_bwd(const float* cos_sin, const void* dy, void* dx, int32_t T, int32_t NH, int32_t head_dim, int32_t rotary_dim,
                         int32_t pairing, int64_t dy_stride_t, int64_t dy_stride_h, int64_t dx_stride_t, int32_t dtype, void* stream);
/* Projection-wide q/k RMSNorm + RoPE (OLMo-2 / OLMo-3: `q_norm(q_proj(x))` with a weight of [NH*D], then the reshape to heads and
 * rotate-half RoPE - transformers' Olmo2Attention.forward).  x: [T, NH, D] with token stride x_stride_t (q or k read in place from the
 * fused projection output); w: [NH*D]; cos_sin as above; y: [T, NH, D] contiguous; rstd: [T].  D = 64 or 128, any NH >= 1 with
 * NH*D <= 8192.  Arithmetic: r = rsqrt(mean over all NH*D elements of x^2 + eps); a = cast(w x r) - Olmo2RMSNorm multiplies by the
 * weight in fp32 and rounds ONCE (`(self.weight * hidden_states).to(input_dtype)`), where the Qwen3 / Llama norm of dta_rmsnorm_fwd
 * rounds x r first; y = cast(a cos + partner(a) sin).  One wave per token - the four waves of a workgroup for rows above 2048 elements - holds the row in
 * registers: x is read once, the token's table row once.
 * bwd: da = dy cos + partner'(dy) sin stays in fp32 and is never rounded; dx = r (da w - t^ mean_{NH*D}(da w t^)), t^ = x r;
 * dw_partial: float [dta_wide_qk_norm_rope_bwd_blocks(T), NH*D], summed over dim 0 by dta_sum_slabs; NULL: a frozen weight, dx only.
 * dy: token stride dy_stride_t, head stride dy_stride_h; dx: token stride dx_stride_t (>= NH*D); dx == dy (same strides) is allowed:
 * a lane writes exactly the 16-byte groups it read.
 * Refusals come in this order: DTA_EINVAL (a null pointer, a size <= 0, a NaN eps), DTA_EUNSUPPORTED (dtype, head_dim, NH*D > 8192),
 * DTA_EALIGN (a pointer off 16 bytes, a stride off 8 elements), DTA_EINVAL (a token stride below NH*D), DTA_EPRIOR. */
int dta_wide_qk_norm_rope_fwd(const void* x, const void* w, const float* cos_sin, void* y, float* rstd,
                              int32_t T, int32_t NH, int32_t head_dim, int64_t x_stride_t, float eps, int32_t dtype, void* stream);
int dta_wide_qk_norm_rope_bwd_blocks(int32_t T);   /* rows of dw_partial [blocks, NH*head_dim] */
int dta_wide_qk_norm_rope_bwd(const void* x, const void* w, const float* cos_sin, const void* dy, const float* rstd,
                              void* dx, float* dw_partial, int32_t T, int32_t NH, int32_t head_dim,
                              int64_t x_stride_t, int64_t dy_stride_t, int64_t dy_stride_h, int64_t dx_stride_t,
                              int32_t dtype, void* stream);
/* RMSNorm, then the residual add (OLMo's post-norm layer, `residual + post_attention_layernorm(attn_out)` - Olmo2DecoderLayer.forward):
 * yn = cast(w y r) (one rounding, as Olmo2RMSNorm), r = rsqrt(mean(y^2) + eps), and out = cast(res + yn) in one pass over rows of H (H % 8 == 0, any H: above
 * 4096 the row is read twice, as in dta_rmsnorm_fwd).  yn may be NULL when only out is wanted; rstd: [R].  No operand may alias an
 * output.  The backward is dta_rmsnorm_bwd on (y, w, d out, rstd) with dres NULL; d res = d out.
 * Refusals come in this order: DTA_EINVAL (a null pointer, a size <= 0, a NaN eps), DTA_EUNSUPPORTED (dtype, H % 8), DTA_EALIGN,
 * DTA_EPRIOR. */
int dta_rmsnorm_add_fwd(const void* y, const void* w, const void* res, void* out, void* yn, float* rstd,
                        int32_t R, int32_t H, float eps, int32_t dtype, void* stream);
/* gate/up: [rows, cols] with `ld` elements between rows (they may be the two halves of one fused [rows, 2*cols]
 * projection output); y/dy: [rows, cols] contiguous; dgate/dup: `ld_grad` between rows. */
int dta_swiglu_fwd(const void* gate, const void* up, void* y, int64_t rows, int32_t cols, int64_t ld, int32_t dtype, void* stream);
int dta_swiglu_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup,
                   int64_t rows, int32_t cols, int64_t ld, int64_t ld_grad, int32_t dtype, void* stream);
/* GeGLU (Gemma): y = cast(gelu_tanh(g)) * u with gelu_tanh(g) = 0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3))), HF's gelu_pytorch_tanh.
 * Arguments and layouts of dta_swiglu_fwd / _bwd. */
int dta_geglu_fwd(const void* gate, const void* up, void* y, int64_t rows, int32_t cols, int64_t ld, int32_t dtype, void* stream);
int dta_geglu_bwd(const void* gate, const void* up, const void* dy, void* dgate, void* dup,
                  int64_t rows, int32_t cols, int64_t ld, int64_t ld_grad, int32_t dtype, void* stream);

/* out[c][r] = in[r][c]: `rows` x `cols` elements of `elem_size` bytes (2: bf16 / f16, 4: f32), `ld_in` / `ld_out` elements between rows
 * (`rows`, `cols`, `ld_in` and `ld_out` multiples of 16 / elem_size: 8 for 2-byte types, 4 for f32; pointers 16-byte aligned).  HBM-bound (one read + one write).  Used for transposed copies of the projection and
 * LM-head weights, made once per weight version: the input-gradient GEMMs dx = dy . W of the model calls (tree_training_engine.py:440,
 * torch.autograd.backward) run 12-25 % faster with the contraction index contiguous in both operands. */
int dta_transpose(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, int32_t elem_size, void* stream);

/* out[i] = round_to(out_dtype)( sum_{s < slabs} part[s * slab_stride + i]  + (extra ? extra[i] : 0) ),  i < n; all sums in fp32.
 * The reduction of weight-gradient partials fused with the rounding to the parameter dtype: the per-workgroup dw partials of
 * dta_rmsnorm_bwd / dta_qk_norm_rope_bwd (slabs = workgroups, n = H or head_dim) and the slices of the split-K weight-gradient GEMM
 * (slabs = the split, n = out*in, extra = the product of the rows the equal slices leave over).  Stands where the reference's
 * autograd sums a weight's gradient over all rows of a model call in one GEMM (tree_training_engine.py:440).  `out` may not alias
 * `part` or `extra`.  Any n; the vector form is taken when slabs <= 16 and n, slab_stride are multiples of 4 with 16-byte aligned pointers. */
int dta_sum_slabs(const float* part, int64_t slabs, int64_t n, int64_t slab_stride, const float* extra, void* out, int32_t out_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mixture of experts (Qwen3MoeSparseMoeBlock, transformers 5.x modeling_qwen3_moe.py).  T tokens, E experts (E <= 256), top k
 * (k <= 16, k <= E); no power-of-two requirement.  dtype DTA_BF16 / DTA_F16 (MFMA GEMMs) or DTA_F32 (plain-FMA GEMMs, the gradient-check
 * path of fp32 models).  Nothing in the routing path copies to the host: offsets, rows and the GEMM tile table stay on the device.
 * ------------------------------------------------------------------------------------------- */
#define DTA_MOE_BM 128       /* rows per tile of the grouped GEMMs (tile table granularity) */
#define DTA_MOE_FWD 0
#define DTA_MOE_DGRAD 1
#define DTA_MOE_WGRAD 2

/* Router.  logits [T, E] (model dtype).  Restates Qwen3MoeTopKRouter.forward:
 *     router_probs = softmax(router_logits, dtype=float); top_value, indices = topk(router_probs, k)
 *     if norm_topk_prob: top_value /= top_value.sum(-1); top_value = top_value.to(router_logits.dtype)
 * Writes topk_ids int32 [T, k] in descending probability, topk_w [T, k] (model dtype, rounded once from fp32) and lse float [T]
 * (natural log-sum-exp of the logit row, for the backward).  Ties: the LOWER expert index wins (it comes first). */
int dta_moe_router_fwd(const void* logits, int32_t* topk_ids, void* topk_w, float* lse, int32_t T, int32_t E, int32_t k, int32_t norm_topk,
                       int32_t dtype, void* stream);
/* dlogits [T, E] (model dtype) from dtopk_w [T, k] (model dtype) through the renormalisation (norm_topk) and the fp32 softmax: the autograd
 * backward of the lines above, with p recomputed from logits and lse. */
int dta_moe_router_bwd(const void* logits, const float* lse, const int32_t* topk_ids, const void* dtopk_w, void* dlogits,
                       int32_t T, int32_t E, int32_t k, int32_t norm_topk, int32_t dtype, void* stream);

/* Permutation: counting sort of the P = T*k (token, slot) pairs by expert, replacing the one_hot / where / index loop of
 * Qwen3MoeExperts.forward.  Writes expert_offsets [E+1] (rows of expert e: [off[e], off[e+1])), row_of_pair [P] (pair t*k+j -> its row
 * in expert order; -1 for an id outside [0, E)), src_token [P] (row -> token) and the tile table tiles [2 * dta_moe_tile_bound(P, E)]:
 * {expert, first row} per DTA_MOE_BM-row tile of every expert, entries past the last tile {-1, 0}.  Within an expert the rows are in pair
 * (= token) order; the result is the same bit for bit on every call (no order comes from atomics).  workspace: int32
 * [dta_moe_permute_workspace(P, E)]. */
int dta_moe_permute_workspace(int32_t n_pairs, int32_t E);
int dta_moe_tile_bound(int32_t n_pairs, int32_t E);          /* ceil(P / DTA_MOE_BM) + E */
int dta_moe_permute(const int32_t* topk_ids, int32_t T, int32_t k, int32_t E, int32_t* workspace,
                    int32_t* expert_offsets, int32_t* row_of_pair, int32_t* src_token, int32_t* tiles, void* stream);

/* Grouped GEMM over the expert-sorted rows (n_rows = P of the permutation), weights w [E, N, K] (the per-expert nn.functional.linear of
 * Qwen3MoeExperts.forward; gate_up_proj is [E, 2I, H], down_proj [E, H, I]).  fp32 accumulation, each output rounded once.
 *   DTA_MOE_FWD:   out[r][n] = sum_k x[g(r)][k] w[e(r)][n][k]           out [n_rows, N]     (Y_e = X_e W_e^T)
 *   DTA_MOE_DGRAD: out[r][k] = sum_n dy[r][n] w[e(r)][n][k]             out [n_rows, K]     (dX_e = dY_e W_e, sorted rows)
 *   DTA_MOE_WGRAD: out[e][n][k] = sum_{r of e} dy[r][n] x[g(r)][k]      out [E, N, K]       (dW_e = dY_e^T X_e; empty experts: zero)
 * g(r) = gather[r] (src_token of the permutation: X read by token inside the operand load) or r when gather is NULL.  x / dy rows are
 * contiguous (ld = K / N).  The fwd / dgrad grid is sized from the bound of the tile table; workgroups past its last tile exit.
 * N and K multiples of 16 (DTA_EUNSUPPORTED otherwise); pointers 16-byte aligned (DTA_EALIGN). */
int dta_moe_grouped_gemm(int32_t mode, const void* x, const void* w, const void* dy, void* out, const int32_t* gather,
                         const int32_t* expert_offsets, const int32_t* tiles, int32_t n_rows, int32_t E, int32_t N, int32_t K,
                         int32_t dtype, void* stream);

/* Combine: out[t] = sum_j topk_w[t][j] * y[row_of_pair[t*k+j]], summed in fp32 and rounded once (Qwen3MoeExperts.forward's
 * `current_hidden_states * top_k_weights` + index_add_).  topk_w == NULL: weight 1 - the fixed-order scatter-back
 * dX[t] = sum_j dXsorted[row(t, j)] of the gathered GEMM input. */
int dta_moe_combine_fwd(const void* y, const void* topk_w, const int32_t* row_of_pair, void* out, int32_t T, int32_t k, int32_t H,
                        int32_t dtype, void* stream);
/* dy[row(t, j)] = topk_w[t][j] * dout[t];  dtopk_w[t][j] = <dout[t], y[row(t, j)]> (fp32, fixed order).  No float atomics. */
int dta_moe_combine_bwd(const void* dout, const void* y, const void* topk_w, const int32_t* row_of_pair, void* dy, void* dtopk_w,
                        int32_t T, int32_t k, int32_t H, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Low-rank adapters (LoRA): y = base(x) + scaling * (x A^T) B^T on a projection whose base weight stays frozen.  The products with
 * one long operand (T packed rows) and one of rank R <= 256; dtype DTA_BF16 / DTA_F16 (MFMA, fp32 accumulation; fp32 models use torch
 * expressions - DTA_EUNSUPPORTED here).  ld* are row pitches in elements; a pitch or pointer that is not a multiple of 16 bytes is
 * served by element loads (a rank-6 operand is [T, 6] in memory: the rank is padded in staging, never in HBM).  T any row count, K and
 * N multiples of 16, R any integer 1..256 (DTA_EUNSUPPORTED otherwise).  The *_host arguments are HOST arrays, read during the
 * call (they travel as kernel arguments); NULL rscale_host = all ones.  Scales multiply the fp32 accumulator.  No float atomics: the
 * same inputs give the same bits on every call.
 * ------------------------------------------------------------------------------------------- */
/* out[t][r] = rscale[r] * sum_k x[t][k] m[r][k];  x [T, K], m [R, K], out [T, R] (model dtype).  One read of x. */
int dta_lora_down(const void* x, int64_t ldx, const void* m, int64_t ldm, void* out, int64_t ldo, const float* rscale_host,
                  int32_t T, int32_t R, int32_t K, int32_t dtype, void* stream);
/* part[s][r][k] = rscale[r] * sum_{t in slab s} l[t][r] x[t][k]:  l [T, R], x [T, K], part float [dta_lora_wgrad_slabs(T, K), R, K].  The
 * slabs are whole 64-row steps of T in order; the caller adds them in slab order (dta_sum_slabs), which also rounds to the gradient's
 * dtype (fp32 adapters get the fp32 sum unrounded).  One read of x and l. */
int dta_lora_wgrad_slabs(int32_t T, int32_t K);
int dta_lora_wgrad(const void* l, int64_t ldl, const void* x, int64_t ldx, float* part, const float* rscale_host,
                   int32_t T, int32_t R, int32_t K, int32_t dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Policy objective over the packed trie (losses.PolicyLoss; HBM-bound; fp32 throughout): the clipped PPO / GRPO surrogate with an
 * optional dual clip, a KL penalty to a reference policy, an entropy bonus and a loss mask, evaluated per packed ROW.  Stands where the
 * reference calls the user's loss_fn once per sequence on gathered slices and sums the per-sequence gradients back
 * (tree_training_engine.py:379-440).  Three options of this one objective: the level of the importance ratio (ratio_level), the form of
 * the surrogate (surrogate) and a rollout importance weight on it (is_level, is_mode, is_cap, is_floor).
 *
 * Sequences are numbered in callback order: leaf by leaf in packed order, within a leaf in attach-list order.  Sequence s has
 * n_s = len_s - 1 predictions; its per-token inputs are elements [seq_ptr[s], seq_ptr[s+1]) of old_lp / ref_lp / rollout_lp / mask / adv
 * (fp32, N = seq_ptr[S] elements each; element j belongs to the prediction of token j + 1).  adv_per_seq != 0: adv is [S], one value per
 * sequence.  old_lp NULL: on-policy (ratio 1, gradient as if old_lp == lp).  ref_lp may be NULL when kl_coef == 0, rollout_lp (the
 * sampler's log-prob of each token) when is_level == 0: they are not read then.
 *
 * Row t (depth[t] = d, log-prob lp[t] of its token given its parent, entropy ent[t] of the distribution at it) lies on the path of the
 * sequences s in [row_seq_lo[t], row_seq_hi[t]) with n_s >= d - one contiguous range, because the sequences through a subtree are
 * contiguous in callback order; an empty range (filler rows) is legal.  For each such s the row owns
 *   the log-prob term (s, j = d - 1) when d >= 1:   x = lp[t] - old_lp[.],  r = exp(x),  A = adv,  m = mask,  lo = 1 - clip_low,
 *                                                   hi = 1 + clip_high
 *       pg = max(-r A, -clamp(r, lo, hi) A);  dual_clip = c > 1 and A < 0:  pg = min(pg, -c A)                   (surrogate 0, "ppo")
 *       dd = ref_lp[.] - lp[t];  kl = -dd (estimator 0, "k1") | dd^2 / 2 (1, "k2") | exp(dd) - dd - 1 (2, "k3")
 *       loss += w_s m (omega pg + kl_coef kl);   dlp[t] += w_s m (omega dpg + kl_coef dkl),  dpg = -r A where -r A is the active branch
 *       (ties included), 0 where the clamp or the dual clip is;  dkl = 1 | -dd | 1 - exp(dd);  omega: the rollout weight, below
 *   the entropy term (s, j = d) when d < n_s:       loss -= w_s m entropy_coef ent[t];   dent[t] -= w_s m entropy_coef
 * w_s = scale / n^, n^ = max(sum_j m_j, 1) (agg 0, "seq_mean") or scale (agg 1, "token_sum").  exp is the accurate expf.  Every (s, j) is
 * owned by exactly one row in each role: no scatter, no atomics; dlp[T] and dent[T] are written for EVERY row (0 where nothing
 * contributes), and identical calls give identical bits.
 *
 * surrogate 1 "cispo", on the token ratio r:
 *       pg = -clamp(r, lo, hi) A lp[t],   dpg = -clamp(r, lo, hi) A  (the clamp is a constant of the gradient: dpg is never zeroed);
 *       "clipped" counts the masked tokens with r outside [lo, hi], whatever the sign of A.
 * ratio_level 1 "sequence" (GSPO; ratio_level 0 "token" is the above): ONE importance ratio per sequence,
 *       r_s  = exp( sum_j m_j (lp[row(s, j)] - old_lp[.]) / n^ )        (old_lp NULL: r_s = 1; length-normalised under agg 1 too)
 *       pg_j = max(-r_s A_j, -clamp(r_s, lo, hi) A_j);  dual_clip = c > 1 and A_j < 0:  pg_j = min(pg_j, -c A_j)
 *       loss += w_s m_j (omega_j pg_j + kl_coef kl_j);    d loss / d lp[row(s, t)] = c_s m_t + w_s m_t kl_coef dkl_t,
 *       c_s  = w_s r_s / n^ * sum_j m_j omega_j (-A_j) [-r_s A_j is the active branch of pg_j (ties included)]
 * (the gradient flows through r_s to every masked token of the sequence).  row(s, j), the packed row of depth j + 1 on the root path
 * of s, comes from a path table over the M leaves: the path of leaf i is runs [leaf_run_ptr[i], leaf_run_ptr[i+1]) of contiguous packed
 * rows, root first; run k starts at row run_row0[k] with depth run_depth0[k] and ends where the leaf's next run starts (the last run:
 * at the leaf's end, which no sequence of the leaf passes); seq_leaf[s] is the leaf of sequence s.  R = leaf_run_ptr[M] runs in all.
 * Table entries that point outside [0, M), [0, R) or [0, T) are clamped or skipped, never followed.
 * The rollout importance weight omega (an off-policy correction), per prediction j of s:
 *       y_j = old_lp[.] - rollout_lp[.]            old_lp NULL: y_j = lp[row(s, j)] - rollout_lp[.]; y carries no gradient either way
 *       is_level 0:                  omega = 1
 *       is_level 1 "token":          rho_j = exp(y_j)
 *       is_level 2 "sequence":       rho_s = exp(sum_j m_j y_j)
 *       is_level 3 "sequence_mean":  rho_s = exp(sum_j m_j y_j / n^)
 *       is_mode 0 "truncate":  omega = min(rho, is_cap);     is_mode 1 "mask":  omega = rho if is_floor <= rho <= is_cap, else 0
 * omega multiplies the surrogate alone, never the KL or the entropy term, and is a constant of the gradient.  omega is formed by
 * comparisons on rho, never by arithmetic on it: an exponent above 88.7, where expf gives +inf, yields is_cap under "truncate" and 0
 * under "mask", one far below zero yields 0 (or what is_floor says of 0); no finite input gives NaN.
 * The path tables may be NULL, with M = R = 0, when nothing walks a path: ratio_level 0 with is_level 0 or 1, and ratio_level 0 with
 * is_level 2 or 3 when old_lp is given (y is then a sweep over the per-token inputs alone).  They are required for ratio_level 1 and for
 * is_level 2 or 3 with old_lp NULL.  w[S], c[S] and omega[S] are workspaces the caller may read afterwards: w[s] = w_s, omega[s] is the
 * sequence's weight (1 for is_level 0 and 1), c[s] is 0 for ratio_level 0.
 * Three launches on `stream`; their geometry depends on T and S alone:
 *   sequence pass  one workgroup per sequence (grid-strided past 2048).  It owns w[s], omega[s] and c[s].  It walks the path only for
 *                  what reads a row's lp: sum m x of r_s (ratio_level 1 with old_lp), sum m y with old_lp NULL, and the c_s sweep when
 *                  that forms a per-token weight with old_lp NULL; everything else is a sweep of the per-token inputs, and the mask is
 *                  not swept at all where nothing reads its sum (agg 1 with ratio_level 0 and is_level 0 or 1).  Under ratio_level 1 it
 *                  owns the surrogate's share of loss, sum m pg' and the clipped tokens; under ratio_level 1 or is_level 2 / 3 it owns
 *                  sum m omega and sum m [omega != rho];
 *   row pass       one thread per row, a wave for a row with more than 16 sequences: the terms above.  ratio_level 0: r, the surrogate
 *                  form and the weight - a per-token weight is formed here (y from old_lp, or from the row's lp; truncate or mask), a
 *                  sequence's weight is read from omega[s].  ratio_level 1: c_s m in place of the token's own surrogate gradient (c_s
 *                  holds the weight).  It owns every statistic the sequence pass does not;
 *   reduction      both passes' partials, partial[dta_policy_loss_blocks(T, S)][8], summed in a fixed order into
 *                  stats[8] = {loss, sum m pg' (pg' = omega pg), sum m kl, sum m ent, clipped, sum m, sum m omega, sum m [omega != rho]}
 *                  (losses.OFFPOLICY_STATS), always all eight: is_level 0 gives stats[6] = sum m and stats[7] = 0.  "clipped" counts
 *                  the masked tokens whose branch is the clamp or the dual clip.  The three counts are exact.
 * Refusals come in this order: DTA_EINVAL (a null pointer other than old_lp / ref_lp / rollout_lp / the path tables, T <= 0, S <= 0, a
 * negative or non-finite clip, dual_clip neither 0 (= none) nor a finite value > 1, kl_estimator not 0..2, agg not 0 / 1, a non-finite
 * coefficient or scale, kl_coef != 0 with ref_lp NULL, ratio_level not 0 / 1, surrogate not 0 / 1, is_level not 0..3, is_mode not 0 / 1,
 * is_cap non-finite or <= 0, is_floor non-finite, negative or not below is_cap, is_floor != 0 with is_mode 0, surrogate 1 with
 * ratio_level 1 or with a dual clip, is_level != 0 with rollout_lp NULL, a path table NULL or M or R <= 0 where a path is walked),
 * DTA_EALIGN (a pointer off 16 bytes), DTA_EPRIOR.  The path tables and their sizes come last among the DTA_EINVAL checks: a call with
 * a missing path table or M <= 0 AND a bad hyper-parameter is refused for the hyper-parameter (the status is DTA_EINVAL either way). */
int dta_policy_loss_blocks(int32_t T, int32_t S);   /* rows of the partial workspace [blocks, 8] (float); T <= 0 or S <= 0: DTA_EINVAL */
int dta_policy_loss(const float* lp, const float* ent, const int32_t* depth, const int32_t* row_seq_lo, const int32_t* row_seq_hi,
                    const int32_t* seq_ptr, const int32_t* leaf_run_ptr, const int32_t* run_row0, const int32_t* run_depth0,
                    const int32_t* seq_leaf, const float* old_lp, const float* ref_lp, const float* rollout_lp, const float* mask,
                    const float* adv, int32_t adv_per_seq, float* w, float* c, float* omega, float* dlp, float* dent, float* partial,
                    float* stats, int32_t T, int32_t S, int32_t M, int32_t R, float clip_low, float clip_high, float dual_clip,
                    float kl_coef, int32_t kl_estimator, float entropy_coef, int32_t agg, float scale, int32_t ratio_level,
                    int32_t surrogate, int32_t is_level, int32_t is_mode, float is_cap, float is_floor, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Preference objectives over the packed trie (losses.PreferenceLoss; HBM-bound, fp32 throughout): DPO / cDPO / SimPO (kind 0,
 * "sigmoid"), SLiC (1, "hinge") and IPO (2, "ipo") over P (chosen, rejected) pairs of the trie's sequences, with an optional NLL term on
 * the chosen member.  A pair couples two sequences, so no per-sequence callback can state it; here the pairs are one stage between a
 * sequence pass and a row pass.  The numbering of the sequences, seq_ptr, mask, the row tables (depth, row_seq_lo, row_seq_hi) and the
 * path tables (leaf_run_ptr, run_row0, run_depth0, seq_leaf over M leaves and R runs) are those of dta_policy_loss; table entries
 * that point outside [0, M), [0, R) or [0, T) are clamped or skipped, never followed.  mask [N] is required (all ones: no mask).
 *
 * The reference policy comes in exactly one of two forms: ref_lp [N], per-token reference log-probs (summed here under the mask), or
 * ref_sum [S], the already masked sum per sequence; the other pointer is NULL.  reference_free != 0: neither is read (both may be NULL).
 * For sequence s, with row(s, j) the packed row of depth j + 1 on its root path:
 *       n^_s = max(sum_j m_j, 1),   P_s = sum_j m_j lp[row(s, j)],   F_s = sum_j m_j ref_lp[.] | ref_sum[s] | 0
 *       u_s  = (P_s - F_s) / N_s,   N_s = n^_s when length_normalize != 0, else 1
 * For pair q, c = pair_c[q] the chosen and r = pair_r[q] the rejected sequence, z = beta (u_c - u_r) - gamma, e = label_smoothing:
 *       kind 0:  L = (1 - e) softplus(-z) + e softplus(z),   dL/dz = sigmoid(z) - (1 - e)
 *       kind 1:  L = max(0, 1 - z),                          dL/dz = -[z < 1]            (a tie z == 1: gradient 0)
 *       kind 2:  L = (u_c - u_r - 1 / (2 beta))^2,           dL/d(u_c - u_r) = 2 (u_c - u_r - 1 / (2 beta))
 *       loss = scale sum_q L_q - scale sft_coef sum_q P_c / n^_c
 *       g[c] = scale (dL/du_c) / N_c - scale sft_coef / n^_c,    g[r] = -scale (dL/du_c) / N_r,    dL/du_c = beta dL/dz (kinds 0, 1)
 * and d loss / d lp[row(s, j)] = g[s] m_j.  softplus(x) = max(x, 0) + log1pf(expf(-|x|)); the sigmoid is formed from expf(-|z|) and
 * cannot overflow; expf and log1pf are the accurate functions.  Every sequence should be a member of exactly one pair.  A sequence in
 * no pair gets g = 0; a pair with an index outside [0, S) is skipped; a sequence named by several pairs gets the coefficient of one of
 * them (which one is not defined: the Python side refuses such a trie).  Entropy takes no part and there is no dent.
 * Four launches on `stream`; their geometry depends on T, S and P alone; no atomics, identical bits for identical calls:
 *   sequence pass  one workgroup per sequence (grid-strided past 2048): the runs of its path with the threads strided over each run's
 *                  rows, workgroup sums in a fixed order; writes nhat[s] = n^_s, u[s], sft[s] = P_s / n^_s and g[s] = 0 - workspaces [S]
 *                  the caller may read afterwards;
 *   pair pass      one thread per pair (grid-strided past 1024 workgroups of 256): z, L, g[c], g[r] and per-workgroup partial
 *                  statistics, partial[dta_preference_loss_blocks(T, S, P)][8];
 *   row pass       dlp[t] = sum over s in [row_seq_lo[t], row_seq_hi[t]) with n_s >= depth[t] >= 1 of g[s] mask[seq_ptr[s] + depth[t] - 1],
 *                  written for EVERY row of dlp[T], 0 where nothing contributes (rows of depth 0, filler rows);
 *   reduction      the partials in a fixed order into stats[8] = {loss, sum L, sum P_c / n^_c, sum beta (u_c - u_r), sum beta u_c,
 *                  sum beta u_r, pairs with u_c > u_r (a tie is not counted), pairs} (losses.PREFERENCE_STATS).
 * Refusals come in this order: DTA_EINVAL (a null pointer other than ref_lp / ref_sum; T, S, M, R or P <= 0; kind not 0..2; a
 * non-finite beta, label_smoothing, gamma, sft_coef or scale; beta <= 0; label_smoothing outside [0, 0.5) or non-zero with kind != 0;
 * gamma != 0 with kind 2; sft_coef < 0; reference_free == 0 with ref_lp and ref_sum both NULL or both given), DTA_EALIGN (a pointer off
 * 16 bytes), DTA_EPRIOR. */
int dta_preference_loss_blocks(int32_t T, int32_t S, int32_t P);   /* rows of the partial workspace [blocks, 8] (float); T, S or P <= 0: DTA_EINVAL */
int dta_preference_loss(const float* lp, const int32_t* depth, const int32_t* row_seq_lo, const int32_t* row_seq_hi,
                        const int32_t* seq_ptr, const int32_t* leaf_run_ptr, const int32_t* run_row0, const int32_t* run_depth0,
                        const int32_t* seq_leaf, const int32_t* pair_c, const int32_t* pair_r, const float* ref_lp,
                        const float* ref_sum, const float* mask, float* nhat, float* u, float* sft, float* g, float* dlp,
                        float* partial, float* stats, int32_t T, int32_t S, int32_t M, int32_t R, int32_t P, int32_t kind,
                        float beta, float label_smoothing, float gamma, int32_t length_normalize, int32_t reference_free,
                        float sft_coef, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Quantised frozen base (quant.py; HBM-bound): the frozen projection weights of a LoRA model stored in a 4- or 8-bit block format and
 * expanded to the model dtype where a GEMM needs them.  A weight [R, C] (R = out, C = in) is cut into blocks along C; each block has
 * one fp32 scale.  q: the codes, row after row without a pitch; scales: float [R, C / block].
 *   DTA_QUANT_NF4  block 64.  scale = absmax (fp32); v = x / scale (a correctly rounded fp32 division); code = #{i < 15 : v > mid_i},
 *                  mid_i = (c_i + c_{i+1}) / 2 formed in float64 and rounded to fp32 - a value exactly on a midpoint takes the lower
 *                  code; c_0..c_15 the NormalFloat-4 table (csrc/dta_quant_tables.h).  absmax == 0: scale 0, code 7 (c_7 = 0).
 *                  q: uint8 [R, C / 2], byte j of a row = element 2j in bits 7..4, element 2j + 1 in bits 3..0.
 *   DTA_QUANT_FP8  block 128.  scale = absmax / 448 (fp32 division); q = e4m3(clamp(x / scale, -448, 448)), OCP e4m3
 *                  (float8_e4m3fn), fp32 division, round to nearest even.  scale == 0: q = 0.  q: uint8 [R, C].
 * Dequantisation: out = round_to(out_dtype, value(code) * scale) - one fp32 product, one rounding.  Non-finite weights are the
 * caller's to refuse (quant.quantize_base does); the kernels do not check.  Scales in the fp32 subnormal range: DESIGN.md §4q.
 * Refusals of both entries come in this order: DTA_EINVAL (a null pointer, R or C <= 0, a pitch below the row, transposed not 0 / 1),
 * DTA_EUNSUPPORTED (fmt, dtype, C not a multiple of the block, C >= 2^22), DTA_EALIGN (q, scales or out off 16 bytes; w off its
 * element size; row-major: ld_out not a multiple of 16 bytes), DTA_EPRIOR.
 * ------------------------------------------------------------------------------------------- */
#define DTA_QUANT_NF4 0
#define DTA_QUANT_FP8 1
/* w: [R, C] bf16 / f16 / f32 with ld_w elements between rows (a member of a fused weight, a slice).  One wave per block: absmax by a
 * wave reduction, then the codes.  Runs once per weight. */
int dta_quant_blockwise(const void* w, int64_t ld_w, int64_t R, int64_t C, int32_t w_dtype, int32_t fmt, void* q, float* scales,
                        void* stream);
/* transposed == 0: out [R, C] at ld_out elements between rows (>= C; a multiple of 16 bytes) - the members of a fused group (q|k|v,
 * gate|up) go straight into their row ranges of ONE stacked operand.  16-byte stores; a lane reads its block's scale once; the codes
 * are read non-temporally.  transposed == 1: out [C, R] at ld_out elements between rows (>= R, any; rows that start on 16 bytes get
 * 16-byte stores, others and the ragged edge of R element stores) through a 64 x 64 LDS tile as dta_transpose, with the decode on the
 * load side - the members of a group write their column ranges of one transposed stacked operand.  out_dtype bf16 / f16 / f32. */
int dta_dequant_blockwise(const void* q, const float* scales, int64_t R, int64_t C, int32_t fmt, void* out, int64_t ld_out,
                          int32_t out_dtype, int32_t transposed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DTA_H */
