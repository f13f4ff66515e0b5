// Shared host-side launch bookkeeping of the C ABI (include/dta.h).
#ifndef DTA_COMMON_H
#define DTA_COMMON_H
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/dta.h"

// A HIP error that is ALREADY pending when an entry point is called (an earlier asynchronous kernel fault, or a failed
// runtime call nobody checked) must neither be swallowed by this launch nor be blamed on it: nothing is launched and the
// caller gets DTA_EPRIOR; dta_take_pending_error() names and clears it.  (Round 1 cleared it silently here.)
#define DTA_REFUSE_IF_PRIOR_ERROR() do { if (hipPeekAtLastError() != hipSuccess) return DTA_EPRIOR; } while (0)
// status of THIS launch (configuration errors: invalid grid, too much LDS, no code object for the device ...)
#define DTA_LAUNCH_STATUS() (hipGetLastError() == hipSuccess ? DTA_OK : DTA_ELAUNCH)
// The tail of an entry whose checks have passed, where it is exactly these two around the launches: launch(hipStream_t) enqueues them
template <class L> inline int dta_launch(void* stream, L&& launch) {
  DTA_REFUSE_IF_PRIOR_ERROR();
  launch(static_cast<hipStream_t>(stream));
  return DTA_LAUNCH_STATUS();
}

// The arguments of one dta_tree_attn_fwd / dta_tree_attn_bwd call (include/dta.h), under the field names of the kernel parameter structs.
// Host side only: the entry fills it once, tree_attn.hip validates it once, and the launch code copies its fields into the parameter
// struct of the chosen kernel form - it is never a kernel argument itself.  The forward leaves the backward fields null
// (out / lse_w are the forward's outputs; o / lse_r the same buffers as the backward's inputs).
struct DtaAttnArgs {
  const void *q, *k, *v, *o, *dout;
  void *out, *dq, *dk, *dv;
  float* lse_w; const float* lse_r; float* delta;
  const int32_t *subtree_end, *run_ptr, *runs, *ktile_qend;
  const int32_t *dkv_units, *dkv_splits; float* dkv_ws;
  int32_t n_units, n_splits;
  int32_t Tq, Tk, q_offset, Hq, Hkv, head_dim;
  int64_t q_st, q_sh, kv_st, kv_sh, v_st, v_sh, o_st, o_sh, dq_st, dq_sh, dkv_st, dkv_sh;
  float scale; int32_t dtype, accumulate, which;
  const int32_t* win_lo; int32_t window; float softcap;
  hipStream_t stream;
};

// The kernel form of a call, chosen once: f(WIN, CAP) with std::bool_constant arguments.  window <= 0 / softcap <= 0 select the kernels
// compiled without those terms.
template <class F> inline void dta_attn_form(const DtaAttnArgs& a, F&& f) {
  using Y = std::true_type; using N = std::false_type;
  if (a.softcap > 0.f) { if (a.window > 0) f(Y{}, Y{}); else f(N{}, Y{}); }
  else { if (a.window > 0) f(Y{}, N{}); else f(N{}, N{}); }
}

// The storage type of a row-kernel call, chosen once: f(DT) with DT a std::integral_constant of DTA_BF16 / DTA_F16 / DTA_F32.  The entry
// has refused every other dtype before.
template <class F> inline void dta_storage_type(int32_t dtype, F&& f) {
  if (dtype == DTA_BF16) f(std::integral_constant<int, DTA_BF16>{});
  else if (dtype == DTA_F16) f(std::integral_constant<int, DTA_F16>{});
  else f(std::integral_constant<int, DTA_F32>{});
}
inline bool row_dtype_ok(int dtype) { return dtype == DTA_BF16 || dtype == DTA_F16 || dtype == DTA_F32; }
// The same for the MFMA kernels of MoE and LoRA, which exist for the 16-bit types only: f(DT) with DT = DTA_BF16 / DTA_F16
template <class F> inline void dta_storage_type16(int32_t dtype, F&& f) {
  if (dtype == DTA_BF16) f(std::integral_constant<int, DTA_BF16>{});
  else f(std::integral_constant<int, DTA_F16>{});
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <class... P> inline bool all_aligned16(const P*... p) { return (aligned16(p) && ...); }    // a null pointer counts as aligned
// workgroups that cover n items at `per` each; row_blocks: the same for a grid-stride kernel, at least 1 and at most cap
inline unsigned ceil_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline int row_blocks(int64_t rows, int per_block, int cap) { int64_t b = (rows + per_block - 1) / per_block; return (int)(b < cap ? (b > 0 ? b : 1) : cap); }

// fp32 tree attention (tree_attn_f32.hip, head_dim 64 or 128): what dta_tree_attn_fwd / dta_tree_attn_bwd launch for dtype DTA_F32, after
// their argument checks
int dta_attn_fwd_f32(const DtaAttnArgs& a);
int dta_attn_bwd_f32(const DtaAttnArgs& a);

#endif
