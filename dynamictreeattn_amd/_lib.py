"""ctypes binding of libdta_mi355x.so (include/dta.h).  There is no fallback: every entry point
raises if the library is missing or a call returns a non-zero status."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB

_lib = None
_i32, _i64, _f32, _vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p

_PROTOS = {
    "dta_version": ([], C.c_int),
    "dta_take_pending_error": ([C.c_char_p, _i32], C.c_int),
    "dta_lcp_adjacent": ([_vp, _vp, _vp, _i32, _vp, _vp, _vp], C.c_int),
    "dta_leafize": ([_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp], C.c_int),
    "dta_preorder_meta": ([_vp] * 8 + [_i32, _i32] + [_vp] * 4 + [_vp], C.c_int),
    # q k v out lse subtree_end run_ptr runs | Tq Tk q_offset Hq Hkv head_dim | q k v o (token, head) strides | scale dtype |
    # win_lo window softcap stream
    "dta_tree_attn_fwd": ([_vp] * 8 + [_i32] * 6 + [_i64] * 8 + [_f32, _i32] + [_vp, _i32, _f32, _vp], C.c_int),
    # q k v out dout lse delta dq dk dv subtree_end run_ptr runs ktile_qend | sizes | q k v o dq dkv strides | scale dtype accumulate which |
    # dkv_units n_units dkv_splits n_splits dkv_ws | win_lo window softcap stream
    "dta_tree_attn_bwd": ([_vp] * 14 + [_i32] * 6 + [_i64] * 12 + [_f32, _i32, _i32, _i32] + [_vp, _i32, _vp, _i32, _vp]
                          + [_vp, _i32, _f32, _vp], C.c_int),
    "dta_window_lo": ([_vp] * 4 + [_i32, _i32, _i32, _vp, _vp], C.c_int),
    "dta_logprob_entropy_fwd": ([_vp] * 8 + [_i32, _i32, _i64, _f32, _i32, _f32, _vp], C.c_int),
    "dta_logprob_entropy_shard_stats": ([_vp] * 6 + [_i32, _i32, _i64, _f32, _i32, _f32, _vp], C.c_int),
    "dta_logprob_entropy_bwd": ([_vp] * 10 + [_i32, _i32, _i64, _i64, _f32, _i32, _f32, _vp], C.c_int),
    "dta_rmsnorm_fwd": ([_vp] * 6 + [_i32, _i32, _f32, _f32, _i32, _vp], C.c_int),
    "dta_rmsnorm_bwd_blocks": ([_i32], C.c_int),
    "dta_rmsnorm_bwd": ([_vp] * 7 + [_i32, _i32, _f32, _i32, _vp], C.c_int),
    "dta_layernorm_fwd": ([_vp] * 8 + [_i32, _i32, _f32, _i32, _vp], C.c_int),
    "dta_layernorm_bwd_blocks": ([_i32], C.c_int),
    "dta_layernorm_bwd": ([_vp] * 8 + [_i32, _i32, _i32, _vp], C.c_int),
    "dta_qk_norm_rope_fwd": ([_vp] * 5 + [_i32, _i32, _i32, _i64, _f32, _i32, _vp], C.c_int),
    "dta_qk_norm_rope_bwd_blocks": ([_i64], C.c_int),
    "dta_qk_norm_rope_bwd": ([_vp] * 7 + [_i32, _i32, _i32, _i64, _i64, _i64, _i64, _i32, _vp], C.c_int),
    "dta_rope_partial_fwd": ([_vp] * 3 + [_i32] * 5 + [_i64, _i32, _vp], C.c_int),
    "dta_rope_partial_bwd": ([_vp] * 3 + [_i32] * 5 + [_i64, _i64, _i64, _i32, _vp], C.c_int),
    "dta_wide_qk_norm_rope_fwd": ([_vp] * 5 + [_i32, _i32, _i32, _i64, _f32, _i32, _vp], C.c_int),
    "dta_wide_qk_norm_rope_bwd_blocks": ([_i32], C.c_int),
    "dta_wide_qk_norm_rope_bwd": ([_vp] * 7 + [_i32, _i32, _i32, _i64, _i64, _i64, _i64, _i32, _vp], C.c_int),
    "dta_rmsnorm_add_fwd": ([_vp] * 6 + [_i32, _i32, _f32, _i32, _vp], C.c_int),
    "dta_swiglu_fwd": ([_vp] * 3 + [_i64, _i32, _i64, _i32, _vp], C.c_int),
    "dta_swiglu_bwd": ([_vp] * 5 + [_i64, _i32, _i64, _i64, _i32, _vp], C.c_int),
    "dta_geglu_fwd": ([_vp] * 3 + [_i64, _i32, _i64, _i32, _vp], C.c_int),
    "dta_geglu_bwd": ([_vp] * 5 + [_i64, _i32, _i64, _i64, _i32, _vp], C.c_int),
    "dta_transpose": ([_vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp], C.c_int),
    "dta_sum_slabs": ([_vp, _i64, _i64, _i64, _vp, _vp, _i32, _vp], C.c_int),
    "dta_moe_router_fwd": ([_vp] * 4 + [_i32] * 5 + [_vp], C.c_int),
    "dta_moe_router_bwd": ([_vp] * 5 + [_i32] * 5 + [_vp], C.c_int),
    "dta_moe_permute_workspace": ([_i32, _i32], C.c_int),
    "dta_moe_tile_bound": ([_i32, _i32], C.c_int),
    "dta_moe_permute": ([_vp, _i32, _i32, _i32] + [_vp] * 5 + [_vp], C.c_int),
    "dta_moe_grouped_gemm": ([_i32] + [_vp] * 7 + [_i32] * 5 + [_vp], C.c_int),
    "dta_moe_combine_fwd": ([_vp] * 4 + [_i32] * 4 + [_vp], C.c_int),
    "dta_moe_combine_bwd": ([_vp] * 6 + [_i32] * 4 + [_vp], C.c_int),
    "dta_lora_down": ([_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp], C.c_int),
    "dta_lora_wgrad_slabs": ([_i32, _i32], C.c_int),
    "dta_lora_wgrad": ([_vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp], C.c_int),
    "dta_policy_loss_blocks": ([_i32, _i32], C.c_int),
    # lp ent depth row_seq_lo row_seq_hi seq_ptr leaf_run_ptr run_row0 run_depth0 seq_leaf old_lp ref_lp rollout_lp mask adv | adv_per_seq |
    # w c omega dlp dent partial stats | T S M R | clip_low clip_high dual_clip kl_coef | kl_estimator | entropy_coef | agg | scale |
    # ratio_level surrogate is_level is_mode | is_cap is_floor | stream
    "dta_policy_loss": ([_vp] * 15 + [_i32] + [_vp] * 7 + [_i32] * 4 + [_f32] * 4 + [_i32, _f32, _i32, _f32] + [_i32] * 4 + [_f32, _f32, _vp],
                        C.c_int),
    "dta_preference_loss_blocks": ([_i32, _i32, _i32], C.c_int),
    # lp depth row_seq_lo row_seq_hi seq_ptr leaf_run_ptr run_row0 run_depth0 seq_leaf pair_c pair_r ref_lp ref_sum mask |
    # nhat u sft g dlp partial stats | T S M R P kind | beta label_smoothing gamma | length_normalize reference_free | sft_coef scale | stream
    "dta_preference_loss": ([_vp] * 21 + [_i32] * 6 + [_f32] * 3 + [_i32, _i32, _f32, _f32, _vp], C.c_int),
    "dta_quant_blockwise": ([_vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp], C.c_int),
    "dta_dequant_blockwise": ([_vp, _vp, _i64, _i64, _i32, _vp, _i64, _i32, _i32, _vp], C.c_int),
}
EXPORTS = tuple(_PROTOS)
_ERR = {-1: "DTA_EINVAL", -2: "DTA_EUNSUPPORTED", -3: "DTA_EALIGN", -4: "DTA_ELAUNCH", -5: "DTA_EPRIOR"}


def _hip_runtimes_mapped():
    """Paths of every libamdhip64 mapped into this process (Linux)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    except OSError:
        return []


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError(f"{LIB} is missing: run `python -m dynamictreeattn_amd.build` (hipcc, gfx950). "
                               "There is no CPU fallback for the hot path.")
        # torch ships its own libamdhip64; it must be resident BEFORE this library so that both resolve
        # to ONE HIP runtime (otherwise torch's streams/pointers are foreign to our kernels: launches fail).
        import torch  # noqa: F401
        l = C.CDLL(LIB)
        rts = _hip_runtimes_mapped()
        if len(rts) > 1:
            # two HIP runtimes = two sets of streams/contexts: torch's device pointers are foreign to our kernels and
            # every launch fails (round 1: "dta_lcp_adjacent failed: DTA_ELAUNCH").  Refuse to run like that.
            raise RuntimeError("more than one libamdhip64 is mapped into this process: " + ", ".join(rts) +
                               " — libdta_mi355x.so must resolve to the HIP runtime torch ships")
        for name, (args, res) in _PROTOS.items():
            fn = getattr(l, name)
            fn.argtypes, fn.restype = args, res
        _lib = l
    return _lib


def check(status: int, what: str):
    if status == 0:
        return
    if status == -5:
        buf = C.create_string_buffer(256)
        code = lib().dta_take_pending_error(buf, 256)
        raise RuntimeError(f"{what}: not launched, a HIP error was already pending on this thread: {buf.value.decode() or code} "
                           f"(hipError {code}; now cleared — after an asynchronous kernel fault the GPU context stays unusable)")
    raise RuntimeError(f"{what} failed: {_ERR.get(status, status)}")


def ptr(t):
    return None if t is None else t.data_ptr()
