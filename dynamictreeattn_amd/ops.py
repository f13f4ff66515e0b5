"""torch-facing operators over the C ABI (include/dta.h).  PyTorch supplies device memory, streams
and autograd plumbing only; all arithmetic of these ops runs in the HIP kernels."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import packing
from ._lib import check, lib, ptr

# DTA_BF16 / DTA_F16: the MFMA kernels; DTA_F32: fp32 models (plain-FMA attention of tree_attn_f32.hip, fp32 row kernels)
_DT = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


class _on:
    """Launch context of one operator call: every operand must live on ONE MI355X; the kernels go to THAT device's
    current stream with that device made current for the call — so the reference's form
    ``TreeTrainingEngine(cfg, 'cuda:1', ...)`` works without a prior ``torch.cuda.set_device`` (a launch on device 0
    against device-1 pointers is a memory fault).  ``with _on(a, b) as stream: lib().dta_*(…, stream)``."""
    __slots__ = ("dev", "_guard")

    def __init__(self, *ts):
        dev = None
        for t in ts:
            if t is None:
                continue
            if not t.is_cuda:
                raise RuntimeError("dynamictreeattn_amd ops run on the MI355X only (tensor is on %s); there is no CPU path" % t.device)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError(f"operands of one dynamictreeattn_amd op live on different devices ({dev} and {t.device})")
        if dev is None:
            raise RuntimeError("dynamictreeattn_amd op called without a device tensor")
        self.dev, self._guard = dev, None

    def __enter__(self):
        if torch.cuda.current_device() != self.dev.index:
            self._guard = torch.cuda.device(self.dev)
            self._guard.__enter__()
        return torch.cuda.current_stream(self.dev).cuda_stream

    def __exit__(self, *exc):
        if self._guard is not None:
            self._guard.__exit__(*exc)
        return False


class KernelTimer:
    """Optional live timing of the C-ABI launches with HIP events recorded on the launch stream (bench.py's roofline leg).
    Disabled unless `KernelTimer.active` is set to an instance.  `spans[name]` = [(start event, end event, algorithmic bytes)]."""
    active: Optional["KernelTimer"] = None

    def __init__(self):
        from collections import defaultdict
        self.spans = defaultdict(list)
        for k in ("fwd", "bwd_dq", "bwd_dkv", "bwd_dkv_finalize"):
            self.spans[k]

    def span(self, name, nbytes: int = 0):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.spans[name].append((a, b, nbytes))
        return a, b

    def totals_ms(self):
        torch.cuda.synchronize()
        return {k: (sum(s[0].elapsed_time(s[1]) for s in v), len(v)) for k, v in self.spans.items()}

    def totals_bytes(self):
        return {k: sum(s[2] for s in v) for k, v in self.spans.items()}


def _require_cuda(*ts):
    _on(*ts)


def free_hbm(device) -> int:
    """HBM THIS PROCESS can still use on `device`: the smaller of
    * what the driver reports free on the card (device-wide: other processes' allocations are already taken out) plus what
      torch's caching allocator holds without using (after the first step most of the card is 'reserved'), and
    * what is left under this process's allocator cap (`torch.cuda.set_per_process_memory_fraction`: ranks that share a card,
      or a co-tenant's reservation) - `mem_get_info` alone knows nothing about that cap, so every rank of a shared card used to
      size its logits / activation budgets from the WHOLE free card."""
    free, total = torch.cuda.mem_get_info(device)
    alloc, reserved = torch.cuda.memory_allocated(device), torch.cuda.memory_reserved(device)
    usable = free + reserved - alloc
    frac = torch.cuda.get_per_process_memory_fraction(device)
    if frac < 1.0:
        usable = min(usable, int(frac * total) - alloc)
    return max(int(usable), 0)


def _launch(name: str, tensors, *args, nbytes: int = 0, span: Optional[str] = None):
    """One C-ABI call on the device / current stream of `tensors` (see _on); raises on a non-zero status.
    `nbytes`: algorithmic HBM bytes of the launch (one read of every input, one write of every output) for the roofline leg;
    `span`: the KernelTimer name of the launch (default: the entry point's)."""
    tm = KernelTimer.active
    with _on(*tensors) as stream:
        if tm is not None:
            a, b = tm.span(span or name, nbytes); a.record()
        st = getattr(lib(), name)(*args, stream)
        if tm is not None:
            b.record()
    check(st, name)


@dataclass
class TreeAttnMeta:
    """Device-resident visibility metadata of one packed trie (or None fields for the stack form).  window > 0: a sliding-window
    layer (key s visible to row t only if depth[t] - depth[s] < window); then win_lo [T] holds each row's lowest visible key (packed
    form; None in the stack form) and run_ptr / runs / ktile_qend / dK/dV units are the windowed plan's (window_meta)."""
    T: int
    subtree_end: Optional[torch.Tensor]      # int32 [T]
    run_ptr: Optional[torch.Tensor]          # int32 [nqt+1]
    runs: Optional[torch.Tensor]             # int32 [nruns,4]
    ktile_qend: Optional[torch.Tensor]       # int32 [nkt]
    q_offset: int = 0
    dkv_units: Optional[torch.Tensor] = None     # int32 [n,4] balanced work units of the dK/dV sweep (packing.plan_dkv_units)
    dkv_splits: Optional[torch.Tensor] = None    # int32 [m,4]
    n_slabs: int = 0
    win_lo: Optional[torch.Tensor] = None        # int32 [T] (packing.window_lo_host / dta_window_lo)
    window: int = 0


def ktile_qend_from(subtree_end: torch.Tensor, tile: int = packing.KTILE) -> torch.Tensor:
    T = subtree_end.numel()
    nkt = (T + tile - 1) // tile
    pad = nkt * tile - T
    se = torch.nn.functional.pad(subtree_end, (0, pad), value=0) if pad else subtree_end
    return se.view(nkt, tile).amax(dim=1).to(torch.int32).contiguous()


def _strides(t):
    if t.stride(-1) != 1:
        raise ValueError("head_dim must be contiguous")
    return t.stride(0), t.stride(1)


def _cap_of(softcap) -> float:
    """A model's soft-cap as the kernels take it: None / 0 = no cap (the uncapped kernels); negative, NaN or infinite is refused."""
    c = float(softcap or 0.0)
    if not (0.0 <= c < float("inf")):
        raise ValueError(f"softcap must be a finite number >= 0 (got {softcap!r})")
    return c


def attn_fwd_raw(q, k, v, meta: TreeAttnMeta, scale: float, softcap: float = 0.0):
    """softcap > 0: scores softcap * tanh(scale q.k / softcap), capped before the visibility mask."""
    softcap = _cap_of(softcap)
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    out = torch.empty((Tq, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((Hq, Tq), dtype=torch.float32, device=q.device)          # head-major: rows of one head are contiguous
    (qs, qh), (ks, kh), (vs, vh), (os_, oh) = _strides(q), _strides(k), _strides(v), _strides(out)
    _launch("dta_tree_attn_fwd", (q, k, v, meta.subtree_end, meta.runs, meta.win_lo),
            ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(meta.subtree_end), ptr(meta.run_ptr), ptr(meta.runs),
            Tq, Tk, meta.q_offset, Hq, Hkv, D, qs, qh, ks, kh, vs, vh, os_, oh, float(scale), _DT[q.dtype],
            ptr(meta.win_lo) if meta.window > 0 else None, int(meta.window), softcap, span="fwd")
    return out, lse, k, v


def attn_bwd_raw(q, k, v, out, dout, lse, meta: TreeAttnMeta, scale: float, dk=None, dv=None, accumulate=False, dq=None, softcap: float = 0.0):
    """dq/dk/dv may be given as output buffers (row stride, head stride; dk and dv with the SAME strides).  softcap: the forward's."""
    softcap = _cap_of(softcap)
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    if dout.stride() != out.stride():
        dout = dout.contiguous(); out = out.contiguous()
    if dq is None:
        dq = torch.empty((Tq, Hq, D), dtype=q.dtype, device=q.device)
    if dk is None:
        dk = torch.empty((Tk, Hkv, D), dtype=q.dtype, device=q.device); dv = torch.empty_like(dk)
    delta = torch.empty((Hq, Tq), dtype=torch.float32, device=q.device)
    (qs, qh), (ks, kh), (vs, vh), (os_, oh), (dqs, dqh), (dks, dkh) = _strides(q), _strides(k), _strides(v), _strides(out), _strides(dq), _strides(dk)
    units, splits = meta.dkv_units, meta.dkv_splits
    n_units = units.shape[0] if units is not None else 0
    n_splits = splits.shape[0] if splits is not None else 0
    if q.dtype == torch.float32:            # the fp32 path sweeps one key block per workgroup: no split-Q units, no slabs
        units = splits = None; n_units = n_splits = 0
    ws = torch.empty((meta.n_slabs, Hkv, 2, packing.KTILE, D), dtype=torch.float32, device=q.device) if (units is not None and meta.n_slabs) else None

    def launch(which, span=None):
        _launch("dta_tree_attn_bwd", (q, k, v, out, dout, lse, dk, dv, meta.subtree_end, units, meta.win_lo),
                ptr(q), ptr(k), ptr(v), ptr(out), ptr(dout), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
                ptr(meta.subtree_end), ptr(meta.run_ptr), ptr(meta.runs), ptr(meta.ktile_qend),
                Tq, Tk, meta.q_offset, Hq, Hkv, D, qs, qh, ks, kh, vs, vh, os_, oh, dqs, dqh, dks, dkh,
                float(scale), _DT[q.dtype], int(accumulate), which,
                ptr(units), n_units, ptr(splits) if n_splits else None, n_splits, ptr(ws),
                ptr(meta.win_lo) if meta.window > 0 else None, int(meta.window), softcap, span=span)
    if KernelTimer.active is None:
        launch(3)
    else:                                   # one launch per span, so that the timer's events bracket each kernel
        launch(1, "bwd_dq"); launch(2 | 8, "bwd_dkv")
        if n_splits:
            launch(4, "bwd_dkv_finalize")
    return dq, dk, dv


class AttentionTape:
    """Keeps the attention outputs (out, lse) of a no-grad forward so that a later recomputation of the same layer
    (per-layer activation recomputation in the engine) does not run the forward attention kernel again: in
    "record" mode `tree_attention` appends what it produced, in "replay" mode it takes the next entry instead of
    launching the kernel.  q, k, v come from the recomputed projections either way (the backward needs them), and so do the call's scale
    and soft-cap: the replayed call's own arguments go into its backward, so a capped layer whose forward kernel was skipped still runs the
    capped backward (an entry also records the cap it was produced under, and a replay under another cap is refused)."""
    current = None

    def __init__(self, mode: str, items=None):
        assert mode in ("record", "replay")
        self.mode, self.items, self.pos = mode, ([] if items is None else items), 0

    def __enter__(self):
        self._prev, AttentionTape.current = AttentionTape.current, self
        return self

    def __exit__(self, *exc):
        AttentionTape.current = self._prev
        return False


class _TreeAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, meta: TreeAttnMeta, scale: float, softcap: float = 0.0):
        tape = AttentionTape.current
        if tape is not None and tape.mode == "replay" and tape.pos < len(tape.items):
            out, lse, *cap = tape.items[tape.pos]; tape.pos += 1
            if out.shape != q.shape:
                raise RuntimeError("attention replay: recorded output does not match the recomputed query")
            if cap and cap[0] != softcap:
                raise RuntimeError(f"attention replay: recorded under softcap {cap[0]}, replayed under {softcap}")
        else:
            out, lse, k, v = attn_fwd_raw(q, k, v, meta, scale, softcap)
            if tape is not None and tape.mode == "record":
                tape.items.append((out, lse, softcap))
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.meta, ctx.scale, ctx.softcap = meta, scale, softcap
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        Hq, Hkv = q.shape[1], k.shape[1]
        if q.shape[0] == k.shape[0]:
            # the three gradients side by side in ONE [T, Hq+2Hkv, D] buffer, the layout of the fused projection's gradient: the q|k|v
            # prep's backward recognises it (_fused_grad_buffer: what is built here must satisfy it), transforms dq and dk in place and
            # hands the buffer on - no gather of dv (0.65 ms per step at tau2 size)
            fused = torch.empty((q.shape[0], Hq + 2 * Hkv, q.shape[2]), dtype=q.dtype, device=q.device)
            dq, dk, dv = fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
            attn_bwd_raw(q, k, v, out, dout, lse, ctx.meta, ctx.scale, dk=dk, dv=dv, dq=dq, softcap=ctx.softcap)
        else:
            dq, dk, dv = attn_bwd_raw(q, k, v, out, dout, lse, ctx.meta, ctx.scale, softcap=ctx.softcap)
        return dq, dk, dv, None, None, None


class _StackAttention(torch.autograd.Function):
    """Attention of a block of B new rows at stack positions [start, start+B) over the KV STACK in place (the form of
    tree_training_engine.py:171-186, 339-353 without `DynamicCache`/`torch.cat`): forward writes the block's K/V into the
    stack rows and attends rows [0, start+B) rectangular-causally; backward adds this block's dK/dV into the fp32 grad
    stacks for ALL rows [0, start+B) (`accumulate = 2`; replaces the prefix-sized `.grad` tensors and `+=` of tte:447-451)
    and returns, as the gradient of the block's own K/V, what the grad stack now holds for its rows — i.e. the
    contributions of every already-popped descendant plus the block's own."""

    @staticmethod
    def forward(ctx, q, k_new, v_new, kst, vst, gk, gv, start, scale, window, softcap=0.0):
        B = q.shape[0]
        end = start + B
        kst[start:end].copy_(k_new); vst[start:end].copy_(v_new)
        meta = stack_meta(start, window)
        out, lse, _, _ = attn_fwd_raw(q, kst[:end], vst[:end], meta, scale, softcap)
        ctx.save_for_backward(q, out, lse)
        ctx.stacks, ctx.meta, ctx.scale, ctx.span, ctx.softcap = (kst, vst, gk, gv), meta, scale, (start, end), softcap
        return out

    @staticmethod
    def backward(ctx, dout):
        q, out, lse = ctx.saved_tensors
        kst, vst, gk, gv = ctx.stacks
        start, end = ctx.span
        dq, _, _ = attn_bwd_raw(q, kst[:end], vst[:end], out, dout, lse, ctx.meta, ctx.scale, dk=gk[:end], dv=gv[:end], accumulate=2,
                                softcap=ctx.softcap)
        return dq, gk[start:end].to(q.dtype), gv[start:end].to(q.dtype), None, None, None, None, None, None, None, None


def stack_attention(q, k_new, v_new, kst, vst, gk, gv, start: int, scale: Optional[float] = None, window: int = 0, softcap: float = 0.0):
    """q [B,Hq,D], k_new/v_new [B,Hkv,D] at stack positions start..start+B-1; kst/vst [cap,Hkv,D] (model dtype),
    gk/gv [cap,Hkv,D] fp32 grad stacks (may be None under no_grad) -> out [B,Hq,D] (D = head_dim, 64 or 128).
    window > 0: sliding window, row t sees stack rows (t - window, t] (the whole stack is kept either way).
    softcap > 0: scores softcap * tanh(scale q.k / softcap), capped before the mask."""
    if q.dtype not in _DT:
        raise TypeError("stack_attention supports bf16 / f16 / f32 (got %s)" % q.dtype)
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    return _StackAttention.apply(q, k_new, v_new, kst, vst, gk, gv, start, scale, int(window), _cap_of(softcap))


def tree_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, meta: TreeAttnMeta, scale: Optional[float] = None,
                   softcap: float = 0.0) -> torch.Tensor:
    """q [T,Hq,D], k/v [T,Hkv,D] packed in DFS pre-order -> out [T,Hq,D] (D = head_dim, 64 or 128).  Differentiable.
    softcap > 0: scores softcap * tanh(scale q.k / softcap), capped before the visibility mask (Gemma-2)."""
    if q.dtype not in _DT:
        raise TypeError("tree_attention supports bf16 / f16 / f32 (got %s)" % q.dtype)
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    return _TreeAttention.apply(q, k, v, meta, scale, _cap_of(softcap))


def stack_meta(start: int, window: int = 0) -> TreeAttnMeta:
    """Rectangular-causal stack form: query i sits at stack position start+i (tte:171-186); window > 0: it sees only the
    positions (start + i - window, start + i]."""
    return TreeAttnMeta(T=0, subtree_end=None, run_ptr=None, runs=None, ktile_qend=None, q_offset=start, window=max(int(window), 0))


def attach_dkv_units(meta: TreeAttnMeta, Hkv: int) -> TreeAttnMeta:
    """Plans the balanced dK/dV work units from ktile_qend (one small D2H read) and uploads them."""
    kq = meta.ktile_qend.cpu().numpy()
    units, splits, n_slabs = packing.plan_dkv_units(kq, meta.T, meta.T, meta.q_offset, Hkv)
    dev = meta.ktile_qend.device
    meta.dkv_units = torch.from_numpy(units).to(dev).contiguous()
    meta.dkv_splits = torch.from_numpy(splits).to(dev).contiguous() if splits.shape[0] else None
    meta.n_slabs = n_slabs
    return meta


def meta_from_plan(plan: packing.SegmentPlan, subtree_end: torch.Tensor, device, Hkv: int = 8) -> TreeAttnMeta:
    rp, runs = packing.plan_qtile_runs(plan)
    meta = TreeAttnMeta(T=plan.T, subtree_end=subtree_end,
                        run_ptr=torch.from_numpy(rp).to(device), runs=torch.from_numpy(runs).to(device).contiguous(),
                        ktile_qend=ktile_qend_from(subtree_end))
    return attach_dkv_units(meta, Hkv)


def window_lo_device(depth: torch.Tensor, seg_off: torch.Tensor, seg_depth0: torch.Tensor, parent_of_seg: torch.Tensor,
                     window: int) -> torch.Tensor:
    """win_lo [T] of a packed trie on the device (dta_window_lo): depth from dta_preorder_meta, the segment tables of its plan."""
    T, M = depth.numel(), parent_of_seg.numel()
    out = torch.empty(T, dtype=torch.int32, device=depth.device)
    _launch("dta_window_lo", (depth,), ptr(depth), ptr(seg_off), ptr(seg_depth0), ptr(parent_of_seg), M, T, int(window), ptr(out))
    return out


def window_meta(meta: TreeAttnMeta, plan: packing.SegmentPlan, depth: torch.Tensor, window: int, Hkv: int = 8, seg_tables=None) -> TreeAttnMeta:
    """The sliding-window meta of a packed trie from its full meta: win_lo on the device (dta_window_lo), the windowed tile plan
    (packing.plan_qtile_runs_window: query tiles visit O(window) keys), the tighter dK/dV query ends and their work units.  Build
    it once per distinct window per call and share it between layers.  window <= 0, or wider than the deepest token: `meta`
    itself (the unwindowed kernels, bit for bit).  seg_tables: (seg_off, seg_depth0, parent_of_seg) already on the device."""
    if window <= 0 or window > packing.max_depth(plan):
        return meta
    dev = depth.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    if seg_tables is None:
        seg_tables = (up(plan.seg_off), up(plan.seg_depth0), up(plan.parent_of_seg))
    win_lo = window_lo_device(depth, *seg_tables, window)
    wl_host = packing.window_lo_host(plan, window)
    rp, runs = packing.plan_qtile_runs_window(plan, wl_host)
    kq = packing.ktile_qend_window(packing.ktile_qend_host(plan), wl_host)
    units, splits, n_slabs = packing.plan_dkv_units(kq, plan.T, plan.T, 0, Hkv)
    return TreeAttnMeta(T=plan.T, subtree_end=meta.subtree_end, run_ptr=up(rp), runs=up(runs).view(-1, 4), ktile_qend=up(kq),
                        dkv_units=up(units).view(-1, 4), dkv_splits=up(splits).view(-1, 4) if splits.shape[0] else None, n_slabs=n_slabs,
                        win_lo=win_lo, window=int(window))


# --------------------------------------------------------------------------------------------------
# LM head + log-prob / entropy over packed rows (HIP statistics kernels around hipBLASLt GEMMs)
# --------------------------------------------------------------------------------------------------
def logprob_entropy_fwd_raw(logits, labels, want_entropy=True, temperature=1.0, extra_ptr=None, extra_labels=None, extra_out=None, softcap=0.0):
    """logits [R,V] bf16/f16/f32 (row-contiguous) -> (lse, entropy|None, logprob|None) fp32 [R].
    `extra_ptr` int32 [R+1] / `extra_labels` int64 [F]: further labels per row (CSR, absolute indices); their
    log-probs are written to `extra_out` fp32 [F] (rows of this call only)."""
    R, V = logits.shape
    lse = torch.empty(R, dtype=torch.float32, device=logits.device)
    ent = torch.empty_like(lse) if want_entropy else None
    lp = torch.empty_like(lse) if labels is not None else None
    _launch("dta_logprob_entropy_fwd", (logits, labels, extra_ptr, extra_labels, extra_out),
            ptr(logits), ptr(labels), ptr(extra_ptr), ptr(extra_labels), ptr(lse), ptr(ent), ptr(lp), ptr(extra_out),
            R, V, logits.stride(0), float(temperature), _DT[logits.dtype], float(softcap), nbytes=R * V * logits.element_size())
    return lse, ent, lp


def logprob_entropy_bwd_raw(logits, labels, lse, ent, g_lp, g_ent, temperature=1.0, extra_ptr=None, extra_labels=None, g_extra=None, out=None,
                            softcap=0.0):
    """dLoss/dlogits into `out` (None: IN PLACE over `logits`)."""
    R, V = logits.shape
    out = logits if out is None else out
    _launch("dta_logprob_entropy_bwd", (logits, out, labels, extra_ptr, extra_labels, lse, g_lp, g_extra, g_ent),
            ptr(logits), ptr(out), ptr(labels), ptr(extra_ptr), ptr(extra_labels), ptr(lse), ptr(ent), ptr(g_lp), ptr(g_extra), ptr(g_ent),
            R, V, logits.stride(0), out.stride(0), float(temperature), _DT[logits.dtype], float(softcap), nbytes=2 * R * V * logits.element_size())
    return out


def logprob_entropy_shard_stats_raw(logits, labels_local, temperature=1.0, extra_ptr=None, extra_labels=None, extra_out=None, softcap=0.0):
    """Per-shard statistics [R,4] = {m, s, t, picked} (log2 domain) of logits [R, V/tp]; see dta.h.  Extra picks -> raw x/T or 0."""
    R, V = logits.shape
    stats = torch.empty((R, 4), dtype=torch.float32, device=logits.device)
    _launch("dta_logprob_entropy_shard_stats", (logits, labels_local, extra_ptr, extra_labels, extra_out),
            ptr(logits), ptr(labels_local), ptr(extra_ptr), ptr(extra_labels), ptr(stats), ptr(extra_out),
            R, V, logits.stride(0), float(temperature), _DT[logits.dtype], float(softcap), nbytes=R * V * logits.element_size())
    return stats


_LN2 = 0.6931471805599453


def combine_shard_stats(stats, extra_sum, group):
    """Cross-rank combine of the per-shard statistics: ONE MAX all-reduce, then ONE packed SUM all-reduce
    (s, t, picked and `extra_sum`, the raw logits picked for fork children) — vocab_parallel.py:134,142,156 /
    264,273,291,298 issue 3-4 separate latency-bound reductions per chunk.  Returns (lse, ent, picked, extra)."""
    import torch.distributed as dist
    m = stats[:, 0].contiguous()
    M = m.clone()
    dist.all_reduce(M, op=dist.ReduceOp.MAX, group=group)
    f = torch.exp2(m - M)
    R = stats.shape[0]
    packed = torch.cat([stats[:, 1] * f, stats[:, 2] * f, stats[:, 3], extra_sum])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    S, Tt, picked, extra = packed[:R], packed[R:2 * R], packed[2 * R:3 * R], packed[3 * R:]
    lse = (M + torch.log2(S)) * _LN2
    ent = lse - (Tt / S) * _LN2
    return lse, ent, picked, extra


def local_labels(t, vocab_offset, V):
    """Global token ids -> ids inside the vocabulary slice [vocab_offset, vocab_offset + V); -1 = owned by another rank."""
    return torch.where((t >= vocab_offset) & (t < vocab_offset + V), t - vocab_offset, torch.full_like(t, -1))


def _head_logits(h, W):
    """h Wᵀ [R, V] as the log-prob kernels read it: rows on a pitch of a multiple of 8 elements (16-byte vector loads).  A vocabulary
    (or a rank's slice of one) that is no multiple of 8 gets rows with padding behind them, which nothing reads."""
    V = W.shape[0]
    if V % 8 == 0:
        return torch.mm(h, W.t())
    buf = torch.empty((h.shape[0], (V + 7) // 8 * 8), dtype=h.dtype, device=h.device)
    return torch.mm(h, W.t(), out=buf[:, :V])


HEAD_WGRAD_FUSED_ACCUMULATE = False      # chunked head only: accumulate the weight gradient inside the GEMM (scripts/head_stage_probe.py measures both)


class _HeadRows(torch.autograd.Function):
    """(lp_next [T], lp_fork [F], ent [T]) from hidden rows: lp_next[r] = log p(next_tok[r] | row r),
    lp_fork[f] = log p(fork_tok[f] | row of f), the forks given as a CSR over the rows (`fork_ptr` int32 [T+1]; the HIP
    kernels pick them and add their one-hot gradient terms themselves).  When the model-dtype [T, V] logits fit
    `keep_bytes` they are produced by ONE GEMM, kept, turned into dLoss/dlogits IN PLACE in backward and
    consumed by one dgrad and one wgrad GEMM.  Otherwise rows go `chunk` at a time and the logits of a
    chunk are recomputed in backward (at most one [chunk, V] block alive).
    With `tp_group`, W is this rank's contiguous vocabulary slice starting at `vocab_offset` (labels stay global,
    vocab_parallel.py:128-130): per-shard statistics from the HIP kernel are combined with two all-reduces per
    chunk and the hidden-state gradient is summed across the group while the weight-gradient GEMM runs."""

    @staticmethod
    def forward(ctx, h, W, next_tok, fork_ptr, fork_tok, fork_rows, fork_bounds, want_entropy, chunk, keep_bytes, tp_group, vocab_offset, softcap=0.0,
                temperature=1.0):
        T = h.shape[0]
        dev = h.device
        V = W.shape[0]
        F_ = fork_tok.numel()
        keep = T * V * h.element_size() <= keep_bytes
        step = T if keep else chunk
        lse = torch.empty(T, dtype=torch.float32, device=dev)
        ent = torch.empty(T, dtype=torch.float32, device=dev) if (want_entropy or tp_group is not None) else None
        lp_next = torch.empty(T, dtype=torch.float32, device=dev)
        lp_fork = torch.empty(F_, dtype=torch.float32, device=dev)
        if tp_group is not None:       # shard-local label ids; -1 = owned by another rank
            next_loc, fork_loc = local_labels(next_tok, vocab_offset, V), local_labels(fork_tok, vocab_offset, V)
        else:
            next_loc, fork_loc = next_tok, fork_tok
        xp = fork_ptr if F_ else None
        kept = None
        for ci, a in enumerate(range(0, T, step)):
            b = min(a + step, T)
            logits = _head_logits(h[a:b], W)
            if tp_group is None:
                l, e, p = logprob_entropy_fwd_raw(logits, next_loc[a:b], want_entropy, temperature,
                                                  xp[a:b + 1] if F_ else None, fork_loc if F_ else None, lp_fork if F_ else None, softcap)
            else:
                f0, f1 = (0, F_) if keep else (fork_bounds[ci], fork_bounds[ci + 1])
                stats = logprob_entropy_shard_stats_raw(logits, next_loc[a:b], temperature, xp[a:b + 1] if F_ else None, fork_loc if F_ else None,
                                                        lp_fork if F_ else None, softcap)
                l, e, picked, raw = combine_shard_stats(stats, lp_fork[f0:f1], tp_group)
                p = picked - l
                if f1 > f0:
                    lp_fork[f0:f1] = raw - l[fork_rows[f0:f1] - a]
            lse[a:b] = l; lp_next[a:b] = p
            if ent is not None:
                ent[a:b] = e
            if keep:
                kept = logits
        ctx.save_for_backward(h, W, next_loc, fork_loc, lse, ent if ent is not None else lse, xp if F_ else lse)
        ctx.kept, ctx.chunk, ctx.want_entropy, ctx.tp_group, ctx.has_forks, ctx.softcap = kept, chunk, want_entropy, tp_group, bool(F_), softcap
        ctx.temperature = temperature
        return lp_next, lp_fork, (ent if want_entropy else lse.new_zeros(0))

    @staticmethod
    def backward(ctx, g_next, g_fork, g_ent):
        h, W, next_loc, fork_loc, lse, ent, xp = ctx.saved_tensors
        T = h.shape[0]
        g_next = g_next.contiguous().float()
        g_ent = g_ent.contiguous().float() if ctx.want_entropy else None
        g_fork = g_fork.contiguous().float() if ctx.has_forks else None
        kept = ctx.kept
        step = T if kept is not None else ctx.chunk
        dh = torch.empty_like(h)
        need_w = ctx.needs_input_grad[1]          # a frozen head (LoRA: the tied embedding or lm_head): no [V, hidden] product, no buffer
        dW = None if (kept is not None or not need_w) else torch.zeros(W.shape, dtype=torch.float32, device=W.device)
        pending = []
        for a in range(0, T, step):
            b = min(a + step, T)
            logits = kept if kept is not None else _head_logits(h[a:b], W)
            logprob_entropy_bwd_raw(logits, next_loc[a:b], lse[a:b], ent[a:b] if ctx.want_entropy else None, g_next[a:b],
                                    g_ent[a:b] if ctx.want_entropy else None, ctx.temperature,
                                    xp[a:b + 1] if ctx.has_forks else None, fork_loc if ctx.has_forks else None, g_fork, softcap=ctx.softcap)
            if W.dtype in (torch.bfloat16, torch.float16) and (b - a) >= 4096 and W.shape[0] % 8 == 0 and W.shape[1] % 8 == 0:
                torch.mm(logits, _TransposedWeights.get(W).t(), out=dh[a:b])        # contraction index contiguous in both operands (see _dgrad)
            else:
                torch.mm(logits, W, out=dh[a:b])
            if ctx.tp_group is not None:       # each rank saw only its vocabulary slice: sum dh while the wgrad GEMM runs
                import torch.distributed as dist
                pending.append(dist.all_reduce(dh[a:b], op=dist.ReduceOp.SUM, group=ctx.tp_group, async_op=True))
            if not need_w:
                pass
            elif kept is not None:
                dW = torch.mm(logits.t(), h)                 # one wgrad GEMM over all T rows (fp32 accumulate inside)
            elif HEAD_WGRAD_FUSED_ACCUMULATE:
                dW = torch.addmm(dW, logits.t(), h[a:b], out_dtype=torch.float32)      # hipBLASLt: 16-bit operands, fp32 C/D - no [V, hidden] temporary
            else:
                dW += torch.mm(logits.t(), h[a:b])
        ctx.kept = None
        for w in pending:
            w.wait()
        return dh, (dW.to(W.dtype) if need_w else None), None, None, None, None, None, None, None, None, None, None, None, None


MAX_CAPPED_PICKS_PER_ROW = 2048     # dta.h: extra picks of one row in the in-place backward of the capped log-prob kernel


def lm_head_rows(h, W, next_tok, fork_ptr, fork_tok, fork_rows, fork_bounds, want_entropy, chunk, keep_bytes=None, tp_group=None, vocab_offset=0,
                 softcap: float = 0.0, max_picks_per_row: Optional[int] = None, temperature: float = 1.0):
    """See _HeadRows.  `fork_ptr` int32 [T+1]: CSR of the forks over the rows; `fork_rows` int64 [F] their rows (ascending);
    `fork_bounds[c] .. fork_bounds[c+1]` = the forks whose row lies in chunk c (host list; used by the vocabulary-split path).
    softcap > 0: final-logit soft-capping - every statistic is taken on softcap * tanh(logit / softcap), inside the kernels (the
    [chunk, V] logits get no extra pass).  `max_picks_per_row`: the largest number of forks on one row, from the caller's host tables;
    it is checked against the capped kernel's limit (None: unknown - beyond the limit the kernel writes NaN for the pick, dta.h).
    `temperature`: every statistic is taken on logit / temperature, inside the kernels (a model with a logit scale s passes 1 / s:
    model.logit_scale_of); 1.0 is the plain head."""
    _require_cuda(h, W)
    temperature = float(temperature)
    if not (0.0 < temperature < float("inf")):
        raise ValueError(f"temperature must be a finite number > 0 (got {temperature!r})")
    softcap = _cap_of(softcap)
    if softcap > 0 and max_picks_per_row is not None and max_picks_per_row > MAX_CAPPED_PICKS_PER_ROW:
        raise ValueError(f"a row with {max_picks_per_row} fork picks exceeds the capped log-prob kernel's {MAX_CAPPED_PICKS_PER_ROW} per row")
    if keep_bytes is None:
        keep_bytes = free_hbm(h.device) // 4
    if tp_group is not None:
        # keeping or chunking the logits sets the NUMBER of collectives below: the ranks of the group must take the same branch
        # whatever their own free memory is - keep only if every rank can
        import torch.distributed as dist
        ok = torch.tensor([1 if h.shape[0] * W.shape[0] * h.element_size() <= keep_bytes else 0], device=h.device, dtype=torch.int32)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=tp_group)
        keep_bytes = (1 << 62) if int(ok.item()) else 0
    lp_next, lp_fork, ent = _HeadRows.apply(h, W, next_tok, fork_ptr, fork_tok, fork_rows, fork_bounds, want_entropy, chunk, keep_bytes,
                                            tp_group, vocab_offset, softcap, temperature)
    return lp_next, lp_fork, (ent if want_entropy else None)


class _LogProbEntropyHIP(torch.autograd.Function):
    """The public ``gather_logprobs(_entropy)`` of vocab_parallel.py:399-467 on the HIP kernels: logits [R, V] in bf16 / f16 /
    f32 (the reference up-casts with ``.float()``; the kernels read the stored dtype and do all arithmetic in fp32, which
    is the same thing), labels int64 [R] with -1 = no label.  Backward writes dLoss/dlogits out of place (the caller's
    logits stay intact) in the logits' dtype, as autograd through ``.float()`` does."""

    @staticmethod
    def forward(ctx, logits, labels, temperature, want_entropy):
        lse, ent, lp = logprob_entropy_fwd_raw(logits, labels, want_entropy, temperature)
        ctx.save_for_backward(logits, labels, lse, ent if ent is not None else lse)
        ctx.temperature, ctx.want_entropy = temperature, want_entropy
        return lp, (ent if want_entropy else lse.new_zeros(0))

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        logits, labels, lse, ent = ctx.saved_tensors
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=logits.device)
        logprob_entropy_bwd_raw(logits, labels, lse, ent if ctx.want_entropy else None, g_lp.contiguous().float(),
                                g_ent.contiguous().float() if ctx.want_entropy else None, ctx.temperature, out=out)
        return out, None, None, None


class _ShardedLogProbEntropyHIP(torch.autograd.Function):
    """Vocabulary-sharded form (vocab_parallel.py:82-370) on the HIP kernels: per-shard statistics, ONE MAX + ONE packed SUM
    all-reduce for all rows (the reference issues 3-4 per 1024-row chunk), backward on the shard with shard-local labels."""

    @staticmethod
    def forward(ctx, logits, labels_local, temperature, want_entropy, group):
        stats = logprob_entropy_shard_stats_raw(logits, labels_local, temperature)
        lse, ent, picked, _ = combine_shard_stats(stats, stats.new_zeros(0), group)
        ctx.save_for_backward(logits, labels_local, lse, ent)
        ctx.temperature, ctx.want_entropy = temperature, want_entropy
        return picked - lse, (ent if want_entropy else lse.new_zeros(0))

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        logits, labels_local, lse, ent = ctx.saved_tensors
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=logits.dtype, device=logits.device)
        logprob_entropy_bwd_raw(logits, labels_local, lse, ent if ctx.want_entropy else None, g_lp.contiguous().float(),
                                g_ent.contiguous().float() if ctx.want_entropy else None, ctx.temperature, out=out)
        return out, None, None, None, None


def _rows_for_kernel(logits2d):
    """Row-contiguous [R, V] view whose row stride is a multiple of 8 elements (16-byte vector loads); copies only when needed."""
    if logits2d.stride(-1) != 1:
        logits2d = logits2d.contiguous()
    if logits2d.stride(0) % 8 or logits2d.data_ptr() % 32:
        R, V = logits2d.shape
        buf = torch.empty((R, (V + 7) // 8 * 8), dtype=logits2d.dtype, device=logits2d.device)
        view = buf[:, :V]
        view.copy_(logits2d)
        return view
    return logits2d


def logprob_entropy(logits2d, labels1d, temperature=1.0, want_entropy=True, tp_group=None):
    """(logprob [R], entropy [R] | None) of CUDA logits [R, V] through the HIP kernels; labels1d int64 [R], -1 = none.
    With `tp_group`, logits hold this rank's vocabulary slice (rank * V .. ) and labels are global ids."""
    if logits2d.dtype not in _DT:
        raise TypeError("logprob_entropy supports bf16 / f16 / f32 logits (got %s)" % logits2d.dtype)
    x = _rows_for_kernel(logits2d)
    if tp_group is None:
        lp, ent = _LogProbEntropyHIP.apply(x, labels1d, float(temperature), want_entropy)
    else:
        import torch.distributed as dist
        V = x.shape[1]
        lab = local_labels(labels1d, dist.get_rank(tp_group) * V, V)
        lp, ent = _ShardedLogProbEntropyHIP.apply(x, lab, float(temperature), want_entropy, tp_group)
    return lp, (ent if want_entropy else None)


# --------------------------------------------------------------------------------------------------
# Fused decoder-layer row kernels (RMSNorm, head-norm + RoPE, SwiGLU)
# --------------------------------------------------------------------------------------------------
def _norm_bwd(entry, x2, w, dy, g_res, stats, tail, need_w):
    """The backward of the row norms, one `entry` launch (dta_rmsnorm_bwd / dta_layernorm_bwd): (dx shaped as dy, dw | None) of the
    saved input rows x2 [R, H], the output gradient dy and the residual stream's g_res (or None), `stats` the forward's per-row
    statistics and `tail` the entry's scalars between H and the dtype.  A frozen norm weight (need_w False) is still read - dx depends
    on it - but gets no partial slab and no dta_sum_slabs."""
    R, H = x2.shape
    dy2 = dy.contiguous().view(R, H)
    gr = g_res.contiguous().view(R, H) if g_res is not None else None
    dx = torch.empty_like(x2)
    part = torch.empty(getattr(lib(), entry + "_blocks")(R), H, dtype=torch.float32, device=x2.device) if need_w else None
    _launch(entry, (x2, w, dy2, gr), ptr(x2), ptr(w), ptr(dy2), ptr(gr), *map(ptr, stats), ptr(dx), ptr(part), R, H, *tail, _DT[x2.dtype],
            nbytes=R * H * x2.element_size() * (4 if gr is not None else 3))
    return dx.view(dy.shape), (sum_slabs(part, w.dtype) if need_w else None)


class _RMSNorm(torch.autograd.Function):
    """(x_out, y) = (x + delta, rmsnorm(x + delta) * w); delta may be None (then x_out is x itself).  w_offset != 0 (Gemma: 1):
    y = rmsnorm(x + delta) * (w_offset + w) with the sum formed in fp32 inside the kernel and one rounding."""

    @staticmethod
    def forward(ctx, x, delta, w, eps, w_offset=0.0):
        _require_cuda(x, w)
        x2 = x.contiguous().view(-1, x.shape[-1])
        R, H = x2.shape
        y = torch.empty_like(x2)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        if delta is not None:
            d2 = delta.contiguous().view(R, H)
            xo = torch.empty_like(x2)
        else:
            d2, xo = None, None
        off = float(w_offset)
        _launch("dta_rmsnorm_fwd", (x2, d2, w), ptr(x2), ptr(d2), ptr(w), ptr(xo), ptr(y), ptr(rstd), R, H, float(eps), off, _DT[x.dtype],
                nbytes=R * H * x2.element_size() * (4 if delta is not None else 2))
        xin = xo if xo is not None else x2
        ctx.save_for_backward(xin, w, rstd)
        ctx.has_delta, ctx.off = delta is not None, off
        return xin.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, g_res, dy):
        x2, w, rstd = ctx.saved_tensors
        dx, dw = _norm_bwd("dta_rmsnorm_bwd", x2, w, dy, g_res, (rstd,), (ctx.off,), ctx.needs_input_grad[2])
        return dx, (dx if ctx.has_delta else None), dw, None, None


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, w_offset: float = 0.0) -> torch.Tensor:
    return _RMSNorm.apply(x, None, w, eps, float(w_offset))[1]


def add_rms_norm(x: torch.Tensor, delta: Optional[torch.Tensor], w: torch.Tensor, eps: float, w_offset: float = 0.0):
    """Residual-stream update fused with the following RMSNorm: returns (x + delta, rmsnorm(x + delta) * (w_offset + w))."""
    return _RMSNorm.apply(x, delta, w, eps, float(w_offset))


class _LayerNorm(torch.autograd.Function):
    """(x_out, y) = (x + delta_a + delta_b, LN(x_out) * w) without bias (CohereLayerNorm): mean-centred, the weight multiplied in fp32
    and one rounding.  delta_b needs delta_a; without deltas x_out is x itself.  Both deltas and x share the one input gradient."""

    @staticmethod
    def forward(ctx, x, delta_a, delta_b, w, eps):
        _require_cuda(x, w)
        if delta_b is not None and delta_a is None:
            raise ValueError("layer norm: delta_b without delta_a")
        x2 = x.contiguous().view(-1, x.shape[-1])
        R, H = x2.shape
        y = torch.empty_like(x2)
        mean = torch.empty(R, dtype=torch.float32, device=x.device)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        a2 = delta_a.contiguous().view(R, H) if delta_a is not None else None
        b2 = delta_b.contiguous().view(R, H) if delta_b is not None else None
        xo = torch.empty_like(x2) if a2 is not None else None
        n_in = 1 + (a2 is not None) + (b2 is not None)
        _launch("dta_layernorm_fwd", (x2, a2, b2, w), ptr(x2), ptr(a2), ptr(b2), ptr(w), ptr(xo), ptr(y), ptr(mean), ptr(rstd), R, H, float(eps),
                _DT[x.dtype], nbytes=R * H * x2.element_size() * (n_in + 1 + (xo is not None)))
        xin = xo if xo is not None else x2
        ctx.save_for_backward(xin, w, mean, rstd)
        ctx.deltas = (delta_a is not None, delta_b is not None)
        return xin.view(x.shape), y.view(x.shape)

    @staticmethod
    def backward(ctx, g_res, dy):
        x2, w, mean, rstd = ctx.saved_tensors
        dx, dw = _norm_bwd("dta_layernorm_bwd", x2, w, dy, g_res, (mean, rstd), (), ctx.needs_input_grad[3])
        return dx, (dx if ctx.deltas[0] else None), (dx if ctx.deltas[1] else None), dw, None


def layer_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """CohereLayerNorm: w * (x - mean) * rsqrt(var + eps) in fp32 with one rounding; no bias."""
    return _LayerNorm.apply(x, None, None, w, eps)[1]


def add_layer_norm(x: torch.Tensor, delta_a: Optional[torch.Tensor], delta_b: Optional[torch.Tensor], w: torch.Tensor, eps: float):
    """The residual join of the parallel attention || MLP block fused with the next LayerNorm: returns (x + delta_a + delta_b summed
    in fp32 and rounded once, LN of that).  Either delta may be None (delta_b only with delta_a)."""
    return _LayerNorm.apply(x, delta_a, delta_b, w, eps)


class _RMSNormAdd(torch.autograd.Function):
    """out = res + rmsnorm(y) * w in one pass (OLMo's post-norm branch end); the normalised branch itself is not kept.  The backward is
    the plain RMSNorm backward on (y, w, d out, rstd); d res = d out passes through."""

    @staticmethod
    def forward(ctx, res, y, w, eps):
        _require_cuda(res, y, w)
        H = y.shape[-1]
        y2, r2 = y.contiguous().view(-1, H), res.contiguous().view(-1, H)
        R = y2.shape[0]
        out = torch.empty_like(y2)
        rstd = torch.empty(R, dtype=torch.float32, device=y.device)
        _launch("dta_rmsnorm_add_fwd", (y2, w, r2), ptr(y2), ptr(w), ptr(r2), ptr(out), None, ptr(rstd), R, H, float(eps), _DT[y.dtype],
                nbytes=3 * R * H * y2.element_size())
        ctx.save_for_backward(y2, w, rstd)
        return out.view(y.shape)

    @staticmethod
    def backward(ctx, dout):
        y2, w, rstd = ctx.saved_tensors
        dy, dw = _norm_bwd("dta_rmsnorm_bwd", y2, w, dout, None, (rstd,), (0.0,), ctx.needs_input_grad[2])
        return dout, dy, dw, None


def rms_norm_add(res: torch.Tensor, y: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """res + rmsnorm(y) * w: the branch output is normalised and joins the residual stream in one pass (norm first, then the add -
    add_rms_norm is the other order)."""
    return _RMSNormAdd.apply(res, y, w, eps)


# A q / k member form is a pair of launch functions over one member x [T, NH, D] of the fused projection output (rows of D contiguous, any
# token stride): fwd(x, w, cos_sin, arg) -> (y contiguous, the statistic the backward needs | None) and
# bwd(x, w, cos_sin, dy, stat, dx, need_w, arg) -> dw | None, which writes dx [T, NH, D] (any token stride; may be dy: a lane reads and
# writes the same 16 bytes, partner values travel through registers).  arg: eps of the norm forms, the pairing of the partial form.
def _wide_qk_norm_rope_fwd(x, w, cos_sin, eps):
    """One dta_wide_qk_norm_rope_fwd launch over x [T, NH, D] (any token stride), w [NH*D]: (y contiguous, rstd [T])."""
    T, NH, D = x.shape
    if w.numel() != NH * D:
        raise ValueError(f"projection-wide norm weight has {w.numel()} elements for {NH} heads of {D}")
    y = torch.empty((T, NH, D), dtype=x.dtype, device=x.device)
    rstd = torch.empty(T, dtype=torch.float32, device=x.device)
    _launch("dta_wide_qk_norm_rope_fwd", (x, w, cos_sin), ptr(x), ptr(w), ptr(cos_sin), ptr(y), ptr(rstd), T, NH, D, x.stride(0), float(eps),
            _DT[x.dtype], nbytes=2 * T * NH * D * x.element_size() + T * D * 4)
    return y, rstd


def _wide_qk_norm_rope_bwd(x, w, cos_sin, dy, rstd, dx, need_w, eps=None):
    """One dta_wide_qk_norm_rope_bwd launch into dx [T, NH, D] (any token stride; may be dy).  Returns dw (None unless need_w)."""
    T, NH, D = x.shape
    if dy.stride(2) != 1:
        dy = dy.contiguous()
    part = torch.empty(lib().dta_wide_qk_norm_rope_bwd_blocks(T), NH * D, dtype=torch.float32, device=x.device) if need_w else None
    _launch("dta_wide_qk_norm_rope_bwd", (x, w, cos_sin, dy), ptr(x), ptr(w), ptr(cos_sin), ptr(dy), ptr(rstd), ptr(dx), ptr(part), T, NH, D,
            x.stride(0), dy.stride(0), dy.stride(1), dx.stride(0), _DT[x.dtype], nbytes=3 * T * NH * D * x.element_size() + T * D * 4)
    return sum_slabs(part, w.dtype) if part is not None else None


def _qk_norm_rope_fwd(x, w, cos_sin, eps):
    """One dta_qk_norm_rope_fwd launch over x [T, NH, D] (rows of D contiguous, any token stride): (y contiguous, rstd | None without w)."""
    T, NH, D = x.shape
    y = torch.empty((T, NH, D), dtype=x.dtype, device=x.device)
    rstd = torch.empty(T * NH, dtype=torch.float32, device=x.device) if w is not None else None
    _launch("dta_qk_norm_rope_fwd", (x, w, cos_sin), ptr(x), ptr(w), ptr(cos_sin), ptr(y), ptr(rstd), T, NH, D, x.stride(0), float(eps),
            _DT[x.dtype], nbytes=2 * T * NH * D * x.element_size() + T * D * 4)
    return y, rstd


def _qk_norm_rope_bwd(x, w, cos_sin, dy, rstd, dx, need_w, eps=None):
    """One dta_qk_norm_rope_bwd launch into dx [T, NH, D] (any token stride; may be dy); w None: RoPE only.  Returns dw (None unless
    w is given and need_w)."""
    T, NH, D = x.shape
    if dy.stride(2) != 1:
        dy = dy.contiguous()
    part = torch.empty(lib().dta_qk_norm_rope_bwd_blocks(T * NH), D, dtype=torch.float32, device=x.device) if w is not None and need_w else None
    _launch("dta_qk_norm_rope_bwd", (x, cos_sin, dy), ptr(x), ptr(w), ptr(cos_sin), ptr(dy), ptr(rstd) if w is not None else None,
            ptr(dx), ptr(part), T, NH, D, x.stride(0), dy.stride(0), dy.stride(1), dx.stride(0), _DT[x.dtype],
            nbytes=(3 if w is not None else 2) * T * NH * D * x.element_size() + T * D * 4)
    return sum_slabs(part, w.dtype) if part is not None else None


def _rope_partial_fwd(x, w, cos_sin, interleaved):
    """One dta_rope_partial_fwd launch over x [T, NH, D] (rows of D contiguous, any token stride), cos_sin [T, R]: (y contiguous, None).
    The form has no norm: w is None."""
    T, NH, D = x.shape
    R = cos_sin.shape[1]
    y = torch.empty((T, NH, D), dtype=x.dtype, device=x.device)
    _launch("dta_rope_partial_fwd", (x, cos_sin), ptr(x), ptr(cos_sin), ptr(y), T, NH, D, R, int(interleaved), x.stride(0), _DT[x.dtype],
            nbytes=2 * T * NH * D * x.element_size() + T * R * 4)
    return y, None


def _rope_partial_bwd(x, w, cos_sin, dy, stat, dx, need_w, interleaved):
    """One dta_rope_partial_bwd launch into dx [T, NH, D] (any token stride; may be dy).  The rotation by the negative angle needs
    neither the input nor a statistic: x, w and stat are None."""
    T, NH, D = dx.shape
    if dy.stride(2) != 1:
        dy = dy.contiguous()
    _launch("dta_rope_partial_bwd", (cos_sin, dy), ptr(cos_sin), ptr(dy), ptr(dx), T, NH, D, cos_sin.shape[1], int(interleaved),
            dy.stride(0), dy.stride(1), dx.stride(0), _DT[dx.dtype], nbytes=2 * T * NH * D * dx.element_size() + T * cos_sin.shape[1] * 4)


def _check_partial_table(x, cos_sin):
    if cos_sin.dim() != 2 or cos_sin.shape[0] != x.shape[0] or cos_sin.dtype != torch.float32 or not cos_sin.is_contiguous():
        raise ValueError(f"partial RoPE: cos_sin must be a contiguous fp32 [T, R] table for x {tuple(x.shape)}, got {cos_sin.dtype} {tuple(cos_sin.shape)}")


_HEAD_NORM = (_qk_norm_rope_fwd, _qk_norm_rope_bwd)                 # per-head norm + RoPE; w None: RoPE alone
_WIDE_NORM = (_wide_qk_norm_rope_fwd, _wide_qk_norm_rope_bwd)       # OLMo's projection-wide norm + RoPE
_PARTIAL = (_rope_partial_fwd, _rope_partial_bwd)                   # partial / interleaved RoPE: keeps nothing but the table for its backward


class _Rotate(torch.autograd.Function):
    """One member form over a single tensor x [T, NH, D] (made contiguous first): what _QKVPrep does to q and to k."""

    @staticmethod
    def forward(ctx, x, w, cos_sin, form, arg):
        _require_cuda(x, cos_sin)
        if form is _PARTIAL:
            _check_partial_table(x, cos_sin)
        if x.stride(2) != 1 or x.stride(1) != x.shape[2]:
            x = x.contiguous()
        y, stat = form[0](x, w, cos_sin, arg)
        ctx.save_for_backward(None if form is _PARTIAL else x, w, cos_sin, stat)
        ctx.form, ctx.arg = form, arg
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, cos_sin, stat = ctx.saved_tensors
        dx = torch.empty(dy.shape, dtype=dy.dtype, device=dy.device)
        return dx, ctx.form[1](x, w, cos_sin, dy, stat, dx, ctx.needs_input_grad[1], ctx.arg), None, None, None


def _fused_grad_buffer(dq, dk, dv, T, Hq, Hkv, D, dtype):
    """The fused-gradient-buffer contract: the ONE contiguous [T, Hq+2Hkv, D] buffer of `dtype` whose q | k | v head slices
    dq, dk and dv are - the layout _TreeAttention.backward writes them in, which is that of the fused projection's gradient - or None
    when they are anything else (then the caller gathers them into a fresh buffer)."""
    H3 = Hq + 2 * Hkv
    base = dv._base
    in_place = (base is not None and dq._base is base and dk._base is base and base.shape == (T, H3, D) and base.is_contiguous()
                and base.dtype == dtype and dq.shape == (T, Hq, D) and dk.shape == (T, Hkv, D) and dv.shape == (T, Hkv, D)
                and dq.stride() == dk.stride() == dv.stride() == (H3 * D, D, 1)
                and (dq.storage_offset(), dk.storage_offset(), dv.storage_offset()) == (0, Hq * D, (Hq + Hkv) * D))
    return base if in_place else None


class _QKVPrep(torch.autograd.Function):
    """Fused projection output qkv [T, Hq+2Hkv, D] -> (form(q), form(k), v).  q and k are read in place from the fused buffer (token
    stride) and v is returned as a view of it; form None (Cohere2's NoPE layers): q and k are views too, no kernel, nothing saved.
    The backward hands back ONE [T, Hq+2Hkv, D] buffer: the one _TreeAttention's backward laid the three gradients out in
    (_fused_grad_buffer), transformed in place, else a fresh one the members' backwards write into (the kernels take an output token
    stride) and dv is copied to - either way without the 200 MB concatenation that `split`'s backward would do per layer."""

    @staticmethod
    def forward(ctx, qkv, wq, wk, cos_sin, Hq, Hkv, form, arg):
        T, H3, D = qkv.shape
        ctx.geom, ctx.form, ctx.arg = (T, Hq, Hkv, D, qkv.dtype), form, arg
        xq, xk, v = qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:]
        if form is not None:
            _require_cuda(qkv, cos_sin)
        assert H3 == Hq + 2 * Hkv and qkv.is_contiguous()
        if form is None:
            return xq, xk, v
        if form is _PARTIAL:
            _check_partial_table(qkv, cos_sin)
        (q, sq), (k, sk) = form[0](xq, wq, cos_sin, arg), form[0](xk, wk, cos_sin, arg)
        ctx.save_for_backward(None if form is _PARTIAL else qkv, wq, wk, cos_sin, sq, sk)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        T, Hq, Hkv, D, dtype = ctx.geom
        fused = _fused_grad_buffer(dq, dk, dv, T, Hq, Hkv, D, dtype)
        d = fused if fused is not None else torch.empty((T, Hq + 2 * Hkv, D), dtype=dtype, device=dv.device)
        dwq = dwk = None
        if ctx.form is not None:
            qkv, wq, wk, cos_sin, sq, sk = ctx.saved_tensors
            xq, xk = (qkv[:, :Hq], qkv[:, Hq:Hq + Hkv]) if qkv is not None else (None, None)
            dwq = ctx.form[1](xq, wq, cos_sin, dq, sq, d[:, :Hq], ctx.needs_input_grad[1], ctx.arg)
            dwk = ctx.form[1](xk, wk, cos_sin, dk, sk, d[:, Hq:Hq + Hkv], ctx.needs_input_grad[2], ctx.arg)
        elif fused is None:
            d[:, :Hq].copy_(dq); d[:, Hq:Hq + Hkv].copy_(dk)
        if fused is None:
            d[:, Hq + Hkv:].copy_(dv)
        return d, dwq, dwk, None, None, None, None, None


def qkv_prep(qkv: torch.Tensor, wq: Optional[torch.Tensor], wk: Optional[torch.Tensor], cos_sin: torch.Tensor, eps: float,
             Hq: int, Hkv: int):
    """(q, k, v) for `tree_attention` from the fused projection output [T, Hq+2Hkv, D]."""
    return _QKVPrep.apply(qkv, wq, wk, cos_sin, Hq, Hkv, _HEAD_NORM, eps)


def qkv_prep_wide(qkv: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, cos_sin: torch.Tensor, eps: float, Hq: int, Hkv: int):
    """qkv_prep with the projection-wide norms of OLMo-2 / OLMo-3: wq [Hq*D] and wk [Hkv*D] normalise the whole q / k row of a token
    before the heads are rotated (dta_wide_qk_norm_rope_*).  q and k are read in place, v is a view, the three gradients land in one
    [T, Hq+2Hkv, D] buffer and a frozen weight gets no partials - as qkv_prep."""
    assert wq is not None and wk is not None
    return _QKVPrep.apply(qkv, wq, wk, cos_sin, Hq, Hkv, _WIDE_NORM, eps)


def qkv_prep_partial(qkv: torch.Tensor, cos_sin: torch.Tensor, Hq: int, Hkv: int, interleaved: bool):
    """(q, k, v) for `tree_attention` from the fused projection output [T, Hq+2Hkv, D] of a model without q/k norms whose RoPE covers
    the first R = cos_sin.shape[1] elements of the head (rope_partial)."""
    return _QKVPrep.apply(qkv, None, None, cos_sin, Hq, Hkv, _PARTIAL, bool(interleaved))


def qkv_prep_nope(qkv: torch.Tensor, Hq: int, Hkv: int):
    """(q, k, v) for `tree_attention` from the fused projection output [T, Hq+2Hkv, D] of a layer that applies no RoPE (Cohere2's
    full-attention layers): strided views - the projection's values bit for bit - no kernel."""
    return _QKVPrep.apply(qkv, None, None, None, Hq, Hkv, None, None)


def rope_partial(x: torch.Tensor, cos_sin: torch.Tensor, interleaved: bool) -> torch.Tensor:
    """x [T, NH, D] (D = 64 or 128) -> RoPE over the first R = cos_sin.shape[1] elements of every head at the positions encoded in
    cos_sin [T, R] (fp32, rope_cos_sin with R as its D); elements R.. pass through.  interleaved False: the half-split pairing
    i <-> i + R/2 (Phi-3, R % 16 == 0); True: the pairs (2i, 2i+1) (GLM-4, R % 8 == 0)."""
    return _Rotate.apply(x, None, cos_sin, _PARTIAL, bool(interleaved))


def qk_norm_rope(x: torch.Tensor, w: Optional[torch.Tensor], cos_sin: torch.Tensor, eps: float) -> torch.Tensor:
    """x [T, NH, D] (D = 64 or 128) -> RoPE(RMSNorm_D(x) * w) at the positions encoded in cos_sin [T,D] (fp32)."""
    return _Rotate.apply(x, w, cos_sin, _HEAD_NORM, eps)


ROPE_TYPES = ("default", "linear", "llama3", "yarn")


def rope_inv_freq(D: int, rope_parameters: dict, max_position_embeddings: Optional[int] = None):
    """(inv_freq [D/2] fp32 on the host, attention_factor) of a RoPE parameter dict (`rope_type` default / linear / llama3 / yarn,
    `rope_theta` and the type's own fields - the dict transformers keeps in config.rope_parameters).  The formulas are those of
    transformers' modeling_rope_utils (_compute_linear_scaling_rope_parameters, _compute_llama3_parameters, _compute_yarn_parameters)
    restated with the same fp32 host operations in the same order, so that the frequencies come out bit for bit (see rope_cos_sin for
    what one ulp costs).  `max_position_embeddings` stands in for an absent `original_max_position_embeddings` and for YaRN's absent
    `factor`, as there."""
    rp = rope_parameters
    kind = rp.get("rope_type", rp.get("type")) or "default"
    if kind not in ROPE_TYPES:
        raise ValueError(f"rope_parameters: rope_type {kind!r} is not supported ({' / '.join(ROPE_TYPES)})")
    base = float(rp["rope_theta"])
    steps = torch.arange(0, D, 2, dtype=torch.int64).to(torch.float32)
    if kind == "default":
        return 1.0 / (base ** (steps / D)), 1.0
    if kind == "linear":
        inv = 1.0 / (base ** (steps / D))
        inv /= rp["factor"]
        return inv, 1.0
    orig = rp.get("original_max_position_embeddings") or max_position_embeddings
    if orig is None:
        raise ValueError(f"rope_parameters: rope_type {kind!r} needs original_max_position_embeddings (or max_position_embeddings)")
    if kind == "llama3":
        inv = 1.0 / (base ** (steps / D))
        factor, low_f, high_f = rp["factor"], rp["low_freq_factor"], rp["high_freq_factor"]
        low_wavelen, high_wavelen = orig / low_f, orig / high_f
        wavelen = 2 * math.pi / inv
        scaled = torch.where(wavelen > low_wavelen, inv / factor, inv)          # long wavelengths: divided by factor; short ones: kept
        smooth = (orig / wavelen - low_f) / (high_f - low_f)                    # the band between: interpolated
        smoothed = (1 - smooth) * scaled / factor + smooth * scaled
        medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
        return torch.where(medium, smoothed, scaled), 1.0
    # yarn
    factor = rp.get("factor")
    if factor is None:
        if max_position_embeddings is None:
            raise ValueError("rope_parameters: yarn needs factor (or max_position_embeddings)")
        factor = max_position_embeddings / orig
    mscale_of = lambda scale, m=1: 1.0 if scale <= 1 else 0.1 * m * math.log(scale) + 1.0
    att = rp.get("attention_factor")
    if att is None:
        ms, ms_all = rp.get("mscale"), rp.get("mscale_all_dim")
        att = float(mscale_of(factor, ms) / mscale_of(factor, ms_all)) if ms and ms_all else mscale_of(factor)
    beta_fast, beta_slow = rp.get("beta_fast") or 32, rp.get("beta_slow") or 1
    corr_dim = lambda rot: (D * math.log(orig / (rot * 2 * math.pi))) / (2 * math.log(base))
    low, high = corr_dim(beta_fast), corr_dim(beta_slow)
    if rp.get("truncate", True):
        low, high = math.floor(low), math.ceil(high)
    low, high = max(low, 0), min(high, D - 1)
    if low == high:
        high += 0.001
    pos_freqs = base ** (steps / D)
    extrapolation, interpolation = 1.0 / pos_freqs, 1.0 / (factor * pos_freqs)
    keep = 1 - torch.clamp((torch.arange(D // 2, dtype=torch.float32) - low) / (high - low), 0, 1)
    return interpolation * (1 - keep) + extrapolation * keep, att


def longrope_inv_freq(R: int, rope_parameters: dict, max_position_embeddings: Optional[int], long: bool):
    """(inv_freq [R/2] fp32 on the host, attention_factor) of a `longrope` parameter dict (Phi-3 / Phi-4-mini) over the rotary dimension
    R, with the `long_factor` (long) or the `short_factor` list: transformers' _compute_longrope_parameters restated with the same fp32
    host operations in the same order - 1 / (ext_factors * base ** (arange(0, R, 2) / R)) - so that the frequencies come out bit for bit.
    Which set a call uses is the caller's decision (HF: long when the sequence is longer than original_max_position_embeddings).
    factor defaults to max_position_embeddings / original_max_position_embeddings; without an explicit attention_factor the table is
    scaled by sqrt(1 + ln(factor) / ln(original_max_position_embeddings)) when factor > 1."""
    rp = rope_parameters
    orig = rp.get("original_max_position_embeddings")
    if orig is None:
        raise ValueError("rope_parameters: longrope needs original_max_position_embeddings")
    name = "long_factor" if long else "short_factor"
    ext = rp.get(name)
    if ext is None or len(ext) != R // 2:
        raise ValueError(f"rope_parameters: longrope needs {name} with {R // 2} entries (rotary dimension {R}), got "
                         f"{'none' if ext is None else len(ext)}")
    factor = rp.get("factor")
    if factor is None:
        if max_position_embeddings is None:
            raise ValueError("rope_parameters: longrope needs factor (or max_position_embeddings)")
        factor = max_position_embeddings / orig
    att = rp.get("attention_factor")
    if att is None:
        att = 1.0 if factor <= 1.0 else math.sqrt(1 + math.log(factor) / math.log(orig))
    base = rp["rope_theta"]
    shape = torch.arange(0, R, 2, dtype=torch.int64).float() / R
    return 1.0 / (torch.tensor(ext, dtype=torch.float32) * base ** shape), att


_INV_FREQ: dict = {}


def rope_cos_sin(depth: torch.Tensor, D: int, rope) -> torch.Tensor:
    """fp32 [T, D] table {cos[D/2], sin[D/2]} * attention_factor of position = trie depth (computed once per trie).  `rope` is the
    resolved pair (inv_freq [D/2] fp32 on the host, attention_factor) of rope_inv_freq, or a plain theta for the default
    frequencies.  The inverse frequencies are computed ON
    THE HOST in fp32, exactly as transformers' rotary-embedding init does (`1 / base ** (arange(0, D, 2) / D)`): the GPU's `pow` differs
    from the host's in the last bit, and one ulp of an inverse frequency is 1e-7 x position radians of phase - 5e-5 rad at depth 512,
    1.6e-3 at 16 384 - which the fp32 engine showed as a 6e-4 deviation of gradient norms from the reference at Qwen3-0.6B size.
    The device copy is cached by the frequencies' VALUE (two configurations with one theta and different scaling do not share it)."""
    if isinstance(rope, (int, float)):
        key, host, factor = (D, float(rope), depth.device), None, 1.0
    else:
        host, factor = rope
        if host.shape != (D // 2,) or host.dtype != torch.float32 or host.device.type != "cpu":
            raise ValueError(f"rope_cos_sin: inv_freq must be a host fp32 [{D // 2}] tensor, got {host.dtype} {tuple(host.shape)} on {host.device}")
        key = (D, host.numpy().tobytes(), depth.device)
    inv = _INV_FREQ.get(key)
    if inv is None:
        if host is None:
            host = rope_inv_freq(D, {"rope_theta": float(rope)})[0]
        inv = host.to(depth.device)
        _INV_FREQ[key] = inv
    ang = depth.float()[:, None] * inv[None, :]
    table = torch.cat([ang.cos(), ang.sin()], dim=-1)
    if float(factor) != 1.0:
        table = table * float(factor)
    return table.contiguous()


class _SwiGLU(torch.autograd.Function):
    """y = silu(gate) * up.  `gu` is either the fused [rows, 2C] projection output (gate | up) or None with
    separate contiguous gate/up.  `kernel`: "dta_swiglu", or "dta_geglu" for y = gelu_tanh(gate) * up (same layouts)."""

    @staticmethod
    def forward(ctx, gu, g, u, kernel="dta_swiglu"):
        ctx.kernel = kernel
        if gu is not None:
            _require_cuda(gu)
            gu = gu if gu.stride(-1) == 1 and gu.dim() == 2 else gu.contiguous().view(-1, gu.shape[-1])
            C = gu.shape[1] // 2
            g, u, ld = gu[:, :C], gu[:, C:], gu.stride(0)
        else:
            _require_cuda(g, u)
            g = g.contiguous().view(-1, g.shape[-1]); u = u.contiguous().view(-1, u.shape[-1])
            C, ld = g.shape[1], g.shape[1]
        rows = g.shape[0]
        y = torch.empty((rows, C), dtype=g.dtype, device=g.device)
        _launch(ctx.kernel + "_fwd", (g, u), ptr(g), ptr(u), ptr(y), rows, C, ld, _DT[g.dtype], nbytes=3 * rows * C * g.element_size())
        ctx.save_for_backward(g, u)
        ctx.fused, ctx.ld = gu is not None, ld
        return y

    @staticmethod
    def backward(ctx, dy):
        g, u = ctx.saved_tensors
        rows, C = g.shape
        dy = dy.contiguous()
        if ctx.fused:
            dgu = torch.empty((rows, 2 * C), dtype=g.dtype, device=g.device)
            dg, du, ldg = dgu[:, :C], dgu[:, C:], 2 * C
        else:
            dg, du, ldg = torch.empty_like(g), torch.empty_like(u), C
        _launch(ctx.kernel + "_bwd", (g, u, dy), ptr(g), ptr(u), ptr(dy), ptr(dg), ptr(du), rows, C, ctx.ld, ldg, _DT[g.dtype],
                nbytes=5 * rows * C * g.element_size())
        return (dgu, None, None, None) if ctx.fused else (None, dg, du, None)


def swiglu(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    return _SwiGLU.apply(None, g, u, "dta_swiglu")


def swiglu_fused(gu: torch.Tensor) -> torch.Tensor:
    """gu [rows, 2C] = (gate | up) of one fused projection GEMM -> silu(gate) * up  [rows, C]."""
    return _SwiGLU.apply(gu, None, None, "dta_swiglu")


def geglu(g: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """gelu_tanh(g) * u (HF's gelu_pytorch_tanh; Gemma) on the dta_geglu kernels; the layouts of swiglu."""
    return _SwiGLU.apply(None, g, u, "dta_geglu")


def geglu_fused(gu: torch.Tensor) -> torch.Tensor:
    """gu [rows, 2C] = (gate | up) of one fused projection GEMM -> gelu_tanh(gate) * up  [rows, C]."""
    return _SwiGLU.apply(gu, None, None, "dta_geglu")


class weight_cache:
    """Scope in which per-weight copies (stacked projection rows, transposed weights) are shared: ONE engine call (`forward`, `backward`,
    a dense pass).  Inside it every layer call, the recomputation pass and every block of the block-wise walk reuse one copy per weight;
    when the outermost scope ends the copies are dropped - the optimizer step that follows changes the weights anyway, and nothing is keyed
    across calls on identifiers a later tensor could recycle (object ids, storage addresses, version counters: a cache that outlived the
    call once served another model's layer to a new one in the test suite).  Outside any scope nothing is cached."""
    depth = 0

    def __enter__(self):
        weight_cache.depth += 1
        return self

    def __exit__(self, *exc):
        weight_cache.depth -= 1
        if weight_cache.depth == 0:
            clear_weight_caches()
        return False


class _StackRows(torch.autograd.Function):
    """Concatenate weight matrices along dim 0 into one GEMM operand.  Backward hands each input its row
    slice of the fused gradient as a VIEW (no copy); forward is len(ws) plain copies (torch.cat's batched
    copy kernel took 170 us for two 6 MB inputs on gfx950) - and none at all when the same weights were stacked before
    INSIDE THE SAME `weight_cache` SCOPE (one engine call): every layer call of a step, the recomputation pass and every block
    of the block-wise walk share ONE fused copy."""

    CACHE_BYTES = 8 << 30            # fused copies kept at most (Qwen3-0.6B: 0.59 GB, Qwen3-4B: 4.7 GB); beyond it, copy per call
    _cache: dict = {}
    _cached_bytes = 0

    @staticmethod
    def _fused(ws):
        rows = [w.shape[0] for w in ws]
        key = tuple((id(w), w.data_ptr(), w._version) for w in ws)
        if weight_cache.depth > 0:
            hit = _StackRows._cache.get(key)
            if hit is not None:
                return hit
        out = torch.empty((sum(rows),) + tuple(ws[0].shape[1:]), dtype=ws[0].dtype, device=ws[0].device)
        o = 0
        for w, r in zip(ws, rows):
            out[o:o + r].copy_(w); o += r
        nbytes = out.numel() * out.element_size()
        if weight_cache.depth > 0 and _StackRows._cached_bytes + nbytes <= _StackRows.CACHE_BYTES:
            _StackRows._cache[key] = out; _StackRows._cached_bytes += nbytes
        return out

    @staticmethod
    def forward(ctx, *ws):
        ctx.rows = [w.shape[0] for w in ws]
        return _StackRows._fused(ws).detach()           # a fresh alias: autograd attaches this call's node to it, not to the cached buffer

    @staticmethod
    def backward(ctx, g):
        outs, o = [], 0
        for r in ctx.rows:
            outs.append(g[o:o + r]); o += r
        return tuple(outs)


def stack_rows(*ws: torch.Tensor) -> torch.Tensor:
    return _StackRows.apply(*ws)


def clear_stack_rows_cache() -> None:
    _StackRows._cache.clear(); _StackRows._cached_bytes = 0


def sum_slabs(part: torch.Tensor, out_dtype: torch.dtype, extra: torch.Tensor = None) -> torch.Tensor:
    """part [S, ...] fp32 -> (Σ_s part[s] + extra) rounded once to `out_dtype`, ONE launch (torch: sum, add, cast = three, and its
    column sum of a [2048, 1024] partial runs at 0.45 TB/s)."""
    assert part.dtype == torch.float32 and part.is_contiguous() and (extra is None or (extra.dtype == torch.float32 and extra.is_contiguous()))
    S, n = part.shape[0], part[0].numel()
    assert extra is None or extra.numel() == n
    out = torch.empty(part.shape[1:], dtype=out_dtype, device=part.device)
    _launch("dta_sum_slabs", (part, extra, out), ptr(part), S, n, n, ptr(extra), ptr(out), _DT[out_dtype], nbytes=(S + (extra is not None)) * n * 4)
    return out


def transpose_2d(w: torch.Tensor) -> torch.Tensor:
    """[R, C] -> contiguous [C, R] by the HIP transpose kernel (16-byte accesses both ways; torch's transposing copy of a 311 MB head
    weight takes 2.5 ms, an HBM-rate copy 0.2)."""
    R, C = w.shape
    if w.stride(1) != 1:
        w = w.contiguous()
    out = torch.empty((C, R), dtype=w.dtype, device=w.device)
    _launch("dta_transpose", (w, out), ptr(w), ptr(out), R, C, w.stride(0), R, w.element_size(), nbytes=2 * R * C * w.element_size())
    return out


class _TransposedWeights:
    """Transposed copies of weight matrices, one per weight inside a `weight_cache` scope (one engine call): shared by every use of the weight
    in that call (recomputation passes, blocks of the block-wise walk).  Same 8 GB bound as the stacked-rows cache; beyond it, and outside a
    scope, the copy is made per use."""
    cache: dict = {}
    nbytes = 0

    @staticmethod
    def get(w: torch.Tensor) -> torch.Tensor:
        if weight_cache.depth == 0:
            return transpose_2d(w)
        # strides too: two views of one storage (a column slice of a fused buffer, a contiguous matrix at the same address) share the
        # pointer, the shape and the version counter and are different matrices
        key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()), w.dtype, w._version)
        hit = _TransposedWeights.cache.get(key)
        if hit is not None:
            return hit
        wt = transpose_2d(w)
        n = wt.numel() * wt.element_size()
        if _TransposedWeights.nbytes + n <= _StackRows.CACHE_BYTES:
            _TransposedWeights.cache[key] = wt; _TransposedWeights.nbytes += n
        return wt


def clear_weight_caches() -> None:
    """Drop the per-call copies of the weights (stacked projection rows, transposed copies); `weight_cache.__exit__` calls this."""
    clear_stack_rows_cache()
    _TransposedWeights.cache.clear(); _TransposedWeights.nbytes = 0


def _dgrad(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dx[T, in] = dy[T, out] · W[out, in].  With W row-major the contraction index strides by `in`; against a transposed copy (contraction
    index contiguous in both operands) hipBLASLt runs the same product 12-25 % faster on gfx950 (scripts/gemm_dgrad_layout_probe.py:
    q/k/v 0.252 -> 0.202 ms, gate/up 0.322 -> 0.275, down 0.183 -> 0.155, LM head 9.68 -> 8.34 at T = 28 160) - the copy (HIP transpose,
    once per weight version) costs a tenth of that."""
    if _dgrad_transposed(dy, w.shape, w.dtype):
        return dy @ _TransposedWeights.get(w).t()
    return dy @ w


def _dgrad_transposed(dy: torch.Tensor, w_shape, w_dtype) -> bool:
    """Whether `_dgrad` runs dy · W against a transposed copy of W [out, in] (from 4096 rows on) or against W as it is."""
    return dy.is_cuda and w_dtype in (torch.bfloat16, torch.float16) and dy.shape[0] >= 4096 and w_shape[0] % 8 == 0 and w_shape[1] % 8 == 0


WGRAD_SPLIT_K = 4      # slices of the packed rows in the weight-gradient GEMM of a small projection


def _wgrad(x: torch.Tensor, dy: torch.Tensor, transposed: bool) -> torch.Tensor:
    """dW[out, in] = dyᵀ[out, T] · x[T, in] - few output tiles, long K.  Qwen3-0.6B's q/k/v, o and down projections give 32-64 tiles of
    256x256 for 256 CUs with K = T ≈ 28 k: hipBLASLt runs them at 580-720 TFLOP/s.  A manual split-K fills the chip: the T rows are cut
    into `WGRAD_SPLIT_K` equal slices (multiples of 64 rows), ONE batched GEMM forms the slices' products with fp32 outputs, and they
    are summed in fp32 and rounded once by `sum_slabs` (closer to the exact product than the single bf16-output GEMM) - 0.344 -> 0.260 ms (q/k/v),
    0.203 -> 0.147 (o), 0.248 -> 0.201 (down) at T = 28 160 (scripts/gemm_splitk_probe.py; gate/up with 96 tiles does not gain and
    larger geometries have enough tiles).  `transposed`: form xᵀ·dy and return its transpose view (_Linear's layout choice)."""
    T = x.shape[0]
    a, b = (x, dy) if transposed else (dy, x)                    # result = aᵀ · b
    S = WGRAD_SPLIT_K
    tiles = -(-a.shape[1] // 256) * -(-b.shape[1] // 256)
    per = (T // S) // 64 * 64      # packed lengths are multiples of 256 from 2 048 rows on: nothing is left over at S = 4
    if tiles > 64 or per < 2048 or not x.is_cuda or x.dtype == torch.float32:
        out = a.t() @ b
    else:
        body = per * S
        part = torch.bmm(a[:body].reshape(S, per, a.shape[1]).transpose(1, 2), b[:body].reshape(S, per, b.shape[1]), out_dtype=torch.float32)
        rest = torch.mm(a[body:].t(), b[body:], out_dtype=torch.float32) if body < T else None
        out = sum_slabs(part, x.dtype, rest)
    if not transposed:
        return out
    # a contiguous [out, in]: autograd keeps it as the parameter's gradient as it is (a transposed VIEW is cloned by a strided copy that
    # takes 13-18 us for a 4-6 MB matrix; this kernel 7)
    V = 16 // out.element_size()
    return transpose_2d(out) if out.is_cuda and out.shape[0] % V == 0 and out.shape[1] % V == 0 else out.t()


class _Linear(torch.autograd.Function):
    """y = x Wᵀ (+ b) over packed rows with the weight-gradient GEMM issued in the layout hipBLASLt runs faster on
    gfx950: for a projection that narrows by 2x or more (Qwen3-0.6B o_proj 2048->1024, down_proj 3072->1024) `xᵀ·dy`
    (then viewed transposed) is 1.2-1.5× faster than autograd's `dyᵀ·x`; for the widening ones and for mild narrowing
    (Qwen3-4B o_proj 4096->2560) it is the other way round (scripts/gemm_wgrad_variants.py, both geometries)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = _dgrad(dy, w) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = _wgrad(x, dy, w.shape[1] >= 2 * w.shape[0])
        db = dy.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db


def linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [rows, in] @ w[out, in]ᵀ."""
    return _Linear.apply(x, w, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# Mixture of experts (Qwen3MoeSparseMoeBlock): router top-k, permutation by expert, grouped GEMMs, combine - include/dta.h "Mixture of experts"
# ------------------------------------------------------------------------------------------------------------------------------------
MOE_FWD, MOE_DGRAD, MOE_WGRAD = 0, 1, 2


@dataclass
class MoeRouting:
    """Device-side result of the permutation of one layer's T*k (token, slot) pairs: expert_offsets [E+1], row_of_pair [T*k],
    src_token [T*k] (row -> token), tiles [2 * bound] (the grouped GEMMs' tile table).  Nothing of it is read on the host."""
    T: int
    k: int
    E: int
    expert_offsets: torch.Tensor
    row_of_pair: torch.Tensor
    src_token: torch.Tensor
    tiles: torch.Tensor


def moe_router_fwd_raw(logits: torch.Tensor, k: int, norm: bool):
    """logits [T, E] -> (ids int32 [T, k], weights [T, k] in the logits' dtype, lse float [T])."""
    T, E_ = logits.shape
    logits = logits.contiguous()
    ids = torch.empty((T, k), dtype=torch.int32, device=logits.device)
    w = torch.empty((T, k), dtype=logits.dtype, device=logits.device)
    lse = torch.empty(T, dtype=torch.float32, device=logits.device)
    _launch("dta_moe_router_fwd", (logits,), ptr(logits), ptr(ids), ptr(w), ptr(lse), T, E_, k, int(bool(norm)), _DT[logits.dtype],
            nbytes=T * E_ * logits.element_size())
    return ids, w, lse


def moe_router_bwd_raw(logits, lse, ids, dw, norm: bool):
    T, E_ = logits.shape
    dw = dw.contiguous().to(logits.dtype)
    dl = torch.empty_like(logits)
    _launch("dta_moe_router_bwd", (logits, dw), ptr(logits), ptr(lse), ptr(ids), ptr(dw), ptr(dl), T, E_, ids.shape[1], int(bool(norm)),
            _DT[logits.dtype], nbytes=2 * T * E_ * logits.element_size())
    return dl


def moe_permute(ids: torch.Tensor, E_: int) -> MoeRouting:
    """Counting sort of the (token, slot) pairs of ids [T, k] (int32) by expert: rows of an expert in token order, bitwise the same on
    every call (the layer recomputation re-routes in the backward)."""
    T, k = ids.shape
    P = T * k
    L = lib()
    dev = ids.device
    ws = torch.empty(max(int(L.dta_moe_permute_workspace(P, E_)), 1), dtype=torch.int32, device=dev)
    bound = int(L.dta_moe_tile_bound(P, E_))
    offs = torch.empty(E_ + 1, dtype=torch.int32, device=dev)
    rop = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    src = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    tiles = torch.empty(2 * bound, dtype=torch.int32, device=dev)
    ids = ids.contiguous()
    _launch("dta_moe_permute", (ids,), ptr(ids), T, k, E_, ptr(ws), ptr(offs), ptr(rop), ptr(src), ptr(tiles), nbytes=12 * P)
    return MoeRouting(T, k, E_, offs, rop[:P], src[:P], tiles)


def moe_grouped_gemm(mode: int, route: MoeRouting, w_shape, out_dtype, x=None, w=None, dy=None, gather: bool = False) -> torch.Tensor:
    """One grouped GEMM over the expert-sorted rows (dta_moe_grouped_gemm); w_shape = (E, N, K) of the expert weights."""
    E_, N, K = w_shape
    R = route.T * route.k
    ref = x if x is not None else dy
    shape = (R, N) if mode == MOE_FWD else (R, K) if mode == MOE_DGRAD else (E_, N, K)
    out = torch.empty(shape, dtype=out_dtype, device=ref.device)
    if R == 0:          # no rows: nothing to launch (an empty tensor has no address to hand over); the weight gradient of no rows is zero
        return out.zero_() if mode == MOE_WGRAD else out
    x, w, dy = (None if t is None else t.contiguous() for t in (x, w, dy))
    esz = out.element_size()
    _launch("dta_moe_grouped_gemm", tuple(t for t in (x, w, dy) if t is not None), mode, ptr(x), ptr(w), ptr(dy), ptr(out),
            ptr(route.src_token) if gather else None, ptr(route.expert_offsets), ptr(route.tiles), R, E_, N, K, _DT[out_dtype],
            nbytes=esz * (R * N + R * K + E_ * N * K), span=f"moe_gemm_{('fwd', 'dgrad', 'wgrad')[mode]}_{N}x{K}")
    return out


def moe_combine_fwd_raw(y, w, route: MoeRouting):
    """out[t] = Σ_j w[t, j] · y[row(t, j)] (w None: weight 1)."""
    H = y.shape[1]
    out = torch.empty((route.T, H), dtype=y.dtype, device=y.device)
    _launch("dta_moe_combine_fwd", (y,), ptr(y), ptr(w), ptr(route.row_of_pair), ptr(out), route.T, route.k, H, _DT[y.dtype],
            nbytes=(route.k + 1) * route.T * H * y.element_size())
    return out


def moe_combine_bwd_raw(dout, y, w, route: MoeRouting):
    H = y.shape[1]
    dout = dout.contiguous()
    dy = torch.empty_like(y)
    dw = torch.empty_like(w)
    _launch("dta_moe_combine_bwd", (dout, y, w), ptr(dout), ptr(y), ptr(w), ptr(route.row_of_pair), ptr(dy), ptr(dw), route.T, route.k, H,
            _DT[y.dtype], nbytes=(3 * route.k + 1) * route.T * H * y.element_size())
    return dy, dw


class _MoeRouter(torch.autograd.Function):
    """logits [T, E] -> top-k weights [T, k] (differentiable) and ids (not)."""

    @staticmethod
    def forward(ctx, logits, k, norm):
        ids, w, lse = moe_router_fwd_raw(logits, k, norm)
        ctx.save_for_backward(logits, lse, ids)
        ctx.norm = norm
        ctx.mark_non_differentiable(ids)
        return w, ids

    @staticmethod
    def backward(ctx, dw, _dids):
        logits, lse, ids = ctx.saved_tensors
        return moe_router_bwd_raw(logits, lse, ids, dw, ctx.norm), None, None


class _MoeLinear(torch.autograd.Function):
    """y [T*k, N] = per-expert x · W_eᵀ over the expert-sorted rows; `gather`: x is [T, K] token rows read through src_token (the MoE
    block's input), else x is already expert-sorted [T*k, K].  Backward: dgrad (and, for a gathered x, the fixed-order scatter-back onto
    tokens) and wgrad as grouped GEMMs - no transposed copy of the expert weights."""

    @staticmethod
    def forward(ctx, x, w, route, gather):
        ctx.save_for_backward(x, w)
        ctx.route, ctx.gather = route, gather
        return moe_grouped_gemm(MOE_FWD, route, w.shape, x.dtype, x=x, w=w, gather=gather)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        route, gather = ctx.route, ctx.gather
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dxs = moe_grouped_gemm(MOE_DGRAD, route, w.shape, x.dtype, w=w, dy=dy)
            dx = moe_combine_fwd_raw(dxs, None, route) if gather else dxs
        if ctx.needs_input_grad[1]:
            dw = moe_grouped_gemm(MOE_WGRAD, route, w.shape, w.dtype, x=x, dy=dy, gather=gather)
        return dx, dw, None, None


class _MoeCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, w, route):
        ctx.save_for_backward(y, w)
        ctx.route = route
        return moe_combine_fwd_raw(y, w, route)

    @staticmethod
    def backward(ctx, dout):
        y, w = ctx.saved_tensors
        dy, dw = moe_combine_bwd_raw(dout, y, w, ctx.route)
        return dy, dw, None


def moe_mlp(h: torch.Tensor, router_w: torch.Tensor, gate_up_w: torch.Tensor, down_w: torch.Tensor, top_k: int,
            norm_topk_prob: bool) -> torch.Tensor:
    """Qwen3MoeSparseMoeBlock over packed rows h [T, H]: router GEMM (ops.linear), top-k routing, expert-sorted grouped GEMMs
    gate_up_proj [E, 2I, H] -> SwiGLU (swiglu_fused: HF's (gate | up) row halves) -> down_proj [E, H, I], weighted combine.
    No router auxiliary loss (HF adds it only with output_router_logits)."""
    if not h.is_cuda:
        raise RuntimeError("moe_mlp runs on the MI355X only; there is no CPU path")
    E_ = gate_up_w.shape[0]
    logits = linear(h, router_w)
    w, ids = _MoeRouter.apply(logits, int(top_k), bool(norm_topk_prob))
    route = moe_permute(ids, E_)
    gu = _MoeLinear.apply(h, gate_up_w, route, True)
    act = swiglu_fused(gu)
    y = _MoeLinear.apply(act, down_w, route, False)
    return _MoeCombine.apply(y, w, route)


# ------------------------------------------------------------------------------------------------------------------------------------
# Low-rank adapters (LoRA): y = base(x) + scaling (x Aᵀ) Bᵀ with the base weight frozen - include/dta.h "Low-rank adapters", lora.py
# ------------------------------------------------------------------------------------------------------------------------------------
def _host_f32(vals):
    return None if vals is None else np.ascontiguousarray(vals, np.float32)


def lora_down(x: torch.Tensor, m: torch.Tensor, rscale=None) -> torch.Tensor:
    """out[T, R] = (x[T, K] · m[R, K]ᵀ) * rscale[r] (dta_lora_down): one read of x.  rscale: R host floats or None."""
    T, K = x.shape
    R = m.shape[0]
    assert x.stride(1) == 1 and m.stride(1) == 1 and m.shape[1] == K and m.dtype == x.dtype
    out = torch.empty((T, R), dtype=x.dtype, device=x.device)
    rs = _host_f32(rscale)
    _launch("dta_lora_down", (x, m), ptr(x), x.stride(0), ptr(m), m.stride(0), ptr(out), R, None if rs is None else rs.ctypes.data,
            T, R, K, _DT[x.dtype], nbytes=(T * K + R * K + T * R) * x.element_size())
    return out


def lora_wgrad(l: torch.Tensor, x: torch.Tensor, out_dtype: torch.dtype, rscale=None) -> torch.Tensor:
    """G[R, K] = rscale[r] * Σ_t l[t, R]ᵀ x[t, K] (dta_lora_wgrad: fp32 partials per slab of rows, then sum_slabs in slab order, rounded
    once to `out_dtype`; fp32: the unrounded sum).  One read of x and l."""
    T, K = x.shape
    R = l.shape[1]
    assert l.shape[0] == T and l.stride(1) == 1 and x.stride(1) == 1 and l.dtype == x.dtype
    S = int(lib().dta_lora_wgrad_slabs(T, K))
    part = torch.empty((S, R, K), dtype=torch.float32, device=x.device)
    rs = _host_f32(rscale)
    _launch("dta_lora_wgrad", (l, x), ptr(l), l.stride(0), ptr(x), x.stride(0), ptr(part), None if rs is None else rs.ctypes.data,
            T, R, K, _DT[x.dtype], nbytes=(T * K + T * R) * x.element_size() + S * R * K * 4)
    return part[0] if (S == 1 and out_dtype == torch.float32) else sum_slabs(part, out_dtype)


# Which form runs each low-rank product: scripts/lora_probe.py on one MI355X (profiles/lora_probe.json: T = 28 160, bf16, the kernel against
# the torch / hipBLASLt expression it replaces, alternating in one process).  A kernel is the default where it was at least as fast:
#   Lᵀ·X          dta_lora_wgrad: faster than dxaᵀ·x and than the manual split-K form up to K = 12 288 (level at 4096), slower at 24 576
#                 -> the kernel for K <= WGRAD_KERNEL_MAX_K, one fp32-output GEMM beyond
#   x·Aᵀ / dy·B   dta_lora_down: faster only at K = 1024 with a rank class of 32; slower at every larger K -> the kernel there only
#   y += s·xa·Bᵀ  an in-place MFMA kernel (scripts/diag/lora_up_add_experiment.hip) lost to addmm_ at every shape: the product ships addmm_
WGRAD_KERNEL_MAX_K = 12288


def _down_by_kernel(K: int, R: int) -> bool:
    return K <= 1024 and R <= 32


def _wgrad_by_kernel(K: int) -> bool:
    return K <= WGRAD_KERNEL_MAX_K


def _lora_wgrad(l: torch.Tensor, x: torch.Tensor, out_dtype: torch.dtype, seg_scale=None) -> torch.Tensor:
    """G[R, K] = Lᵀ·X over the packed rows, rows r0 .. r0+r of every (r0, r, scale) in seg_scale multiplied by scale.  Either form keeps the
    sum in fp32 until ONE rounding to `out_dtype` (none for fp32 adapters) and scales the fp32 sum: the HIP kernel (fp32 slabs, summed in
    slab order), or beyond WGRAD_KERNEL_MAX_K one GEMM with an fp32 result.  The fp32 workspace is S·Σr·K·4 bytes (kernel, S <= 64 slabs)
    or Σr·K·4 (GEMM) per call - for a fused gate|up output of 24 576 columns and Σr = 32 that is 3 MB."""
    K = x.shape[1]
    if _wgrad_by_kernel(K):
        rs = None
        if seg_scale is not None:
            rs = np.ones(l.shape[1], np.float32)
            for r0, r, sc in seg_scale:
                rs[r0:r0 + r] = sc
        return lora_wgrad(l, x, out_dtype, rs)
    g = torch.mm(l.t(), x, out_dtype=torch.float32)
    for r0, r, sc in seg_scale or ():
        if sc != 1.0:
            g[r0:r0 + r] *= sc
    return g if out_dtype == torch.float32 else g.to(out_dtype)


class _LoraLinear(torch.autograd.Function):
    """y = x Wᵀ (+ b) + Σ_seg scaling_seg · (x A_segᵀ) B_segᵀ on the segment's columns of y: ONE base GEMM over the (stacked) base weight
    of a fused projection group and the adapters of its members.  `spec`: per adapter (n0, nlen, r, scaling) - the column range of the
    member in the fused output - and `ab` = (A_0, B_0, A_1, B_1, ...).  The adapters share the input, so their A matrices are stacked:
    xa = x·A_catᵀ is one pass over x.  In the backward dy is read once for dxa (each adapter its own column range), once for the dB
    blocks (formed as the full [Σr, N] product over the fused output, of which each adapter keeps its block: extra FLOPs, no extra pass).  A and B are cast to the model dtype once per call; the scalings multiply fp32 accumulators (a GEMM's alpha, or the kernels'
    per-rank scale), never a rounded copy of B; gradients come back in each adapter parameter's dtype (fp32 adapters: the fp32 slab sum
    of the weight-gradient kernel, unrounded).  Each product runs in the form measured faster at its shape (see above).  Saves x, xa."""

    @staticmethod
    def forward(ctx, x, w, b, spec, *ab):
        dt = x.dtype
        As, Bs = ab[0::2], ab[1::2]
        quantized = isinstance(w, QuantOperand)          # where the base operand comes from is the only difference (see QuantOperand)
        y = F.linear(x, w.matrix(False) if quantized else w, b)
        a_cat = torch.cat([a.to(dt) for a in As]) if len(As) > 1 else As[0].to(dt)
        if not a_cat.is_contiguous():
            a_cat = a_cat.contiguous()
        xa = lora_down(x, a_cat) if _down_by_kernel(x.shape[1], a_cat.shape[0]) else x @ a_cat.t()
        bs = [B_.to(dt) for B_ in Bs]
        r0 = 0
        for (n0, nlen, r, s), B_ in zip(spec, bs):                      # y_seg += s · xa_seg · B_segᵀ in place (alpha on the fp32 accumulator)
            y[:, n0:n0 + nlen].addmm_(xa[:, r0:r0 + r], B_.t(), alpha=s); r0 += r
        ctx.save_for_backward(x, xa, a_cat, *bs, *(() if quantized else (w,)))
        ctx.quant_base = w if quantized else None        # the codes and scales by reference; never the expanded matrix
        ctx.spec, ctx.has_bias, ctx.ab_dtypes = spec, b is not None, [t.dtype for t in ab]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, xa, a_cat = ctx.saved_tensors[:3]
        bs = ctx.saved_tensors[3:3 + len(ctx.spec)]
        w = ctx.quant_base if ctx.quant_base is not None else ctx.saved_tensors[-1]
        spec, dt = ctx.spec, x.dtype
        dy = dy.contiguous()
        R, N = a_cat.shape[0], dy.shape[1]
        seg_scale, r0 = [], 0
        for n0, nlen, r, s in spec:
            seg_scale.append((r0, r, s)); r0 += r
        if _down_by_kernel(N, R):          # one pass over dy against the block-diagonal [Σr, N] of the B_iᵀ (the products with zeros are free)
            bd = torch.zeros((R, N), dtype=dt, device=x.device)
            rs = np.ones(R, np.float32)
            for (n0, nlen, r, s), (q0, _, _), B_ in zip(spec, seg_scale, bs):
                bd[q0:q0 + r, n0:n0 + nlen] = B_.t(); rs[q0:q0 + r] = s
            dxa = lora_down(dy, bd, rs)
        else:                              # every adapter reads its own columns of dy: still one pass over dy in all
            dxa = torch.empty((dy.shape[0], R), dtype=dt, device=x.device)
            for (n0, nlen, r, s), (q0, _, _), B_ in zip(spec, seg_scale, bs):
                torch.addmm(dxa[:, q0:q0 + r], dy[:, n0:n0 + nlen], B_, beta=0, alpha=s, out=dxa[:, q0:q0 + r])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = w.dgrad(dy) if ctx.quant_base is not None else _dgrad(dy, w)
            dx = dx.addmm_(dxa, a_cat) if dx.is_contiguous() else dx + dxa @ a_cat
        dw = _wgrad(x, dy, w.shape[1] >= 2 * w.shape[0]) if ctx.needs_input_grad[1] else None
        db = dy.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        need = ctx.needs_input_grad[4:]
        g32 = lambda i: torch.float32 if ctx.ab_dtypes[i] == torch.float32 else dt
        dA = dB = None
        if any(need[0::2]):
            dA = _lora_wgrad(dxa, x, torch.float32 if any(ctx.ab_dtypes[i] == torch.float32 for i in range(0, len(need), 2)) else dt)
        if any(need[1::2]):
            dB = _lora_wgrad(xa, dy, torch.float32 if any(ctx.ab_dtypes[i] == torch.float32 for i in range(1, len(need), 2)) else dt, seg_scale)
        out, r0 = [], 0
        for i, (n0, nlen, r, _) in enumerate(spec):
            out.append(dA[r0:r0 + r].to(g32(2 * i)) if need[2 * i] else None)
            out.append(dB[r0:r0 + r, n0:n0 + nlen].t().to(g32(2 * i + 1)).contiguous() if need[2 * i + 1] else None)
            r0 += r
        return (dx, dw, db, None, *out)


def lora_linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], adapters) -> torch.Tensor:
    """x [rows, in] through a (fused) projection with adapters: `w` [N, in] the base weight (stacked over the group's members), `adapters`
    a list of (n0, nlen, A [r, in], B [nlen, r], scaling) - one per member that carries one, in column order.  bf16 / f16 on the device:
    _LoraLinear (the HIP kernels where they are the faster form).  fp32 models (the gradient-check path) and host tensors: the same arithmetic as torch expressions."""
    if not adapters:
        return linear(x, w, b)
    if x.is_cuda and x.dtype in (torch.bfloat16, torch.float16):
        spec = tuple((int(n0), int(nlen), int(A.shape[0]), float(s)) for n0, nlen, A, B_, s in adapters)
        ab = [t for _, _, A, B_, _ in adapters for t in (A, B_)]
        return _LoraLinear.apply(x, w, b, spec, *ab)
    y = linear(x, w, b)
    cols, o = [], 0
    for n0, nlen, A, B_, s in adapters:
        if n0 > o:
            cols.append(y[:, o:n0])
        cols.append(y[:, n0:n0 + nlen] + float(s) * ((x @ A.to(x.dtype).t()) @ B_.to(x.dtype).t()))
        o = n0 + nlen
    if o < y.shape[1]:
        cols.append(y[:, o:])
    return cols[0] if len(cols) == 1 else torch.cat(cols, dim=1)


# ------------------------------------------------------------------------------------------------------------------------------------
# Quantised frozen base (quant.py, include/dta.h "Quantised frozen base"): block codes + fp32 scales, expanded to the model dtype per use
# ------------------------------------------------------------------------------------------------------------------------------------
QUANT_FMT = {"nf4": 0, "fp8": 1}
QUANT_BLOCK = {"nf4": 64, "fp8": 128}


def quant_blockwise(w: torch.Tensor, fmt: str):
    """(codes uint8 [R, C / 2] (nf4) or [R, C] (fp8), scales fp32 [R, C / block]) of a weight [R, C] with contiguous rows (dta_quant_blockwise)."""
    R, C = w.shape
    assert w.stride(1) == 1 and C % QUANT_BLOCK[fmt] == 0
    q = torch.empty((R, C // 2 if fmt == "nf4" else C), dtype=torch.uint8, device=w.device)
    scales = torch.empty((R, C // QUANT_BLOCK[fmt]), dtype=torch.float32, device=w.device)
    _launch("dta_quant_blockwise", (w, q, scales), ptr(w), w.stride(0), R, C, _DT[w.dtype], QUANT_FMT[fmt], ptr(q), ptr(scales),
            nbytes=R * C * w.element_size() + q.numel() + scales.numel() * 4)
    return q, scales


def dequant_blockwise(q: torch.Tensor, scales: torch.Tensor, fmt: str, out: torch.Tensor, transposed: bool = False) -> torch.Tensor:
    """Expands codes + scales of a weight [R, C] into `out` (dta_dequant_blockwise): a [R, C] window with contiguous rows at any pitch -
    a row range of a stacked operand - or, `transposed`, a [C, R] window - a column range of a transposed stacked operand."""
    R, C = scales.shape[0], scales.shape[1] * QUANT_BLOCK[fmt]
    assert q.is_contiguous() and scales.is_contiguous() and out.stride(1) == 1 and tuple(out.shape) == ((C, R) if transposed else (R, C))
    _launch("dta_dequant_blockwise", (q, scales, out), ptr(q), ptr(scales), R, C, QUANT_FMT[fmt], ptr(out), out.stride(0), _DT[out.dtype],
            int(transposed), nbytes=q.numel() + scales.numel() * 4 + R * C * out.element_size())
    return out


class QuantOperand:
    """The base operand of one fused projection group (q|k|v, gate|up, or one module) held as block codes: `mods` are the group's
    quant.QuantLinear members in row order.  `matrix` expands them into ONE transient operand from the caching allocator - each member
    straight into its row range (or, transposed, its column range): no stack_rows copy, no transpose pass - which the caller drops after
    its GEMM.  It never enters weight_cache, _StackRows._cache or _TransposedWeights.cache, and an autograd node holds this object (the
    codes and scales by reference), never a matrix."""
    __slots__ = ("mods", "dtype", "shape")

    def __init__(self, mods, dtype):
        self.mods, self.dtype = tuple(mods), dtype
        self.shape = (sum(m.out_features for m in self.mods), self.mods[0].in_features)

    def matrix(self, transposed: bool) -> torch.Tensor:
        N, K = self.shape
        out = torch.empty((K, N) if transposed else (N, K), dtype=self.dtype, device=self.mods[0].qweight.device)
        o = 0
        for m in self.mods:
            r = m.out_features
            dequant_blockwise(m.qweight, m.scales, m.fmt, out[:, o:o + r] if transposed else out[o:o + r], transposed)
            o += r
        return out

    def dgrad(self, dy: torch.Tensor) -> torch.Tensor:
        """dx = dy · W in the orientation `_dgrad` takes for this shape, on a freshly expanded operand."""
        # a member's column range of the transposed operand must start on 16 bytes: every member's rows a multiple of 8, not the sum alone
        if _dgrad_transposed(dy, self.shape, self.dtype) and all(m.out_features % 8 == 0 for m in self.mods):
            return dy @ self.matrix(True).t()
        return dy @ self.matrix(False)


class _QuantLinear(torch.autograd.Function):
    """y = x Wᵀ (+ b) on a quantised base without adapters (a quantised MLP beside adapted attention projections): nothing is saved but
    the operand's codes by reference - the base has no weight gradient, so not even x."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.quant_base, ctx.has_bias = w, b is not None
        return F.linear(x, w.matrix(False), b)

    @staticmethod
    def backward(ctx, dy):
        dx = ctx.quant_base.dgrad(dy) if ctx.needs_input_grad[0] else None
        db = dy.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, None, db


def quant_linear(x: torch.Tensor, qmods, b: Optional[torch.Tensor], adapters) -> torch.Tensor:
    """x [rows, in] through a (fused) projection whose base members `qmods` are quantised (quant.QuantLinear), with `adapters` as
    lora_linear takes them.  bf16 / f16 on the device: the group is expanded by dta_dequant_blockwise into one transient operand for the
    forward GEMM and again, only if dx is needed, for the backward; the adapter arithmetic is _LoraLinear's.  Host tensors (the CPU
    stand-ins): the same arithmetic in torch expressions on quant.dequantize_host."""
    if x.is_cuda:
        if x.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"a quantised base serves bf16 / f16 models; the input is {x.dtype}")
        op = QuantOperand(qmods, x.dtype)
        if not adapters:
            return _QuantLinear.apply(x, op, b)
        spec = tuple((int(n0), int(nlen), int(A.shape[0]), float(s)) for n0, nlen, A, B_, s in adapters)
        return _LoraLinear.apply(x, op, b, spec, *[t for _, _, A, B_, _ in adapters for t in (A, B_)])
    from . import quant
    ws = [quant.dequantize_host(m.qweight, m.scales, m.fmt, x.dtype) for m in qmods]
    return lora_linear(x, ws[0] if len(ws) == 1 else torch.cat(ws), b, adapters)


# --------------------------------------------------------------------------------------------------
# Policy objective over packed rows (losses.PolicyLoss, dta_policy_loss)
# --------------------------------------------------------------------------------------------------
def _cat_per_token(vals, fill, seq_ptr, device):
    """One fp32 device vector of N = seq_ptr[-1] elements from one entry per sequence (callback order): a tensor [n_s], or None / a float,
    which stand for `fill` / that float on every token of the sequence.  Entries that all live on the host are concatenated there and
    uploaded once out of page-locked staging; tensors already on the device are concatenated there."""
    from ._staging import upload
    N = int(seq_ptr[-1])
    lens = np.diff(np.asarray(seq_ptr, np.int64))
    if all(not isinstance(v, torch.Tensor) or not v.is_cuda for v in vals):
        host = np.empty(N, np.float32)
        for v, b, n in zip(vals, seq_ptr[:-1], lens):
            host[b:b + n] = fill if v is None else v if isinstance(v, float) else v.detach().to(torch.float32).numpy()
        return upload([host], device, np.float32)[0]
    if all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == vals[0].dtype for v in vals):
        return torch.cat([v.detach().to(device) for v in vals]).to(torch.float32)       # one concatenation, one cast (bool masks)
    parts = [torch.full((int(n),), fill if v is None else v, dtype=torch.float32, device=device) if not isinstance(v, torch.Tensor)
             else v.detach().to(device=device, dtype=torch.float32) for v, n in zip(vals, lens)]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=device)


def _sequence_fields(loss, attach_lists, seq_ptr):
    """loss.fields(attachment, n) of every sequence, in callback order; n = len - 1 must be the sequence's extent in seq_ptr."""
    s = 0
    for attach_list in attach_lists:
        for attachment, length in attach_list:
            n = int(length) - 1
            if n != int(seq_ptr[s + 1]) - int(seq_ptr[s]):
                raise ValueError("attach lists and seq_ptr disagree")
            yield loss.fields(attachment, n)
            s += 1


def _f32_aligned(t):
    """fp32, contiguous and on a 16-byte boundary (a view into a larger buffer may start anywhere); None stays None"""
    if t is None:
        return None
    t = t.detach().to(torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _carve_f32(device, **parts):
    """One fp32 device buffer carved into the named vectors of the given lengths, in order, each on a 16-byte boundary (a part takes a
    multiple of 4 floats): (buffer, {name: view})."""
    r4 = lambda n: (n + 3) // 4 * 4
    buf = torch.empty(sum(r4(n) for n in parts.values()), dtype=torch.float32, device=device)
    views, o = {}, 0
    for name, n in parts.items():
        views[name] = buf[o:o + n]
        o += r4(n)
    return buf, views


def policy_token_inputs(loss, attach_lists, seq_ptr, device):
    """The per-token inputs of the fused objective, concatenated in callback order behind seq_ptr: (old, ref, mask, adv, adv_per_seq), fp32
    device vectors of N = seq_ptr[-1] elements (old / ref None: on-policy / no KL; adv one value per sequence when every attachment gives
    a float).  Each key is checked as PolicyLoss.__call__ checks it.  A key whose tensors all live on the host is concatenated there and
    uploaded once out of page-locked staging; tensors already on the device are concatenated there."""
    from ._staging import upload
    fields = list(_sequence_fields(loss, attach_lists, seq_ptr))
    advs, olds, refs, masks = ([f[k] for f in fields] for k in range(4))
    cat = lambda vals, fill: _cat_per_token(vals, fill, seq_ptr, device)
    if any(v is None for v in olds) and not all(v is None for v in olds):
        raise ValueError("old_logprobs: given for some sequences of the trie and absent for others")
    old = None if all(v is None for v in olds) else cat(olds, 0.0)
    ref = None if loss.kl_coef == 0 else cat(refs, 0.0)
    mask = cat(masks, 1.0)
    adv_per_seq = all(isinstance(v, float) for v in advs)
    adv = upload([np.asarray(advs, np.float32)], device, np.float32)[0] if adv_per_seq else cat(advs, 0.0)
    return old, ref, mask, adv, adv_per_seq


def policy_rollout_input(loss, attach_lists, seq_ptr, device):
    """The rollout log-probs of an off-policy correction (attachment key rollout_logprobs), concatenated like the vectors of
    policy_token_inputs: an fp32 device vector of N = seq_ptr[-1] elements, or None when loss.is_level is None (the key is not looked at).
    Checked as PolicyLoss.__call__ checks it; given for some sequences and absent for others is a ValueError."""
    if loss.is_level is None:
        return None
    rolls = []
    for s, (attachment, length) in enumerate(pair for attach_list in attach_lists for pair in attach_list):
        n = int(length) - 1
        if n != int(seq_ptr[s + 1]) - int(seq_ptr[s]):
            raise ValueError("attach lists and seq_ptr disagree")
        rolls.append(attachment.get("rollout_logprobs"))
        if rolls[-1] is not None:
            loss.rollout(attachment, n)
    if any(v is None for v in rolls):
        if not all(v is None for v in rolls):
            raise ValueError("rollout_logprobs: given for some sequences of the trie and absent for others")
        raise KeyError(f"rollout_logprobs (required because is_level = {loss.is_level!r})")
    return _cat_per_token(rolls, 0.0, seq_ptr, device)


def policy_walks_paths(loss, on_policy: bool) -> bool:
    """Whether the fused objective follows root paths and so needs packing.policy_path_tables: a sequence-level ratio, or a
    sequence-level rollout weight formed from the rows' own log-probs (no old_logprobs: on_policy)."""
    return loss.ratio == "sequence" or (loss.is_level in ("sequence", "sequence_mean") and on_policy)


def policy_loss(loss, lp: torch.Tensor, ent: torch.Tensor, depth: torch.Tensor, row_seq_lo: torch.Tensor, row_seq_hi: torch.Tensor,
                seq_ptr: torch.Tensor, old: Optional[torch.Tensor], ref: Optional[torch.Tensor], mask: torch.Tensor, adv: torch.Tensor,
                adv_per_seq: bool, path_tables=None, rollout: Optional[torch.Tensor] = None, workspaces: Optional[dict] = None):
    """The objective `loss` (losses.PolicyLoss) over T packed rows in one C-ABI call (dta_policy_loss): returns (dlp [T], dent [T], stats,
    w [S]), fp32.  lp / ent: the fp32 row statistics of packed_logprob_entropy (no graph is followed: the caller back-propagates dlp /
    dent); row_seq_lo / row_seq_hi / seq_ptr: packing.policy_row_tables; old / ref / mask / adv: policy_token_inputs.
    stats = {loss, sum m pg, sum m kl, sum m entropy, clipped tokens, sum m} (losses.STATS), with the two entries more of
    losses.OFFPOLICY_STATS under an off-policy correction or CISPO (loss.extended); w: the per-sequence weights.
    path_tables = (leaf_run_ptr, run_row0, run_depth0, seq_leaf), the int32 device tables of packing.policy_path_tables, are needed
    exactly when policy_walks_paths(loss, old is None), rollout = policy_rollout_input(...) exactly when loss.is_level is not None.
    A dict handed in as `workspaces` receives the per-sequence vectors c and omega."""
    from .losses import AGGREGATIONS, IS_LEVELS, IS_MODES, KL_ESTIMATORS, OFFPOLICY_STATS, RATIOS, STATS, SURROGATES
    walks = policy_walks_paths(loss, old is None)
    if walks != (path_tables is not None):
        raise ValueError(f"ratio = {loss.ratio!r}, is_level = {loss.is_level!r}, old_logprobs {'absent' if old is None else 'given'}: "
                         f"path_tables (packing.policy_path_tables) are {'needed' if walks else 'not used'}")
    if (loss.is_level is not None) != (rollout is not None):
        raise ValueError(f"is_level = {loss.is_level!r}: rollout (policy_rollout_input) goes with an off-policy correction, and only with it")
    T, S = int(lp.shape[0]), int(seq_ptr.shape[0]) - 1
    lp, ent, old, ref, rollout, mask, adv = map(_f32_aligned, (lp, ent, old, ref, rollout, mask, adv))
    path = list(path_tables) if walks else [None] * 4
    _require_cuda(lp, ent, depth, row_seq_lo, row_seq_hi, seq_ptr, old, ref, rollout, mask, adv, *path)
    N = int(mask.shape[0])
    assert ent.shape[0] == T and depth.shape[0] == T and row_seq_lo.shape[0] == T and row_seq_hi.shape[0] == T
    assert all(t.dtype == torch.int32 for t in (depth, row_seq_lo, row_seq_hi, seq_ptr, *path) if t is not None)
    assert adv.shape[0] == (S if adv_per_seq else N) and all(t is None or t.shape[0] == N for t in (old, ref, rollout))
    M = R = 0
    if walks:
        run_ptr, run_row0, run_depth0, seq_leaf = path
        assert seq_leaf.shape[0] == S and run_depth0.shape[0] == run_row0.shape[0]
        M, R = int(run_ptr.shape[0]) - 1, int(run_row0.shape[0])
    nb = lib().dta_policy_loss_blocks(T, S)
    buf, v = _carve_f32(lp.device, dlp=T, dent=T, w=S, partial=8 * nb, stats=8, c=S, omega=S)
    tensors = (lp, ent, depth, row_seq_lo, row_seq_hi, seq_ptr, *path, old, ref, rollout, mask, adv)
    _launch("dta_policy_loss", (*tensors, buf),
            *map(ptr, tensors), int(bool(adv_per_seq)), *(ptr(v[k]) for k in ("w", "c", "omega", "dlp", "dent", "partial", "stats")),
            T, S, M, R,
            float(loss.clip_low), float(loss.clip_high), 0.0 if loss.dual_clip is None else float(loss.dual_clip), float(loss.kl_coef),
            KL_ESTIMATORS.index(loss.kl_estimator), float(loss.entropy_coef), AGGREGATIONS.index(loss.agg), float(loss.scale),
            RATIOS.index(loss.ratio), SURROGATES.index(loss.surrogate), 0 if loss.is_level is None else IS_LEVELS.index(loss.is_level) + 1,
            IS_MODES.index(loss.is_mode), float(loss.is_cap), float(loss.is_floor),
            nbytes=4 * (4 * T + (4 + (old is not None) + (ref is not None) + 2 * (rollout is not None)) * N))
    if workspaces is not None:
        workspaces.update(c=v["c"], omega=v["omega"])
    return v["dlp"], v["dent"], v["stats"][:len(OFFPOLICY_STATS if loss.extended else STATS)], v["w"]


# --------------------------------------------------------------------------------------------------
# Preference objectives over packed rows (losses.PreferenceLoss, dta_preference_loss)
# --------------------------------------------------------------------------------------------------
def preference_token_inputs(loss, attach_lists, seq_ptr, device):
    """The per-token and per-sequence inputs of the fused preference objective in callback order: (ref_lp, ref_sum, mask) - mask fp32 [N]
    (N = seq_ptr[-1]); the reference as per-token log-probs ref_lp fp32 [N] or as masked sums ref_sum fp32 [S], the other None; both None
    with loss.reference_free.  Each key is checked as PreferenceLoss.fields checks it, and one form of the reference must serve every
    sequence.  Staging as policy_token_inputs (_cat_per_token)."""
    from ._staging import upload
    fields = list(_sequence_fields(loss, attach_lists, seq_ptr))
    masks, refs, sums = ([f[k] for f in fields] for k in range(3))
    if not loss.reference_free and any(v is None for v in refs) and any(v is None for v in sums):
        raise ValueError("ref_logprobs for some sequences of the trie and ref_logprob_sum for others: one form of the reference per call")

    cat = lambda vals, fill: _cat_per_token(vals, fill, seq_ptr, device)
    mask = cat(masks, 1.0)
    per_token = not loss.reference_free and all(v is not None for v in refs)
    ref_lp = cat(refs, 0.0) if per_token else None
    ref_sum = None if loss.reference_free or per_token else upload([np.asarray(sums, np.float32)], device, np.float32)[0]
    return ref_lp, ref_sum, mask


def preference_loss(loss, lp: torch.Tensor, depth: torch.Tensor, row_seq_lo: torch.Tensor, row_seq_hi: torch.Tensor, seq_ptr: torch.Tensor,
                    path_tables, pair_tables, ref_lp: Optional[torch.Tensor], ref_sum: Optional[torch.Tensor], mask: torch.Tensor):
    """The objective `loss` (losses.PreferenceLoss) over T packed rows in one C-ABI call (dta_preference_loss): returns
    (dlp [T], stats [8], g [S], u [S]), fp32.  lp: the fp32 row log-probs of packed_logprob_entropy (no graph is followed: the caller
    back-propagates dlp); row_seq_lo / row_seq_hi / seq_ptr: packing.policy_row_tables; path_tables = (leaf_run_ptr, run_row0,
    run_depth0, seq_leaf): packing.policy_path_tables; pair_tables = (pair_c, pair_r): packing.preference_pair_tables - all int32 on the
    device; ref_lp / ref_sum / mask: preference_token_inputs.  stats in the order of losses.PREFERENCE_STATS; g: the per-sequence
    gradient coefficients (d loss / d lp[row(s, j)] = g[s] mask[j]); u: the per-sequence (length-normalised) log-ratio sums."""
    from .losses import PREFERENCE_KINDS
    T, S = int(lp.shape[0]), int(seq_ptr.shape[0]) - 1
    lp, ref_lp, ref_sum, mask = map(_f32_aligned, (lp, ref_lp, ref_sum, mask))
    run_ptr, run_row0, run_depth0, seq_leaf = path_tables
    pair_c, pair_r = pair_tables
    _require_cuda(lp, depth, row_seq_lo, row_seq_hi, seq_ptr, run_ptr, run_row0, run_depth0, seq_leaf, pair_c, pair_r, ref_lp, ref_sum, mask)
    N, P = int(mask.shape[0]), int(pair_c.shape[0])
    M, R = int(run_ptr.shape[0]) - 1, int(run_row0.shape[0])
    if loss.reference_free:
        ref_lp = ref_sum = None
    elif (ref_lp is None) == (ref_sum is None):
        raise ValueError("exactly one of ref_lp and ref_sum is needed (neither with reference_free)")
    if 2 * P != S:
        raise ValueError(f"{P} pairs for {S} sequences: every sequence of the trie is a member of exactly one pair")
    assert depth.shape[0] == T and row_seq_lo.shape[0] == T and row_seq_hi.shape[0] == T and seq_leaf.shape[0] == S
    assert run_depth0.shape[0] == R and pair_r.shape[0] == P
    assert all(t.dtype == torch.int32 for t in (depth, row_seq_lo, row_seq_hi, seq_ptr, run_ptr, run_row0, run_depth0, seq_leaf, pair_c, pair_r))
    assert (ref_lp is None or ref_lp.shape[0] == N) and (ref_sum is None or ref_sum.shape[0] == S)
    nb = lib().dta_preference_loss_blocks(T, S, P)
    buf, v = _carve_f32(lp.device, dlp=T, nhat=S, u=S, sft=S, g=S, partial=8 * nb, stats=8)
    tensors = (lp, depth, row_seq_lo, row_seq_hi, seq_ptr, run_ptr, run_row0, run_depth0, seq_leaf, pair_c, pair_r, ref_lp, ref_sum, mask)
    _launch("dta_preference_loss", (*tensors, buf), *map(ptr, tensors),
            *(ptr(v[k]) for k in ("nhat", "u", "sft", "g", "dlp", "partial", "stats")), T, S, M, R, P,
            PREFERENCE_KINDS.index(loss.kind), float(loss.beta), float(loss.label_smoothing), float(loss.gamma),
            int(loss.length_normalize), int(loss.reference_free), float(loss.sft_coef), float(loss.scale),
            nbytes=4 * (5 * T + (2 + (ref_lp is not None)) * N))
    return v["dlp"], v["stats"], v["g"], v["u"]
