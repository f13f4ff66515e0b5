"""CPU stand-ins for ops.rope_partial / ops.qkv_prep_partial: HF's own formulas - Phi-3's apply_rotary_pos_emb (rotate_half over the
first rotary_dim elements) and GLM-4's (interleaved pairs) - in the tensors' own dtype - and a stack attention that takes the sliding
window of Phi-3 (hostmirror's has none: no family before ran the block-wise walk with a window on the CPU).  install(monkeypatch) goes
BEFORE hostmirror.install (family.check_cpu_engine_matches_fixture calls that itself): the windowed stack attention is put in
hostmirror's own place, from where hostmirror.install hands it to the product; tests/hostmirror.py keeps its fixed set."""
import torch

import hostmirror


def plain_partial(x, cos_sin, interleaved):
    """x [T, NH, D], cos_sin [T, R] = {cos[R/2], sin[R/2]} -> RoPE over x[..., :R] as HF writes it, x[..., R:] as it is."""
    R = cos_sin.shape[1]
    c, s = cos_sin[:, :R // 2].to(x.dtype), cos_sin[:, R // 2:].to(x.dtype)
    rot, rest = x[..., :R], x[..., R:]
    if interleaved:
        cos, sin = c.repeat_interleave(2, -1)[:, None, :], s.repeat_interleave(2, -1)[:, None, :]
        half = torch.stack((-rot[..., 1::2], rot[..., 0::2]), dim=-1).flatten(-2)
    else:
        cos, sin = torch.cat([c, c], -1)[:, None, :], torch.cat([s, s], -1)[:, None, :]
        half = torch.cat((-rot[..., R // 2:], rot[..., :R // 2]), dim=-1)
    return torch.cat([rot * cos + half * sin, rest], -1)


def _cpu_qkv_prep_partial(qkv, cos_sin, Hq, Hkv, interleaved):
    q, k, v = qkv.split([Hq, Hkv, Hkv], dim=1)
    return plain_partial(q, cos_sin, interleaved), plain_partial(k, cos_sin, interleaved), v


def _rect_window_attention(q, k, v, start, scale, window):
    """q [Hq, B, D], k / v [Hkv, start + B, D] -> [B, Hq, D]: attn_oracle.rect_causal_attention with t - s < window."""
    Hq, B, D = q.shape
    rep = Hq // k.shape[0]
    kk, vv = k.repeat_interleave(rep, dim=0), v.repeat_interleave(rep, dim=0)
    s = torch.matmul(q.float(), kk.float().transpose(1, 2)) * scale
    qpos, kpos = torch.arange(start, start + B)[:, None], torch.arange(start + B)[None, :]
    s = s.masked_fill(~((kpos <= qpos) & (qpos - kpos < window)), float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vv.float()).transpose(0, 1).to(q.dtype)


class _CpuWindowStackAttention(torch.autograd.Function):
    """hostmirror._CpuStackAttention with a window: the same side effects on the K/V and gradient stacks."""

    @staticmethod
    def forward(ctx, q, k_new, v_new, kst, vst, gk, gv, start, scale, window):
        end = start + q.shape[0]
        kst[start:end].copy_(k_new); vst[start:end].copy_(v_new)
        ctx.save_for_backward(q)
        ctx.stacks, ctx.span, ctx.args = (kst, vst, gk, gv), (start, end), (scale, window)
        return _rect_window_attention(q.transpose(0, 1), kst[:end].transpose(0, 1), vst[:end].transpose(0, 1), start, scale, window)

    @staticmethod
    def backward(ctx, dout):
        (q,) = ctx.saved_tensors
        kst, vst, gk, gv = ctx.stacks
        start, end = ctx.span
        with torch.enable_grad():
            q_, k_, v_ = (t.detach().clone().requires_grad_(True) for t in (q, kst[:end], vst[:end]))
            out = _rect_window_attention(q_.transpose(0, 1), k_.transpose(0, 1), v_.transpose(0, 1), start, *ctx.args)
            dq, dk, dv = torch.autograd.grad(out, (q_, k_, v_), dout)
        gk[:end] += dk.float(); gv[:end] += dv.float()
        return dq, gk[start:end].to(q.dtype), gv[start:end].to(q.dtype), None, None, None, None, None, None, None


_plain_stack_attention = hostmirror._cpu_stack_attention


def _cpu_stack_attention(q, k_new, v_new, kst, vst, gk, gv, start, scale=None, window=0):
    if window <= 0:
        return _plain_stack_attention(q, k_new, v_new, kst, vst, gk, gv, start, scale)
    return _CpuWindowStackAttention.apply(q, k_new, v_new, kst, vst, gk, gv, start, q.shape[-1] ** -0.5 if scale is None else scale, window)


def install(monkeypatch):
    from dynamictreeattn_amd import ops
    monkeypatch.setattr(ops, "rope_partial", plain_partial)
    monkeypatch.setattr(ops, "qkv_prep_partial", _cpu_qkv_prep_partial)
    monkeypatch.setattr(hostmirror, "_cpu_stack_attention", _cpu_stack_attention)
