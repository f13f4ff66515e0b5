"""Float64 restatement of the two OLMo row kernels of csrc/elementwise_kernels.hip - the projection-wide q/k RMSNorm + RoPE
(dta_wide_qk_norm_rope_fwd / _bwd) and RMSNorm-then-add (dta_rmsnorm_add_fwd) - with a per-element error bound for every output.

The bounds are assembled from the terms tests/rowops_ref64.py defines (imported; no constant of their own), with the row length
n = NH * D in place of the head's D:

    rstd        RSTD_C u32 |r|: the row statistic of rowops_ref64, one per TOKEN (the mean runs over all n elements).
    wide y      a = x r w (two roundings), b its rotate_half partner inside the head: the "RoPE y" row -
                u |y| + 2 u (|a c| + |b s|) + (RSTD_C + 5) u32 (|a c| + |b s|).
    wide dx/dw  da = dy c + partner(dy) s in fp32 (never rounded); then the "RoPE dx/dw" row with H -> n: the mean is a sum of n
                terms (C32 sqrt(n)), |dt| -> (|dy c| + |dy' s|) |w|; dw is a sum over the T tokens (C32 sqrt(T)).
    yn          the plain RMSNorm "y" row (k = 2).
    out         out = res + yn: yn's own bound (its error passes through the sum) and x_out's k = 1 on |res + yn|.

The references take the kernels' ROUNDED inputs, eps as a float and the cos/sin table as given, as rowops_ref64 does.

The kernels round the norm ONCE (Olmo2RMSNorm: cast(w x r), the weight multiplied in fp32) where the "RoPE y" and "y" rows allow for two
roundings (x r, then the product): the bounds are kept as those rows state them, so y and yn sit well inside.

OBSERVED worst err / bound on the MI355X over tests/test_gpu_rowops_olmo.py (from rowops_ref64.check; bf16 / f16 / fp32 storage):
    wide norm + RoPE (every form, grid-stride, qkv_prep_wide)   y .648/.661/.254   dx .994/.988/.046   dw .995/.994/.163   rstd .24 (of RSTD_C)
    norm, then add (every form, operator backward)              yn .494/.499/.214  out .971/.976/.959  dx .991/.969/.039   dw .992/.989/.169   rstd .47
No constant had to be re-derived.  (out at 0.96 in fp32 is the one rounding of the sum, u = u32 there.)"""
import math

import torch

from rowops_ref64 import C32, RSTD_C, TINY, U, U32, _d, _eps, _ku, _table


def _rot(a, D):
    return torch.cat([-a[..., D // 2:], a[..., :D // 2]], -1)


def wide_fwd_ref(x, w, cos_sin, eps, dtype):
    """x [T, NH, D], w [NH * D], cos_sin [T, D] fp32 as given -> {"y" [T, NH, D], "rstd" [T]}: (ref, bound)."""
    x64 = _d(x)
    T, NH, D = x64.shape
    w64 = _d(w).view(1, NH, D)
    cos, sin = _table(cos_sin, D)
    r = torch.rsqrt(x64.pow(2).mean((1, 2)) + _eps(eps))
    a = x64 * r[:, None, None] * w64
    b = _rot(a, D)
    y, mag = a * cos + b * sin, (a * cos).abs() + (b * sin).abs()
    bound = (U[dtype] * y.abs() + (RSTD_C + 5) * U32 * mag + TINY[dtype]
             + _ku(2, dtype) * mag + TINY[dtype] * 2 * (1 + w64.abs().max()))
    return {"rstd": (r, RSTD_C * U32 * r), "y": (y, bound)}


def wide_bwd_ref(x, w, cos_sin, dy, eps, dtype):
    """-> {"dx" [T, NH, D], "dw" [NH * D]}: (ref, bound)."""
    x64, g = _d(x), _d(dy)
    T, NH, D = x64.shape
    n = NH * D
    w64 = _d(w).view(1, NH, D)
    cos, sin = _table(cos_sin, D)
    gp = torch.cat([g[..., D // 2:], -g[..., :D // 2]], -1)              # the transpose of rotate_half
    da, mda = g * cos + gp * sin, (g * cos).abs() + (gp * sin).abs()
    r = torch.rsqrt(x64.pow(2).mean((1, 2), keepdim=True) + _eps(eps))
    t, dt, mdt = x64 * r, da * w64, mda * w64.abs()
    dx = r * (dt - t * (dt * t).mean((1, 2), keepdim=True))
    mag = r * (mdt + t.abs() * (mdt * t.abs()).mean((1, 2), keepdim=True))
    out = {"dx": (dx, U[dtype] * dx.abs() + (C32 * math.sqrt(n) + 3 * RSTD_C + 10) * U32 * mag + TINY[dtype])}
    dw, magw = (da * t).sum(0).reshape(n), (mda * t.abs()).sum(0).reshape(n)
    out["dw"] = (dw, U[dtype] * dw.abs() + (C32 * math.sqrt(T) + RSTD_C + 5) * U32 * magw + TINY[dtype])
    return out


def norm_add_ref(y, w, res, eps, dtype):
    """y, res [R, H], w [H] -> {"rstd" [R], "yn", "out" [R, H]}: (ref, bound)."""
    y64, w64, r64 = _d(y), _d(w), _d(res)
    r = torch.rsqrt(y64.pow(2).mean(-1) + _eps(eps))
    yn = y64 * r[:, None] * w64
    b_yn = _ku(2, dtype) * yn.abs() + (RSTD_C + 3) * U32 * yn.abs() + TINY[dtype] * (1 + w64.abs())
    out = r64 + yn
    return {"rstd": (r, RSTD_C * U32 * r), "yn": (yn, b_yn), "out": (out, b_yn + U[dtype] * out.abs() + TINY[dtype])}
