"""Float64 restatement of the partial RoPE kernels of csrc/elementwise_kernels.hip (dta_rope_partial_fwd / _bwd: the first R of D
elements of a head rotated, in half-split or interleaved pairs; no norm) with a per-element error bound for every output.

The bounds are the RoPE-only rows of tests/rowops_ref64.py (imported; no constant of their own), a = an element, b = its partner with
the pairing's sign, c / s the table values the pair shares:

    y    u |y| + (RSTD_C + 5) u32 (|a c| + |b s|) + TINY          (the "RoPE y" row without a norm weight)
    dx   u |dx| + 3 u32 (|dy c| + |dy' s|) + TINY                 (the "RoPE only" backward row)
    elements R .. D-1: bound 0 - the kernel copies them bit for bit.

pairing 0 (half-split, Phi-3):   i < R/2:  y[i]  = x[i]  c[i] - x[i+R/2] s[i],   y[i+R/2] = x[i+R/2] c[i] + x[i]  s[i]
pairing 1 (interleaved, GLM-4):  i < R/2:  y[2i] = x[2i] c[i] - x[2i+1]  s[i],   y[2i+1]  = x[2i+1]  c[i] + x[2i] s[i]
The backward is the rotation by the negative angle.  The references take the kernels' ROUNDED inputs and the fp32 table as given
([T, R] = {cos[R/2], sin[R/2]}), as rowops_ref64 does.

emulate() is the kernel's arithmetic in fp32 on the host - the products and the sum in fp32 (fused or not: both orders are tried by the
CPU test), one rounding to the storage type, the pass-through elements untouched - and takes the deliberate errors of
tests/test_partial_rope_ref64.py as arguments."""
import torch

from rowops_ref64 import RSTD_C, TINY, U, U32, _d


def spread(cos_sin, R, pairing, dt=None):
    """The [T, R] table {cos[R/2], sin[R/2]} laid out per element of the rotated region: (cos [T, 1, R], sin [T, 1, R])."""
    cs = cos_sin if dt is None else cos_sin.to(dt)
    c, s = cs[:, :R // 2], cs[:, R // 2:]
    if pairing == 0:
        return torch.cat([c, c], -1)[:, None, :], torch.cat([s, s], -1)[:, None, :]
    return c.repeat_interleave(2, -1)[:, None, :], s.repeat_interleave(2, -1)[:, None, :]


def partner(a, pairing):
    """rotate_half of the rotated region `a` [..., R] under the pairing: y = a cos + partner(a) sin."""
    R = a.shape[-1]
    if pairing == 0:
        return torch.cat([-a[..., R // 2:], a[..., :R // 2]], -1)
    return torch.stack([-a[..., 1::2], a[..., 0::2]], -1).flatten(-2)


def _ref(x, cos_sin, pairing, sgn, dtype, c32):
    x64 = _d(x)
    R = cos_sin.shape[1]
    cos, sin = spread(_d(cos_sin), R, pairing)
    a = x64[..., :R]
    b = partner(a, pairing)
    y, mag = a * cos + sgn * b * sin, (a * cos).abs() + (b * sin).abs()
    bound = U[dtype] * y.abs() + c32 * U32 * mag + TINY[dtype]
    rest = x64[..., R:]
    return torch.cat([y, rest], -1), torch.cat([bound, torch.zeros_like(rest)], -1)


def fwd_ref(x, cos_sin, pairing, dtype):
    """x [T, NH, D], cos_sin [T, R] fp32 as given -> {"y": (ref, bound)}; bound 0 on the elements R .. D-1."""
    return {"y": _ref(x, cos_sin, pairing, 1.0, dtype, RSTD_C + 5)}


def bwd_ref(dy, cos_sin, pairing, dtype):
    """-> {"dx": (ref, bound)}: the rotation by the negative angle."""
    return {"dx": _ref(dy, cos_sin, pairing, -1.0, dtype, 3.0)}


def emulate(x, cos_sin, pairing, sgn=1.0, fused=False, rotate_all=False):
    """The kernel's arithmetic on the host: fp32 products and sum (`fused`: the second product enters by an fma, emulated in float64
    with one rounding to fp32), one rounding to x's dtype, elements R.. untouched.  `rotate_all`: the deliberate error of rotating
    the pass-through region too (by the table's first entries)."""
    R = cos_sin.shape[1]
    cos, sin = spread(cos_sin.float(), R, pairing)
    a = x[..., :R].float()
    b = partner(a, pairing)
    if fused:
        y = ((a * cos).double() + sgn * b.double() * sin.double()).float()
    else:
        y = a * cos + sgn * (b * sin)
    rest = x[..., R:]
    if rotate_all and rest.shape[-1]:
        n = rest.shape[-1]
        r = rest.float()
        rest = (r * cos[..., :n] + sgn * partner(r, pairing) * sin[..., :n]).to(x.dtype)
    return torch.cat([y.to(x.dtype), rest], -1)
