"""Float64 restatement of the row kernels of csrc/elementwise_kernels.hip (RMSNorm with and without the residual add and the weight
offset, head-norm + RoPE, SwiGLU, GeGLU) and a per-element error bound for every output.

The references take the kernels' ROUNDED inputs and the fp32 values they really receive (eps as a float, the cos/sin table as given), so
a kernel's error is its own arithmetic: the roundings to the storage type it documents, and fp32 everywhere else.  Every bound is

    bound = k u M  +  c u32 M_red  +  floor

    u = U[dtype], the largest relative error of one rounding to the storage type (2^-8 bf16, 2^-11 f16, 2^-24 fp32); k = roundings to
    the storage type on the output's path; M = the magnitude they apply to (k u is written k u (1 + k u): roundings compound);
    u32 = 2^-24; c u32 M_red = the fp32 part: c counts the fp32 operations on the path (+ C32 sqrt(n) for a sum of n terms, the
    statistical growth of ref64_common.bound) and M_red is the magnitude BEFORE any cancellation (sum of absolute terms);
    floor = TINY[dtype] (f16: the subnormal spacing 2^-24) times the factors a rounded intermediate is multiplied by.

For fp32 storage u = u32 and the same formulas hold: k u is then the rounding of the last k fp32 operations.

Per output (r = rstd, t^ = x r, w' = w_offset + w, dt = dy w'):
    rstd        RSTD_C u32 |r|.  Derived: the sum of squares (per-lane fp32 chains whose errors average out over 64 lanes: < 1; the six
                shuffle additions of the wave sum: 1 each), the division by H and the addition of eps (1 each) - all halved by the
                square root - and the hardware's rsq (1 ulp = 2 u32): 6.5 u32 if every rounding went the same way, about 4 expected.
                Measured on the MI355X over the cases of the GPU tests: 4.9 u32 (bf16, H = 16384, the two-pass forward), 2.9 u32
                up to H = 8192 and for the head norm.  RSTD_C = 10: twice the measured worst.
    x_out       k = 1 on |x + delta|.
    y           plain form k = 2 (x r is rounded, then multiplied by w), offset form k = 1; fp32: (RSTD_C + 3) u32 |y|.
    dx          k = 1; M_red = r (|dt| + |t^| mean|dt t^|) (+ |dres|), c = C32 sqrt(H) + 3 RSTD_C + 8 (r enters three times, the
                products and the two subtractions; the mean is a sum of H terms).
    dw          fp32 sum over rows, rounded once: k = 1; M_red = sum_rows |dy t^|, c = C32 sqrt(R) + RSTD_C + 3.
    RoPE y      a = x r w (two roundings, none without a norm weight), b its rotate_half partner: u |y| + 2 u (|a c| + |b s|)
                + (RSTD_C + 5) u32 (|a c| + |b s|).
    RoPE dx/dw  da = dy c + partner(dy) s in fp32 (never rounded); then as RMSNorm with H -> D and |dt| -> (|dy c| + |dy' s|) |w|;
                RoPE only: u |dx| + 3 u32 (|dy c| + |dy' s|).
    GLU y       k = 2 (the activation is rounded, then the product); dg, du: k = 1; fp32 part: the exponential below.

The exponential.  Both GLU kernels form E = exp(-z) as exp2(-z log2 e) with the hardware's 1-ulp exp2: the product's rounding moves the
argument by u32 |z| log2 e, i.e. E by the relative |z| u32, and exp2 adds 2 u32: dE = (|z| + 2 + c_z |z|) u32 with c_z the fp32
operations that formed z (SwiGLU: z = x, c_z = 0; GeGLU: z = 2 sqrt(2/pi) x (1 + 0.044715 x^2), c_z = 5).  Through the sigmoid
s = 1 / (1 + E): ds = (1 - s) dE + 2 u32 - the DERIVED figure.  MEASURED on the MI355X with fp32 storage against these references: the
SwiGLU forward over the gate range reaches 1.03 x its derived bound (3 of 4112 elements, gates near -46: an error of 54.6 u32 |y| where
53 are derived; the derivation leaves out that the float log2 e is itself off by 0.22 u32, i.e. 0.22 |z| u32 more on E), everything
else stays under 0.86.  So ds carries EXP_C = 2.06, twice the measured worst; at its largest (|z| = 100) that is 1.3e-5 |ref|, and where
it matters to a model (|z| < 20) under 3e-6 |ref|, inside the 4e-6 (1 + |ref|) of test_geglu_values_in_fp32_over_the_gate_range.
SwiGLU's backward forms 1 - s by subtraction, which cancels for large gates: that error is
carried as an absolute one (see swiglu_ref).  Two absolute floors, both far below anything a model sees: a sigmoid under the smallest
normal fp32 number (|z| > 87) may be flushed to zero (FLUSH = 2^-126 times the factors it is multiplied by; this also covers the
overflow of E to inf), and GeGLU clamps -z at 80, so s is never under e^-80 (CLAMP): where a GeGLU reference is (next to) zero the
err / bound of a correct kernel is 1.0 by construction.

OBSERVED worst err / bound on the MI355X over tests/test_gpu_rowops_bounds.py (from `check`; bf16 / f16 / fp32 storage):
    rmsnorm (all forms, wide, grid-stride)   y .992/.996/.33   x_out .996/1.0/1.0   dx .995/.990/.07   dw .995/.997/.20   rstd .49 (of RSTD_C)
    head-norm + RoPE, qkv_prep, grid-stride  y .995/.996/.30   dx .996/.999/.48   dw .981/.974/.11   rstd .26
    swiglu (separate, fused, grid-stride)    y .966/.897/.44   dg .996/.995/.41   du .996/.991/.43      gate range: f16 .74/.98/.98, fp32 .51/.50/.52
    geglu  (separate, fused, grid-stride)    y .990/.899/1.0   dg .996/.995/1.0   du .996/.995/1.0      (fp32 1.0: the clamp floor, see above)
The 2-byte figures sit at 0.99 because u is the exact worst case of ONE rounding (an element just above a power of two, rounded half an
ulp away): the CPU emulation of the same arithmetic reaches the same 0.99 (test_rowops_ref64.py); what is left for the fp32 part shows
in the fp32-storage column.  x_out at 1.0 is a correctly rounded sum that hit that worst case exactly.
"""
import math

import numpy as np
import torch

from ref64_common import C32, TINY, U, U32

RSTD_C = 10.0
EXP_C = 2.06
FLUSH = 2.0 ** -126
CLAMP = math.exp(-80.0)
K0, K1 = math.sqrt(2.0 / math.pi), float(np.float32(0.044715))          # K1: the kernel's float constant, as gelu_pytorch_tanh's
WORST: dict = {}                                                        # (name, dtype) -> largest err / bound seen by check()


def _d(t):
    return t.detach().double()


def _eps(eps):
    return float(np.float32(eps))                                       # the entry points take eps as a float


def _ku(k, dtype):
    return k * U[dtype] * (1.0 + k * U[dtype])


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
def rows(R, H, dtype, seed, scale_hi=10.0):
    """[R, H] rounded to `dtype`: row i is randn times a scale log-spaced from `scale_hi` (row 0) down to 1e-3 (mean(x^2) ~ eps);
    with R >= 4, row R//2 is all zero and row R//2 + 1 has a single non-zero element."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, H, generator=g) * torch.logspace(math.log10(scale_hi), -3.0, R)[:, None]
    if R >= 4:
        x[R // 2] = 0.0
        keep = float(x[R // 2 + 1, H // 3]) or 1.0
        x[R // 2 + 1] = 0.0; x[R // 2 + 1, H // 3] = keep
    return x.to(dtype)


def delta_for(x, seed):
    """A residual delta for rows(): random at half the row's own scale, and such that the special rows stay special in x + delta
    (the zero row's delta is -x: the sum is exactly 0; the single-element row keeps its element)."""
    g = torch.Generator().manual_seed(seed)
    R, H = x.shape
    d = (0.5 * torch.randn(R, H, generator=g) * x.float().abs().mean(-1, keepdim=True)).to(x.dtype)
    if R >= 4:
        d[R // 2] = 0
        d[R // 2 + 1] = 0
    return d


def norm_weight(H, dtype, seed, offset_form):
    g = torch.Generator().manual_seed(seed)
    return ((0.1 * torch.randn(H, generator=g)) if offset_form else (1 + 0.2 * torch.randn(H, generator=g))).to(dtype)


def randn(shape, dtype, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def gate_range(dtype):
    """The SwiGLU gate-range row: +-100 in 4097 steps and the values around the overflow of exp(-x) in fp32 (88.7), [1, 4112]."""
    big = 6e4 if dtype == torch.float16 else 1e4
    extra = [0.0] + [s * v for v in (87.0, 88.0, 89.0, 104.0, big) for s in (1, -1)] + [0.0] * 4
    return torch.cat([torch.linspace(-100, 100, 4097), torch.tensor(extra)]).view(1, -1).to(dtype)


# ------------------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_fwd_ref(x, delta, w, eps, w_offset, dtype, xin=None):
    """-> {"x_out", "rstd", "y"}: (ref, bound).  `xin`: the rounded residual stream the norm is taken of (the kernel's own x_out, once
    it passed its bound); default: x + delta rounded as the kernel rounds it (fp32 sum, then the storage type)."""
    out = {}
    if delta is not None:
        xo = _d(x) + _d(delta)
        out["x_out"] = (xo, U[dtype] * xo.abs() + TINY[dtype])
        x = xin if xin is not None else (x.float() + delta.float()).to(dtype)
    x64, wf = _d(x), w_offset + _d(w)
    r = torch.rsqrt(x64.pow(2).mean(-1) + _eps(eps))
    out["rstd"] = (r, RSTD_C * U32 * r)
    y = x64 * r[:, None] * wf
    k = 1 if w_offset else 2
    out["y"] = (y, _ku(k, dtype) * y.abs() + (RSTD_C + 3) * U32 * y.abs() + TINY[dtype] * (1 + wf.abs()))
    return out


def rmsnorm_bwd_ref(xin, w, dy, dres, eps, w_offset, dtype):
    """-> {"dx", "dw"}: (ref, bound); xin = the normalised rows (x + delta, rounded)."""
    x64, wf, g = _d(xin), w_offset + _d(w), _d(dy)
    R, H = x64.shape
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + _eps(eps))
    t, dt = x64 * r, g * wf
    dx = r * (dt - t * (dt * t).mean(-1, keepdim=True))
    mag = r * (dt.abs() + t.abs() * (dt * t).abs().mean(-1, keepdim=True))
    if dres is not None:
        dx, mag = dx + _d(dres), mag + _d(dres).abs()
    out = {"dx": (dx, U[dtype] * dx.abs() + (C32 * math.sqrt(H) + 3 * RSTD_C + 8) * U32 * mag + TINY[dtype])}
    dw, magw = (g * t).sum(0), (g * t).abs().sum(0)
    out["dw"] = (dw, U[dtype] * dw.abs() + (C32 * math.sqrt(R) + RSTD_C + 3) * U32 * magw + TINY[dtype])
    return out


# ------------------------------------------------------------------------------------------------ head-norm + RoPE
def _table(cos_sin, D):
    cs = _d(cos_sin)
    c, s = cs[:, :D // 2], cs[:, D // 2:]
    return torch.cat([c, c], -1)[:, None, :], torch.cat([s, s], -1)[:, None, :]


def qk_fwd_ref(x, w, cos_sin, eps, dtype):
    """x [T, NH, D], w [D] or None (RoPE only), cos_sin [T, D] fp32 AS GIVEN -> {"y", "rstd" (with w)}: (ref, bound)."""
    x64 = _d(x)
    D = x64.shape[-1]
    cos, sin = _table(cos_sin, D)
    out = {}
    if w is not None:
        r = torch.rsqrt(x64.pow(2).mean(-1) + _eps(eps))
        out["rstd"] = (r.reshape(-1), RSTD_C * U32 * r.reshape(-1))
        a = x64 * r[..., None] * _d(w)
    else:
        a = x64
    b = torch.cat([-a[..., D // 2:], a[..., :D // 2]], -1)
    y, mag = a * cos + b * sin, (a * cos).abs() + (b * sin).abs()
    bound = U[dtype] * y.abs() + (RSTD_C + 5) * U32 * mag + TINY[dtype]
    if w is not None:
        bound = bound + _ku(2, dtype) * mag + TINY[dtype] * 2 * (1 + _d(w).abs().max())
    out["y"] = (y, bound)
    return out


def qk_bwd_ref(x, w, cos_sin, dy, eps, dtype):
    """-> {"dx", "dw" (with w)}: (ref, bound)."""
    g = _d(dy)
    D = g.shape[-1]
    cos, sin = _table(cos_sin, D)
    gp = torch.cat([g[..., D // 2:], -g[..., :D // 2]], -1)              # the transpose of rotate_half
    da, mda = g * cos + gp * sin, (g * cos).abs() + (gp * sin).abs()
    if w is None:
        return {"dx": (da, U[dtype] * da.abs() + 3 * U32 * mda + TINY[dtype])}
    x64, w64 = _d(x), _d(w)
    r = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + _eps(eps))
    t, dt, mdt = x64 * r, da * w64, mda * w64.abs()
    dx = r * (dt - t * (dt * t).mean(-1, keepdim=True))
    mag = r * (mdt + t.abs() * (mdt * t.abs()).mean(-1, keepdim=True))
    out = {"dx": (dx, U[dtype] * dx.abs() + (C32 * math.sqrt(D) + 3 * RSTD_C + 10) * U32 * mag + TINY[dtype])}
    n = g.shape[0] * g.shape[1]
    dw, magw = (da * t).sum((0, 1)), (mda * t.abs()).sum((0, 1))
    out["dw"] = (dw, U[dtype] * dw.abs() + (C32 * math.sqrt(n) + RSTD_C + 5) * U32 * magw + TINY[dtype])
    return out


# ------------------------------------------------------------------------------------------------ SwiGLU / GeGLU
def _sigmoid_of_minus(z, c_z):
    """s = 1 / (1 + exp(-z)) in float64, 1 - s without cancellation, and the relative fp32 error ds of the kernels' s (see the module
    docstring); c_z = fp32 operations that formed z."""
    s, s1 = torch.sigmoid(z), torch.sigmoid(-z)
    dE = ((1 + c_z) * z.abs() + 2) * U32
    return s, s1, EXP_C * (s1 * dE + 2 * U32), dE


def swiglu_ref(g, u, dy, dtype):
    """y = silu(g) u -> {"y", "dg", "du"}: (ref, bound); dy None: forward only."""
    x, u64 = _d(g), _d(u)
    s, s1, ds, _ = _sigmoid_of_minus(x, 0)
    floor = FLUSH * (1 + 4 * U[dtype])
    y = x * s * u64
    out = {"y": (y, _ku(2, dtype) * y.abs() + (ds + U32) * y.abs() + floor * (x * u64).abs() + TINY[dtype] * (1 + u64.abs()))}
    if dy is None:
        return out
    d = _d(dy)
    du = d * x * s
    out["du"] = (du, U[dtype] * du.abs() + (ds + 2 * U32) * du.abs() + floor * (d * x).abs() + TINY[dtype])
    f = 1 + x * s1
    dg = d * u64 * s * f
    # 1 - s by subtraction: absolute error s ds + u32 (1 - s); then x (1 - s) and 1 + x (1 - s), one rounding each
    df = x.abs() * (s * ds + U32 * s1) + U32 * (x * s1).abs() + U32 * f.abs()
    out["dg"] = (dg, U[dtype] * dg.abs() + (d * u64 * s).abs() * df + (ds + 2 * U32) * dg.abs()
                 + floor * (d * u64).abs() * (1 + x.abs()) + TINY[dtype])
    return out


def geglu_ref(g, u, dy, dtype):
    """y = gelu_tanh(g) u, 0.5 (1 + tanh z) = sigmoid(2 z) -> {"y", "dg", "du"}: (ref, bound); dy None: forward only."""
    x, u64 = _d(g), _d(u)
    z2 = 2 * K0 * x * (1 + K1 * x * x)
    s, s1, ds, dE = _sigmoid_of_minus(z2, 5)
    # the kernel's own s where the reference's is (next to) zero; the output roundings apply to it too
    # (and the fp32 error of exp(80) itself: dE at |z| = 80 is under 512 u32)
    floor = torch.maximum(torch.full_like(x, FLUSH), torch.where(z2 < -80.0, torch.full_like(x, CLAMP), torch.zeros_like(x))) * (1 + 4 * U[dtype] + 512 * U32)
    y = x * s * u64
    out = {"y": (y, _ku(2, dtype) * y.abs() + (ds + 2 * U32) * y.abs() + floor * (x * u64).abs() + TINY[dtype] * (1 + u64.abs()))}
    if dy is None:
        return out
    d = _d(dy)
    du = d * x * s
    out["du"] = (du, U[dtype] * du.abs() + (ds + 2 * U32) * du.abs() + floor * (d * x).abs() + TINY[dtype])
    P = 2 * K0 * (1 + 3 * K1 * x * x)
    t2 = x * s * s1 * P
    dgelu = s + t2
    ddgelu = s * ds + t2.abs() * (2 * ds + dE + 8 * U32) + U32 * dgelu.abs()
    dg = d * u64 * dgelu
    out["dg"] = (dg, U[dtype] * dg.abs() + (d * u64).abs() * ddgelu + 2 * U32 * dg.abs()
                 + floor * (d * u64).abs() * (1 + (x * P).abs()) + TINY[dtype])
    return out


# ------------------------------------------------------------------------------------------------ the check
def check(name, got, ref, bound, label=""):
    """Asserts |got - ref| <= bound for EVERY element (a non-finite `got` violates it).  On failure: how many elements violate it, the
    worst err / bound and the (row, column) of that element.  Returns the worst err / bound, also kept in WORST[(name, dtype)]."""
    g = _d(got)
    assert g.shape == ref.shape, f"{label} {name}: shape {tuple(g.shape)}, reference {tuple(ref.shape)}"
    err = (g - ref).abs()
    ratio = err / (bound + 1e-300)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    key = (name, str(got.dtype).split(".")[-1])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        cols = g.shape[-1] if g.dim() > 1 else g.numel()
        i = int(ratio.reshape(-1).argmax())
        row, col = divmod(i, cols)
        raise AssertionError(f"{label} {name} ({key[1]}): {int((~(ratio <= 1.0)).sum())} of {g.numel()} elements over the bound, worst "
                             f"err/bound {worst:.3g} at (row {row}, column {col}): got {float(g.reshape(-1)[i]):.9g}, reference "
                             f"{float(ref.reshape(-1)[i]):.9g}, bound {float(bound.expand_as(g).reshape(-1)[i]):.3e}")
    return worst


def check_all(prefix, got: dict, ref: dict, label=""):
    """check() of every tensor in `got` against ref[name] = (ref, bound) -> {name: worst err / bound}."""
    return {n: check(f"{prefix}.{n}", t, *ref[n], label=label) for n, t in got.items()}
