"""Float64 restatement of the LayerNorm kernels of csrc/elementwise_kernels.hip (dta_layernorm_fwd / _bwd: CohereLayerNorm without bias,
with the residual join of the parallel block) and a per-element error bound for every output, in the form of tests/rowops_ref64.py:

    bound = k u M  +  c u32 M_red  +  floor          (u, u32, k, c, M, M_red, floor as defined there)

The references take the kernels' ROUNDED inputs and eps as the float the entry point receives.  Notation: m = mean(x), c = x - m,
v = mean(c^2), r = rsqrt(v + eps), t = c r, g = dy w.

DERIVATION, by counting the operations of the kernels (one wave per row; a lane adds its 8 H / 512 .. 8 ceil(H / 512) elements in one
fp32 chain, then six shuffle additions):

    x_out   (x + delta_a) + delta_b in fp32, rounded once: k = 1 on |x_out|; the two fp32 additions: 2 u32 (|x| + |delta_a| + |delta_b|).
    mean    a sum of H terms, a multiplication by the float 1/H (itself rounded): dm = (C32 sqrt(H) + 3) u32 mean|x|.  (The longest chain a
            value passes is H / 64 + 14 additions, which is below C32 sqrt(H) + 3 for every H <= 8192: the statistical form is also a
            worst-case one here.)  The bound is on mean|x|, not |m|: on a centred row m is a cancelled sum.
    rstd    RSTD_C u32 r, RSTD_C = 10 from rowops_ref64: the same reduction tree over the squares of c.  Each c carries one fp32 rounding
            (a relative u32 on c, i.e. 2 u32 on its square - what the product x x of the RMSNorm sum of squares carries once), and the
            error dm of the mean enters the variance only at second order, because sum(c) = 0:
            mean((c - dm)^2) = v + dm^2.  That term is kept, not dropped: + r (r dm)^2 / 2.  On the offset row below (8 + 0.05 randn) it
            is under 1 u32; a one-pass variance E[x^2] - m^2 is off by 8.7e-4 there (test_layernorm_ref64.py).
    y       y = cast(w (c r)): ONE rounding, k = 1 on |y|.  fp32: the subtraction, two products and r: (RSTD_C + 3) u32 |y|; the mean's
            error moves every c by dm: |w| r dm (absolute - on an offset row this is the largest fp32 term); the second-order term of r.
            floor TINY (1 + |w|).
    dx      dx = r (g - mean(g) - t mean(g t)) + dres, k = 1.  M_red = r (|g| + mean|g| + |t| mean|g t|) (+ |dres|);
            c = C32 sqrt(H) (the two means; they share the bound of the larger) + 3 RSTD_C (r enters three times: in front, in t, in the
            t of the mean) + 10 (the subtraction and product of t twice, g, the two means' scalings, two subtractions, the outer product,
            the addition of dres).  The forward's mean, which the backward reads, moves t by r dm: r (r dm) (mean|g t| + |t| mean|g|).
    dw      fp32 sum over rows of dy t (per-workgroup partials, then dta_sum_slabs), rounded once: k = 1; M_red = sum_rows |dy t|,
            c = C32 sqrt(R) + RSTD_C + 4; the mean's error: sum_rows |dy| r dm.

The constants are not fitted to the kernel.  OBSERVED worst err / bound on the MI355X over tests/test_gpu_layernorm.py (from `check`;
bf16 / f16 / fp32 storage):
    layernorm (all forms, grid-stride)   y .992/.995/.67   x_out .996/.999/.66   dx .993/.985/.06   dw .987/.986/.09
                                         mean .04/.06/.20   rstd .85/.85/.88 (of its bound; .19 to .31 for H <= 120 and for the grid-stride rows)
The 2-byte figures sit at 0.99 for the reason given in rowops_ref64 (u is the exact worst case of ONE rounding).  mean stays far below
its bound because the bound is the worst case of the chain and the kernel's errors average out.  rstd reaches .77 / .85 / .88 of its
bound at H = 4096 / 8184 / 8192, where RMSNorm's rstd stays at .49 of RSTD_C - on ONE row, the single-element row under eps = 1e-6
(8.8 u32; every other row of those cases stays under 4.1 u32, the median at 0.5): centring turns it into H - 1 EQUAL values -x/H, and a
lane's chain that adds the same square 128 times rounds the same way at every step, in every lane - the errors the derivation lets
average out are correlated there.  Under RMSNorm that row is H - 1 zeros.  It is inside the bound that was derived before the run;
RSTD_C was not raised for it.  On the offset row itself rstd is off by 4e-8 to 1.9e-7 relative (H = 4096).
"""
import math

import torch

import rowops_ref64 as R
from ref64_common import C32, TINY, U, U32

RSTD_C = R.RSTD_C
OFFSET, SPREAD = 8.0, 0.05
check, check_all = R.check, R.check_all


def _d(t):
    return t.detach().double()


def offset_row_of(R_):
    """The row of rows() that carries the common offset (None: R = 1 has none)."""
    return None if R_ < 2 else (R_ // 2 - 1 if R_ >= 4 else 1)


def rows(R_, H, dtype, seed):
    """rowops_ref64.rows (log-spaced scales, the zero row, the single-element row) with one more special row: offset_row_of(R) is
    8 + 0.05 randn - a spread 160 times smaller than the mean, where a one-pass variance cancels."""
    x = R.rows(R_, H, dtype, seed).float()
    o = offset_row_of(R_)
    if o is not None:
        x[o] = OFFSET + SPREAD * torch.randn(H, generator=torch.Generator().manual_seed(seed + 7))
    return x.to(dtype)


def delta_for(x, seed):
    """rowops_ref64.delta_for, with the offset row's delta at its spread's scale, so that the row stays an offset row in the sum."""
    d = R.delta_for(x, seed).float()
    o = offset_row_of(x.shape[0])
    if o is not None:
        d[o] = 0.4 * SPREAD * torch.randn(x.shape[1], generator=torch.Generator().manual_seed(seed + 11))
    return d.to(x.dtype)


def join(x, delta_a, delta_b, dtype):
    """x_out as the kernel rounds it: (x + delta_a) + delta_b in fp32, then the storage type."""
    s = x.float()
    if delta_a is not None:
        s = s + delta_a.float()
    if delta_b is not None:
        s = s + delta_b.float()
    return s.to(dtype)


def _stats(x64, eps):
    H = x64.shape[-1]
    m = x64.mean(-1)
    c = x64 - m[:, None]
    r = torch.rsqrt(c.pow(2).mean(-1) + R._eps(eps))
    dm = (C32 * math.sqrt(H) + 3) * U32 * x64.abs().mean(-1)          # the bound of the mean
    rel2 = 0.5 * (r * dm).pow(2)                                      # second-order relative error of r from dm
    return m, c, r, dm, rel2


def layernorm_fwd_ref(x, delta_a, delta_b, w, eps, dtype, xin=None):
    """-> {"x_out" (with a delta), "mean", "rstd", "y"}: (ref, bound).  `xin`: the rounded stream the norm is taken of (the kernel's own
    x_out, once it passed its bound); default: join()."""
    out = {}
    if delta_a is not None:
        parts = [_d(t) for t in (x, delta_a, delta_b) if t is not None]
        xo, mag = sum(parts), sum(p.abs() for p in parts)
        out["x_out"] = (xo, U[dtype] * xo.abs() + 2 * U32 * mag + TINY[dtype])
        x = xin if xin is not None else join(x, delta_a, delta_b, dtype)
    x64, w64 = _d(x), _d(w)
    m, c, r, dm, rel2 = _stats(x64, eps)
    out["mean"] = (m, dm + 1e-38)
    out["rstd"] = (r, RSTD_C * U32 * r + rel2 * r)
    y = w64 * (c * r[:, None])
    out["y"] = (y, R._ku(1, dtype) * y.abs() + ((RSTD_C + 3) * U32 + rel2[:, None]) * y.abs() + w64.abs() * (r * dm)[:, None]
                + TINY[dtype] * (1 + w64.abs()))
    return out


def layernorm_bwd_ref(xin, w, dy, dres, eps, dtype):
    """-> {"dx", "dw"}: (ref, bound); xin = the normalised rows (the forward's x_out)."""
    x64, w64, d = _d(xin), _d(w), _d(dy)
    R_, H = x64.shape
    m, c, r, dm, rel2 = _stats(x64, eps)
    r, dtm, rel2 = r[:, None], (r * dm)[:, None], rel2[:, None]
    t, g = c * r, d * w64
    mg, mgt = g.mean(-1, keepdim=True), (g * t).mean(-1, keepdim=True)
    amg, amgt = g.abs().mean(-1, keepdim=True), (g * t).abs().mean(-1, keepdim=True)
    dx = r * (g - mg - t * mgt)
    mag = r * (g.abs() + amg + t.abs() * amgt)
    from_mean = r * dtm * (amgt + t.abs() * amg)
    if dres is not None:
        dx, mag = dx + _d(dres), mag + _d(dres).abs()
    out = {"dx": (dx, U[dtype] * dx.abs() + ((C32 * math.sqrt(H) + 3 * RSTD_C + 10) * U32 + 3 * rel2) * mag + from_mean + TINY[dtype])}
    dw, magw = (d * t).sum(0), (d * t).abs().sum(0)
    out["dw"] = (dw, U[dtype] * dw.abs() + (C32 * math.sqrt(R_) + RSTD_C + 4) * U32 * magw + (rel2 * (d * t).abs()).sum(0)
                 + (d.abs() * dtm).sum(0) + TINY[dtype])
    return out
