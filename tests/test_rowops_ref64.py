"""CPU checks of the float64 row-kernel references and their per-element bounds (tests/rowops_ref64.py), on the input generators the GPU
tests use: a torch fp32 emulation of each kernel's documented arithmetic (storage roundings where the kernel has them) stays inside
every bound, each of six named corruptions of that emulation is rejected, and the references agree with hostmirror's fp32 restatement
(and with float64 autograd, for the forms hostmirror does not have), so the restatements cannot drift apart."""
import math

import pytest
import torch

import hostmirror
import rowops_ref64 as R
from dynamictreeattn_amd import ops

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
K0f, K1f = 0.7978845608028654, 0.044715


# ------------------------------------------------------------------------------------------------ fp32 emulations of the kernels
def emu_rmsnorm_fwd(x, delta, w, eps, off, dtype, eps_of_row=None):
    """(x_out | None, y, rstd); eps_of_row: a per-row eps [R] in place of eps (a corruption)."""
    xf, xo = x.float(), None
    if delta is not None:
        xo = (xf + delta.float()).to(dtype); xf = xo.float()
    e = torch.full((xf.shape[0],), eps, dtype=F32) if eps_of_row is None else eps_of_row.float()
    r = torch.rsqrt((xf * xf).sum(-1) / xf.shape[1] + e)
    if off:
        y = (xf * r[:, None] * (torch.tensor(off, dtype=F32) + w.float())).to(dtype)
    else:
        y = (w.float() * (xf * r[:, None]).to(dtype).float()).to(dtype)
    return xo, y, r


def emu_rmsnorm_bwd(xin, w, dy, dres, rstd, off, dtype, no_projection_row=None, dw_skip=None):
    """(dx, dw); no_projection_row: that row of dx without the t^ mean(dt t^) term; dw_skip = (column, rows): dw of that column without
    those rows (corruptions)."""
    xf, g, r = xin.float(), dy.float(), rstd[:, None]
    wf = (torch.tensor(off, dtype=F32) + w.float()) if off else w.float()
    t = xf * r
    dot = (g * wf * t).sum(-1, keepdim=True) / xf.shape[1]
    if no_projection_row is not None:
        dot = dot.clone(); dot[no_projection_row] = 0.0
    dx = r * (g * wf - t * dot)
    if dres is not None:
        dx = dx + dres.float()
    gt = g * t
    if dw_skip is not None:
        gt = gt.clone(); gt[dw_skip[1], dw_skip[0]] = 0.0
    return dx.to(dtype), gt.sum(0).to(dtype)


def _cs_wide(cs, D):
    c, s = cs[:, :D // 2], cs[:, D // 2:]
    return torch.cat([c, c], -1)[:, None, :], torch.cat([s, s], -1)[:, None, :]


def emu_qk_fwd(x, w, cs, eps, dtype):
    xf = x.float()
    D = xf.shape[-1]
    cos, sin = _cs_wide(cs, D)
    r = None
    if w is not None:
        r = torch.rsqrt((xf * xf).sum(-1) * (1.0 / D) + eps)
        xf = (w.float() * (xf * r[..., None]).to(dtype).float()).to(dtype).float()
    b = torch.cat([-xf[..., D // 2:], xf[..., :D // 2]], -1)
    return (xf * cos + b * sin).to(dtype), r


def emu_qk_bwd(x, w, cs, dy, rstd, dtype):
    g = dy.float()
    D = g.shape[-1]
    cos, sin = _cs_wide(cs, D)
    da = g * cos + torch.cat([g[..., D // 2:], -g[..., :D // 2]], -1) * sin
    if w is None:
        return da.to(dtype), None
    r = rstd[..., None]
    t = x.float() * r
    dot = (da * w.float() * t).sum(-1, keepdim=True) * (1.0 / D)
    return (r * (da * w.float() - t * dot)).to(dtype), (da * t).sum((0, 1)).to(dtype)


def emu_swiglu(g, u, dy, dtype, dg_plain_col=None):
    x, uf, d = g.float(), u.float(), dy.float()
    E = torch.exp(-x)
    y = ((x / (1 + E)).to(dtype).float() * uf).to(dtype)
    sg = 1 / (1 + E)
    inner = 1 + x * (1 - sg)
    if dg_plain_col is not None:
        inner = inner.clone(); inner[:, dg_plain_col] = 1.0
    return y, (d * uf * sg * inner).to(dtype), (d * x * sg).to(dtype)


def emu_geglu(g, u, dy, dtype):
    x, uf, d = g.float(), u.float(), dy.float()
    x2 = x * x
    z2 = 2 * K0f * x * (K1f * x2 + 1)
    E = torch.exp(torch.clamp(-z2, max=80.0))
    s = 1 / (1 + E)
    ge = x * s
    dgelu = s + x * s * (E * s) * (2 * K0f * (3 * K1f * x2 + 1))
    return (ge.to(dtype).float() * uf).to(dtype), (d * uf * dgelu).to(dtype), (d * ge).to(dtype)


def _rejected(name, got, ref):
    with pytest.raises(AssertionError, match="over the bound"):
        R.check(name, got, *ref)


# ------------------------------------------------------------------------------------------------ RMSNorm
RMS_SHAPES = [(1, 8), (3, 72), (6, 1024), (6, 1032), (6, 4104), (3, 8192), (8197, 64)]


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("R_,H", RMS_SHAPES)
def test_rmsnorm_emulation_stays_inside_every_bound(R_, H, dtype):
    for i, (off, has_delta) in enumerate([(0.0, False), (0.0, True), (1.0, False), (1.0, True)]):
        eps = (1e-6, 1e-5)[i % 2]
        x, w = R.rows(R_, H, dtype, R_ + H), R.norm_weight(H, dtype, H, bool(off))
        delta = R.delta_for(x, H + 1) if has_delta else None
        dy, dres = R.randn((R_, H), dtype, H + 2), (R.randn((R_, H), dtype, H + 3) if has_delta else None)
        xo, y, rstd = emu_rmsnorm_fwd(x, delta, w, eps, off, dtype)
        xin = xo if has_delta else x
        ref = R.rmsnorm_fwd_ref(x, delta, w, eps, off, dtype, xin=xin)
        R.check_all("emu_rmsnorm", {"y": y, "rstd": rstd, **({"x_out": xo} if has_delta else {})}, ref)
        dx, dw = emu_rmsnorm_bwd(xin, w, dy, dres, rstd, off, dtype)
        R.check_all("emu_rmsnorm", {"dx": dx, "dw": dw}, R.rmsnorm_bwd_ref(xin, w, dy, dres, eps, off, dtype))


@pytest.mark.parametrize("dtype", [BF, F16])
def test_rmsnorm_corruptions_are_rejected(dtype):
    R_, H, eps = 6, 1024, 1e-6
    x, w, dy = R.rows(R_, H, dtype, 1), R.norm_weight(H, dtype, 2, False), R.randn((R_, H), dtype, 3)
    _, y, rstd = emu_rmsnorm_fwd(x, None, w, eps, 0.0, dtype)
    fwd, bwd = R.rmsnorm_fwd_ref(x, None, w, eps, 0.0, dtype), R.rmsnorm_bwd_ref(x, w, dy, None, eps, 0.0, dtype)
    R.check("y", y, *fwd["y"])
    # one row of y x 1.02
    bad = y.clone(); bad[1] = (y[1].float() * 1.02).to(dtype)
    _rejected("y", bad, fwd["y"])
    # one row of dx without the projection term
    dx, dw = emu_rmsnorm_bwd(x, w, dy, None, rstd, 0.0, dtype)
    R.check("dx", dx, *bwd["dx"])
    _rejected("dx", emu_rmsnorm_bwd(x, w, dy, None, rstd, 0.0, dtype, no_projection_row=1)[0], bwd["dx"])
    # eps doubled on the rows where it matters (mean(x^2) < 100 eps): y, rstd and dx all notice
    ms = x.float().pow(2).mean(-1)
    sens = ms < 100 * eps
    assert bool(sens.any()) and not bool(sens.all())
    _, y2, r2 = emu_rmsnorm_fwd(x, None, w, eps, 0.0, dtype, eps_of_row=torch.where(sens, 2 * eps, eps))
    _rejected("y", y2, fwd["y"])
    _rejected("rstd", r2, fwd["rstd"])
    _rejected("dx", emu_rmsnorm_bwd(x, w, dy, None, r2, 0.0, dtype)[0], bwd["dx"])


@pytest.mark.parametrize("dtype", [BF, F16])
def test_a_dw_column_missing_one_grid_stride_pass_is_rejected(dtype):
    """R = 8197 at 4 rows x 2048 workgroups: rows 8192.. belong to the second pass of workgroups 0 and 1."""
    R_, H, eps = 8197, 64, 1e-6
    x, w, dy = R.rows(R_, H, dtype, 4), R.norm_weight(H, dtype, 5, False), R.randn((R_, H), dtype, 6)
    rstd = emu_rmsnorm_fwd(x, None, w, eps, 0.0, dtype)[2]
    ref = R.rmsnorm_bwd_ref(x, w, dy, None, eps, 0.0, dtype)["dw"]
    R.check("dw", emu_rmsnorm_bwd(x, w, dy, None, rstd, 0.0, dtype)[1], *ref)
    _rejected("dw", emu_rmsnorm_bwd(x, w, dy, None, rstd, 0.0, dtype, dw_skip=(7, slice(8192, R_)))[1], ref)


# ------------------------------------------------------------------------------------------------ head-norm + RoPE
def _qk_case(T, NH, D, dtype, norm, seed):
    x = R.rows(T * NH, D, dtype, seed).view(T, NH, D)
    w = R.norm_weight(D, dtype, seed + 1, False) if norm else None
    depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(seed + 2))
    return x, w, ops.rope_cos_sin(depth, D, 1e6), R.randn((T, NH, D), dtype, seed + 3)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("T,NH,D,norm", [(1, 1, 64, True), (5, 3, 128, True), (33, 4, 64, True), (33, 12, 128, True), (5, 4, 128, False),
                                         (33, 3, 64, False), (5462, 3, 128, True)])
def test_qk_norm_rope_emulation_stays_inside_every_bound(T, NH, D, norm, dtype):
    for eps in (1e-6, 1e-5):
        x, w, cs, dy = _qk_case(T, NH, D, dtype, norm, T + NH + D)
        y, rstd = emu_qk_fwd(x, w, cs, eps, dtype)
        R.check_all("emu_qk", {"y": y, **({"rstd": rstd.reshape(-1)} if norm else {})}, R.qk_fwd_ref(x, w, cs, eps, dtype))
        dx, dw = emu_qk_bwd(x, w, cs, dy, rstd, dtype)
        R.check_all("emu_qk", {"dx": dx, **({"dw": dw} if norm else {})}, R.qk_bwd_ref(x, w, cs, dy, eps, dtype))


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("norm", [True, False])
def test_a_head_rotated_with_its_neighbour_tokens_table_is_rejected(norm, dtype):
    T, NH, D = 5, 3, 128
    x, w, cs, dy = _qk_case(T, NH, D, dtype, norm, 11)
    y, _ = emu_qk_fwd(x, w, cs, 1e-6, dtype)
    ref = R.qk_fwd_ref(x, w, cs, 1e-6, dtype)["y"]
    R.check("y", y, *ref)
    bad = y.clone(); bad[0, 1] = emu_qk_fwd(x, w, cs.roll(-1, 0), 1e-6, dtype)[0][0, 1]          # token 0, head 1: token 1's cos / sin
    _rejected("y", bad, ref)


# ------------------------------------------------------------------------------------------------ SwiGLU / GeGLU
@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("rows,C", [(1, 8), (5, 72), (37, 1000)])
def test_glu_emulations_stay_inside_every_bound(rows, C, dtype):
    g, u, dy = R.rows(rows, C, dtype, rows + C), R.randn((rows, C), dtype, C), R.randn((rows, C), dtype, C + 1)
    for emu, ref in ((emu_swiglu, R.swiglu_ref), (emu_geglu, R.geglu_ref)):
        y, dg, du = emu(g, u, dy, dtype)
        R.check_all(emu.__name__, {"y": y, "dg": dg, "du": du}, ref(g, u, dy, dtype))


def test_swiglu_emulation_over_the_gate_range_f16():
    g = R.gate_range(F16)
    u, dy = (R.randn(g.shape, F32, s).clamp(-1, 1).to(F16) for s in (1, 2))
    y, dg, du = emu_swiglu(g, u, dy, F16)
    R.check_all("emu_swiglu_range", {"y": y, "dg": dg, "du": du}, R.swiglu_ref(g, u, dy, F16))


@pytest.mark.parametrize("dtype", [BF, F16])
def test_swiglu_dg_without_its_second_term_on_one_column_is_rejected(dtype):
    g, u, dy = R.rows(37, 1000, dtype, 1), R.randn((37, 1000), dtype, 2), R.randn((37, 1000), dtype, 3)
    ref = R.swiglu_ref(g, u, dy, dtype)["dg"]
    R.check("dg", emu_swiglu(g, u, dy, dtype)[1], *ref)
    _rejected("dg", emu_swiglu(g, u, dy, dtype, dg_plain_col=5)[1], ref)


# ------------------------------------------------------------------------------------------------ the two restatements agree
def _close(a, b, tol):
    a, b = a.detach().double(), b.detach().double()
    assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-30), float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def test_references_agree_with_hostmirror_through_autograd():
    """fp32 inputs, rows at scale 1 .. 1e-2 (hostmirror computes in fp32: 1e-5 relative to each tensor's largest element)."""
    Rr, H, eps = 6, 72, 1e-6
    x, w = R.rows(Rr, H, F32, 1, scale_hi=1.0), R.norm_weight(H, F32, 2, False)
    delta, dy, dres = R.delta_for(x, 3), R.randn((Rr, H), F32, 4), R.randn((Rr, H), F32, 5)
    xa, da, wa = (t.clone().requires_grad_(True) for t in (x, delta, w))
    xo, y = hostmirror._cpu_add_rms_norm(xa, da, wa, eps)
    torch.autograd.backward([xo, y], [dres, dy])
    fwd = R.rmsnorm_fwd_ref(x, delta, w, eps, 0.0, F32)
    bwd = R.rmsnorm_bwd_ref(x + delta, w, dy, dres, eps, 0.0, F32)
    for a, b in ((xo, fwd["x_out"][0]), (y, fwd["y"][0]), (xa.grad, bwd["dx"][0]), (da.grad, bwd["dx"][0]), (wa.grad, bwd["dw"][0])):
        _close(a, b, 1e-5)
    T, Hq, Hkv, D = 5, 3, 1, 64
    qkv = R.rows(T * (Hq + 2 * Hkv), D, F32, 6, scale_hi=1.0).view(T, Hq + 2 * Hkv, D)
    wq, wk = R.norm_weight(D, F32, 7, False), R.norm_weight(D, F32, 8, False)
    cs = ops.rope_cos_sin(torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(9)), D, 1e6)
    grads = R.randn(qkv.shape, F32, 10)
    a, wqa, wka = (t.clone().requires_grad_(True) for t in (qkv, wq, wk))
    q, k, v = hostmirror._cpu_qkv_prep(a, wqa, wka, cs, eps, Hq, Hkv)
    torch.autograd.backward([q, k, v], [grads[:, :Hq], grads[:, Hq:Hq + Hkv], grads[:, Hq + Hkv:]])
    for lo, NH, wt, wg, out in ((0, Hq, wq, wqa.grad, q), (Hq, Hkv, wk, wka.grad, k)):
        xs, gs = qkv[:, lo:lo + NH], grads[:, lo:lo + NH]
        _close(out, R.qk_fwd_ref(xs, wt, cs, eps, F32)["y"][0], 1e-5)
        b = R.qk_bwd_ref(xs, wt, cs, gs, eps, F32)
        _close(a.grad[:, lo:lo + NH], b["dx"][0], 1e-5); _close(wg, b["dw"][0], 1e-5)
    x1 = qkv[:, :Hq].clone().requires_grad_(True)
    y1 = hostmirror._cpu_qk_norm_rope(x1, None, cs, eps); y1.backward(grads[:, :Hq])
    _close(y1, R.qk_fwd_ref(qkv[:, :Hq], None, cs, eps, F32)["y"][0], 1e-5)
    _close(x1.grad, R.qk_bwd_ref(qkv[:, :Hq], None, cs, grads[:, :Hq], eps, F32)["dx"][0], 1e-5)
    g, u, d = R.rows(5, 72, F32, 11), R.randn((5, 72), F32, 12), R.randn((5, 72), F32, 13)
    ga, ua = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    ys = hostmirror._cpu_swiglu(ga, ua); ys.backward(d)
    ref = R.swiglu_ref(g, u, d, F32)
    _close(ys, ref["y"][0], 1e-5); _close(ga.grad, ref["dg"][0], 1e-5); _close(ua.grad, ref["du"][0], 1e-5)


def test_offset_norm_and_geglu_references_agree_with_float64_autograd():
    """The forms hostmirror does not restate: the hand-written float64 gradients against autograd's, to 1e-12."""
    Rr, H, eps = 6, 72, float(torch.tensor(1e-5, dtype=F32))
    x, w = R.rows(Rr, H, F32, 1, scale_hi=1.0).double(), R.norm_weight(H, F32, 2, True).double()
    dy, dres = R.randn((Rr, H), F32, 4).double(), R.randn((Rr, H), F32, 5).double()
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = xa * torch.rsqrt(xa.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + wa)
    torch.autograd.backward([xa * 1.0, y], [dres, dy])
    bwd = R.rmsnorm_bwd_ref(x, w, dy, dres, eps, 1.0, F32)
    _close(y, R.rmsnorm_fwd_ref(x, None, w, eps, 1.0, F32)["y"][0], 1e-12)
    _close(xa.grad, bwd["dx"][0], 1e-12); _close(wa.grad, bwd["dw"][0], 1e-12)
    g, u, d = R.rows(5, 72, F32, 11).double(), R.randn((5, 72), F32, 12).double(), R.randn((5, 72), F32, 13).double()
    ga, ua = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
    z = math.sqrt(2.0 / math.pi) * (ga + R.K1 * ga ** 3)
    yg = 0.5 * ga * (1 + torch.tanh(z)) * ua; yg.backward(d)
    ref = R.geglu_ref(g, u, d, F32)
    _close(yg, ref["y"][0], 1e-12); _close(ga.grad, ref["dg"][0], 1e-12); _close(ua.grad, ref["du"][0], 1e-12)
