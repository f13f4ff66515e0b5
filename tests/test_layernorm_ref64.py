"""tests/layernorm_ref64.py on the CPU: its references are torch's own autograd in float64 of CohereLayerNorm's formula, an fp32
emulation of the kernels' arithmetic stays inside every bound for bf16 / f16 / fp32 storage, and the rstd bound has teeth: the
one-pass variance E[x^2] - m^2 in fp32 exceeds it on the offset row."""
import itertools

import pytest
import torch

import layernorm_ref64 as L

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
EPS = 1e-5


def emu_fwd(x, da, db, w, eps, dtype, one_pass=False):
    """The forward kernel's arithmetic in fp32: the join rounded once, the mean, the CENTRED variance (one_pass: E[x^2] - m^2 instead),
    y = cast(w ((x - m) r))."""
    xo = L.join(x, da, db, dtype)
    xf = xo.float()
    H = xf.shape[-1]
    m = xf.sum(-1) * torch.tensor(1.0 / H, dtype=F32)
    if one_pass:
        v = (xf * xf).sum(-1) * torch.tensor(1.0 / H, dtype=F32) - m * m
    else:
        c = xf - m[:, None]
        v = (c * c).sum(-1) * torch.tensor(1.0 / H, dtype=F32)
    r = torch.rsqrt(v + torch.tensor(eps, dtype=F32))
    y = (w.float() * ((xf - m[:, None]) * r[:, None])).to(dtype)
    return xo, y, m, r


def emu_bwd(xin, w, dy, dres, m, r, dtype):
    xf, g = xin.float(), dy.float() * w.float()
    H = xf.shape[-1]
    t = (xf - m[:, None]) * r[:, None]
    inv = torch.tensor(1.0 / H, dtype=F32)
    mg, mgt = g.sum(-1, keepdim=True) * inv, (g * t).sum(-1, keepdim=True) * inv
    dx = r[:, None] * ((g - mg) - t * mgt)
    if dres is not None:
        dx = dx + dres.float()
    return dx.to(dtype), (dy.float() * t).sum(0).to(dtype)


def _inputs(R_, H, dtype, n_delta, seed=0):
    x = L.rows(R_, H, dtype, R_ + H + seed)
    da = L.delta_for(x, H + 1) if n_delta >= 1 else None
    db = L.delta_for(x, H + 5) if n_delta >= 2 else None
    w = L.R.norm_weight(H, dtype, H, False)
    return x, da, db, w, L.R.randn((R_, H), dtype, H + 2), L.R.randn((R_, H), dtype, H + 3)


@pytest.mark.parametrize("n_delta", [0, 1, 2])
def test_references_are_float64_autograd(n_delta):
    x, da, db, w, dy, dres = (None if t is None else t.double().requires_grad_(True) for t in _inputs(6, 72, F32, n_delta))
    xo = x + (da if da is not None else 0) + (db if db is not None else 0)
    m = xo.mean(-1, keepdim=True)
    y = w * ((xo - m) * torch.rsqrt((xo - m).pow(2).mean(-1, keepdim=True) + L.R._eps(EPS)))
    leaves = [t for t in (x, da, db, w) if t is not None]
    grads = torch.autograd.grad([xo, y], leaves, [dres.detach(), dy.detach()])
    fwd = L.layernorm_fwd_ref(x, da, db, w, EPS, F32, xin=xo.detach())
    bwd = L.layernorm_bwd_ref(xo.detach(), w, dy, dres, EPS, F32)
    assert float((fwd["y"][0] - y.detach()).abs().max()) < 1e-12
    assert float((fwd["mean"][0] - m.detach()[:, 0]).abs().max()) < 1e-14
    if n_delta:
        assert float((fwd["x_out"][0] - xo.detach()).abs().max()) < 1e-14
    for gx in grads[:-1]:                                     # x and both deltas get the one dx
        assert float((bwd["dx"][0] - gx).abs().max()) < 1e-12
    assert float((bwd["dw"][0] - grads[-1]).abs().max()) < 1e-11


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R_,H", [(1, 8), (3, 64), (4, 120), (3, 1024), (5, 1032), (4, 2048), (3, 2056), (65, 4096), (5, 4104),
                                         (7, 8184), (5, 8192)])
def test_emulation_stays_inside_every_bound(R_, H, dtype):
    for n_delta, with_dres in itertools.product((0, 1, 2), (False, True)):
        x, da, db, w, dy, dres = _inputs(R_, H, dtype, n_delta)
        dres = dres if with_dres else None
        xo, y, m, r = emu_fwd(x, da, db, w, EPS, dtype)
        label = f"R={R_} H={H} deltas={n_delta}"
        if n_delta:
            L.check_all("emu_layernorm", {"x_out": xo}, L.layernorm_fwd_ref(x, da, db, w, EPS, dtype), label)
        L.check_all("emu_layernorm", {"y": y, "mean": m, "rstd": r}, L.layernorm_fwd_ref(x, da, db, w, EPS, dtype, xin=xo), label)
        dx, dw = emu_bwd(xo, w, dy, dres, m, r, dtype)
        L.check_all("emu_layernorm", {"dx": dx, "dw": dw}, L.layernorm_bwd_ref(xo, w, dy, dres, EPS, dtype), label)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_pass_variance_exceeds_the_rstd_bound_on_the_offset_row(dtype):
    R_, H = 6, 4096
    x, _, _, w, _, _ = _inputs(R_, H, dtype, 0)
    o = L.offset_row_of(R_)
    ref, bound = L.layernorm_fwd_ref(x, None, None, w, EPS, dtype)["rstd"]
    two = emu_fwd(x, None, None, w, EPS, dtype)[3].double()
    one = emu_fwd(x, None, None, w, EPS, dtype, one_pass=True)[3].double()
    assert float((two[o] - ref[o]).abs() / bound[o]) <= 1.0
    ratio = float((one[o] - ref[o]).abs() / bound[o])
    print(f"one-pass rstd on the offset row ({dtype}): {float((one[o] - ref[o]).abs() / ref[o]):.2e} relative, {ratio:.0f} x the bound")
    assert ratio > 10.0
    with pytest.raises(AssertionError, match="over the bound"):
        L.check("rstd", one.float(), ref, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_corruptions_are_rejected(dtype):
    """A norm without the mean subtraction, a dx without the mean(g) term and a y rounded twice are outside the bounds."""
    x, _, _, w, dy, _ = _inputs(6, 120, dtype, 0)
    xo, y, m, r = emu_fwd(x, None, None, w, EPS, dtype)
    fwd, bwd = L.layernorm_fwd_ref(x, None, None, w, EPS, dtype), L.layernorm_bwd_ref(x, w, dy, None, EPS, dtype)
    xf = x.float()
    rms = (w.float() * (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + EPS))).to(dtype)
    with pytest.raises(AssertionError, match="over the bound"):
        L.check("y", rms, *fwd["y"])
    t = (xf - m[:, None]) * r[:, None]
    g = dy.float() * w.float()
    no_mean = (r[:, None] * (g - t * (g * t).mean(-1, keepdim=True))).to(dtype)
    with pytest.raises(AssertionError, match="over the bound"):
        L.check("dx", no_mean, *bwd["dx"])
    if dtype != F32:
        twice = (w.float() * t.to(dtype).float()).to(dtype)
        with pytest.raises(AssertionError, match="over the bound"):
            L.check("y", twice, *fwd["y"])
