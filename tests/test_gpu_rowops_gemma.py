"""GPU parity of the Gemma-2 row kernels against float64: GeGLU (dta_geglu_fwd / _bwd), RMSNorm with weight offset 1
(dta_rmsnorm_fwd / _bwd with w_offset, with and without the fused residual add) and the final-logit soft-capped log-prob / entropy kernels
(dta_logprob_entropy_fwd / _shard_stats / _bwd with softcap: fork picks, temperature 0.7, labels outside [0, V), V = 256 and 256 000,
shard statistics over two halves of V combined on the host).

Tolerances are those of the uncapped forms: the value / gradient comparison of tests/test_gpu_rowops.py (its `_pair` and `_rel`,
imported: relative Frobenius error 8e-3 bf16 / 2e-3 f16, weight gradients 1e-2) and the figures tests/test_gpu_logprob.py applies in
test_kernels_vs_oracle (it states them inline, so they are named once below).  softcap <= 0 and w_offset = 0 passed to the entries
must give the bits of the operators' defaults."""
import math

import pytest
import torch

from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib, ptr
from test_gpu_logprob import _csr
from test_gpu_rowops import _pair, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# tests/test_gpu_logprob.py::test_kernels_vs_oracle: |d| <= LP_TOL (1 + |ref|) on log-probs, ENT_TOL on entropies, relative gradient error
LP_TOL, ENT_TOL, GRAD_TOL = 2e-5, 5e-5, {BF: 1e-2, F16: 2e-3, F32: 2e-5}


def _f64(fn):
    """A float64 reference behind the fp32 interface of test_gpu_rowops._pair (inputs arrive as the rounded values in fp32)."""
    return lambda *xs: fn(*(x.double() for x in xs)).float()


# ------------------------------------------------------------------------------------------------ GeGLU
def _geglu64(g, u):
    return torch.nn.functional.gelu(g, approximate="tanh") * u


@pytest.mark.parametrize("rows,C,dtype", [(1, 8, BF), (37, 64, BF), (130, 1000, F16), (9, 36864, BF), (33, 72, F32)])
def test_geglu(rows, C, dtype):
    g = torch.Generator().manual_seed(rows + C)
    gate = torch.empty(rows, C).uniform_(-8.0, 8.0, generator=g)            # gates span +-8 ...
    gate.view(-1)[::5] = 0.0                                                # ... and include 0
    gate.view(-1)[1::97] = 8.0; gate.view(-1)[2::97] = -8.0
    up = torch.randn(rows, C, generator=g)
    _pair(ops.geglu, _f64(_geglu64), [gate, up], dtype)
    _pair(lambda gu: ops.geglu_fused(gu), _f64(lambda gu: _geglu64(gu[:, :C], gu[:, C:])), [torch.cat([gate, up], dim=1)], dtype)


def test_geglu_values_in_fp32_over_the_gate_range():
    """fp32 storage: the kernel's own arithmetic (sigmoid form of 0.5 (1 + tanh)) against float64, element by element, over +-8 and 0;
    the derivative too.  No NaN at either end of the range (and far beyond it)."""
    gate = torch.cat([torch.linspace(-8, 8, 4097), torch.tensor([0.0, -30.0, 30.0, -1e4, 1e4, 0.0, 0.0])]).view(1, -1).contiguous()      # 4104 columns
    up = torch.full_like(gate, 1.5)
    ga, ua = gate.to(DEV).requires_grad_(True), up.to(DEV).requires_grad_(True)
    y = ops.geglu(ga, ua)
    y.backward(torch.ones_like(y))
    g64, u64 = gate.double().requires_grad_(True), up.double().requires_grad_(True)
    y64 = _geglu64(g64, u64); y64.backward(torch.ones_like(y64))
    for got, want in ((y, y64), (ga.grad, g64.grad), (ua.grad, u64.grad)):
        got, want = got.detach().double().cpu(), want.detach()
        assert bool(torch.isfinite(got).all())
        assert bool(((got - want).abs() <= 4e-6 * (1 + want.abs())).all())      # element by element: __expf and the fp32 products, a few 1e-7 relative


# ------------------------------------------------------------------------------------------------ RMSNorm with offset
def _norm64(x, w, eps=1e-6, off=1.0):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (off + w)


@pytest.mark.parametrize("R,H,dtype", [(1, 8, BF), (37, 64, BF), (33, 1000, F16), (301, 4608, BF), (40, 2048, F16), (17, 8192, BF), (21, 72, F32)])
def test_rmsnorm_offset(R, H, dtype):
    g = torch.Generator().manual_seed(R + H)
    x = torch.randn(R, H, generator=g) * 2
    w = 0.1 * torch.randn(H, generator=g)                        # Gemma's weights sit around 0: 1 + w formed in bf16 would lose their low bits
    _pair(lambda a, b: ops.rms_norm(a, b, 1e-6, 1.0), _f64(_norm64), [x, w], dtype)
    d = torch.randn(R, H, generator=g)

    def fused(a, dl, b):
        xo, y = ops.add_rms_norm(a, dl, b, 1e-6, 1.0)
        return y + 0.5 * xo

    def fused64(a, dl, b):
        xo = (a + dl).to(dtype).double()                        # the residual stream is rounded to the storage type, then normalised
        return _norm64(xo, b) + 0.5 * xo
    _pair(fused, _f64(fused64), [x, d, w], dtype)


def test_rmsnorm_offset_keeps_the_low_bits_of_w():
    """bf16: y against float64 from the bf16 inputs is within HALF a bf16 ulp everywhere (one rounding); forming 1 + w in bf16 first
    is visibly worse on the same inputs."""
    g = torch.Generator().manual_seed(3)
    R, H = 64, 4608
    x = (torch.randn(R, H, generator=g) * 2).to(BF); w = (0.1 * torch.randn(H, generator=g)).to(BF)
    y = ops.rms_norm(x.to(DEV), w.to(DEV), 1e-6, 1.0).double().cpu()
    want = _norm64(x.double(), w.double())
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 7)
    assert float(((y - want).abs() / ulp).max()) <= 0.5 + 1e-3          # (+ the fp32 error of the kernel's own arithmetic)
    lossy = _norm64(x.double(), (1.0 + w.float()).to(BF).double(), off=0.0)
    assert float(((lossy - want).abs() / ulp).max()) > 0.5


@pytest.mark.parametrize("dtype", [BF, F32])
def test_zero_offset_is_the_plain_entry_bitwise(dtype):
    g = torch.Generator().manual_seed(5)
    R, H = 37, 4608
    x, d, dy = (torch.randn(R, H, generator=g).to(dtype).to(DEV) for _ in range(3))
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(dtype).to(DEV)
    xo, y, rstd = torch.empty_like(x), torch.empty_like(x), torch.empty(R, device=DEV)
    assert lib().dta_rmsnorm_fwd(ptr(x), ptr(d), ptr(w), ptr(xo), ptr(y), ptr(rstd), R, H, 1e-6, 0.0, ops._DT[dtype], None) == 0
    dx = torch.empty_like(x); part = torch.empty(lib().dta_rmsnorm_bwd_blocks(R), H, device=DEV)
    assert lib().dta_rmsnorm_bwd(ptr(xo), ptr(w), ptr(dy), ptr(d), ptr(rstd), ptr(dx), ptr(part), R, H, 0.0, ops._DT[dtype], None) == 0
    torch.cuda.synchronize()
    outs = [(xo, y, rstd, dx, ops.sum_slabs(part, dtype))]           # the operator returns the dw partials summed (one fixed-order launch)
    for off in ((), (0.0,)):                                         # ops.add_rms_norm without an offset and with an explicit 0.0
        xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        xo, y = ops.add_rms_norm(xa, d, wa, 1e-6, *off)
        rstd = y.grad_fn.saved_tensors[2]
        dx, dw = torch.autograd.grad([xo, y], [xa, wa], [d, dy])     # the gradient on the residual stream is the entry's dres
        outs.append((xo.detach(), y.detach(), rstd, dx, dw))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ capped log-prob / entropy
def _cap64(x, c):
    return c * torch.tanh(x / c)


def _lp_case(R, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(R, V, generator=g) * 3).to(dtype)
    labels = torch.randint(0, V, (R,), generator=g)
    labels[0] = -1                                                              # labels outside [0, V): log-prob 0, no gradient
    if R > 2:
        labels[2] = V + 5
    ex_rows = torch.sort(torch.randint(0, R, (min(R, 7),), generator=g)).values          # rows may repeat: a node with several fork children
    ex_lab = (labels[ex_rows].clamp(0, V - 1) + 1 + torch.arange(ex_rows.numel())) % V
    glp, gent = (torch.randn(R, generator=g) for _ in range(2))
    gex = torch.randn(ex_rows.numel(), generator=g)
    return logits, labels, ex_rows, ex_lab, glp, gent, gex


def _ref64(logits, labels, ex_rows, ex_lab, glp, gent, gex, temp, cap):
    V = logits.shape[1]
    x = logits.double().requires_grad_(True)
    xc = _cap64(x, cap) / temp
    lse = torch.logsumexp(xc, -1)
    lp_all = xc - lse[:, None]
    ok = (labels >= 0) & (labels < V)
    picked = xc.gather(-1, labels.clamp(0, V - 1)[:, None]).squeeze(-1) * ok
    lp = (picked - lse) * ok                                  # forward: a label outside [0, V) yields 0
    ent = -(lp_all.exp() * lp_all).sum(-1)
    lp2 = lp_all[ex_rows, ex_lab]
    # backward: a label outside [0, V) is somebody else's (the vocabulary-sharded use: -1 = owned by another rank), so the row's
    # g_logprob still acts through -lse and only the pick's one-hot term is absent - the kernels' contract (dta.h), stated here
    (((picked - lse) * glp.double()).sum() + (lp2 * gex.double()).sum() + (ent * gent.double()).sum()).backward()
    return lp.detach(), ent.detach(), lp2.detach(), x.grad


@pytest.mark.parametrize("R,V,temp,dtype", [(37, 256, 0.7, BF), (16, 256, 1.0, F16), (11, 256, 0.7, F32), (9, 301, 0.7, BF),
                                            (5, 256000, 0.7, BF), (3, 256000, 1.0, F32)])
@pytest.mark.parametrize("cap", [3.0, 30.0])
def test_capped_logprob_kernels_vs_float64(R, V, temp, dtype, cap):
    """fwd + out-of-place and in-place bwd with the cap, incl. the EXTRA picks; logits N(0, 3): cap 3 bends most of them, cap 30
    (Gemma-2's own) hardly any."""
    logits, labels, ex_rows, ex_lab, glp, gent, gex = _lp_case(R, V, dtype, R * 1000 + V)
    lp_ref, ent_ref, lp2_ref, g_ref = _ref64(logits, labels, ex_rows, ex_lab, glp, gent, gex, temp, cap)
    if cap == 3.0:                                          # the cap matters: the uncapped statistics are far outside the tolerance
        plain = _ref64(logits, labels, ex_rows, ex_lab, glp, gent, gex, temp, 1e9)
        assert float((plain[1] - ent_ref).abs().max()) > 100 * ENT_TOL * (1 + float(ent_ref.abs().max()))
    ld = logits.to(DEV)
    if V % 8:
        buf = torch.zeros(R, (V + 7) // 8 * 8, dtype=dtype, device=DEV); buf[:, :V] = ld; ld = buf[:, :V]
    ptr_, exl = _csr(ex_rows, R).to(DEV), ex_lab.to(DEV)
    lp2 = torch.empty(ex_rows.numel(), dtype=F32, device=DEV)
    lse, ent, lp = ops.logprob_entropy_fwd_raw(ld, labels.to(DEV), True, temp, ptr_, exl, lp2, softcap=cap)
    assert (lp.double().cpu() - lp_ref).abs().max() <= LP_TOL * (1 + lp_ref.abs().max())
    assert (lp2.double().cpu() - lp2_ref).abs().max() <= LP_TOL * (1 + lp2_ref.abs().max())
    assert (ent.double().cpu() - ent_ref).abs().max() <= ENT_TOL * (1 + ent_ref.abs().max())
    out = torch.empty_strided(ld.shape, ld.stride(), dtype=ld.dtype, device=DEV)
    ops.logprob_entropy_bwd_raw(ld, labels.to(DEV), lse, ent, glp.to(DEV), gent.to(DEV), temp, ptr_, exl, gex.to(DEV), out=out, softcap=cap)
    assert torch.equal(ld.float().cpu(), logits.float())
    assert float((out.double().cpu() - g_ref).norm() / g_ref.norm()) <= GRAD_TOL[dtype]
    ops.logprob_entropy_bwd_raw(ld, labels.to(DEV), lse, ent, glp.to(DEV), gent.to(DEV), temp, ptr_, exl, gex.to(DEV), softcap=cap)      # in place
    assert torch.equal(ld.float().cpu(), out.float().cpu())


@pytest.mark.parametrize("V,dtype", [(256, BF), (256000, BF), (304, F32)])
def test_capped_shard_stats_over_two_halves_equal_the_unsharded_result(V, dtype):
    """The cap is elementwise and comes before the shard statistics: per-half statistics combined on the host (the arithmetic of
    ops.combine_shard_stats without the collectives) equal the unsharded capped kernel."""
    R, temp, cap = 6, 0.7, 3.0
    logits, labels, ex_rows, ex_lab, *_ = _lp_case(R, V, dtype, V + 1)
    ld = logits.to(DEV)
    ptr_, exl = _csr(ex_rows, R).to(DEV), ex_lab.to(DEV)
    lp2 = torch.empty(ex_rows.numel(), dtype=F32, device=DEV)
    lse, ent, lp = ops.logprob_entropy_fwd_raw(ld, labels.to(DEV), True, temp, ptr_, exl, lp2, softcap=cap)
    h = V // 2
    stats, picks = [], []
    for r in range(2):
        shard = ld[:, r * h:(r + 1) * h]
        ex_out = torch.empty(ex_rows.numel(), dtype=F32, device=DEV)
        stats.append(ops.logprob_entropy_shard_stats_raw(shard, ops.local_labels(labels.to(DEV), r * h, h), temp, ptr_,
                                                         ops.local_labels(exl, r * h, h), ex_out, softcap=cap).double().cpu())
        picks.append(ex_out.double().cpu())
    M = torch.maximum(stats[0][:, 0], stats[1][:, 0])
    f = [torch.exp2(s[:, 0] - M) for s in stats]
    S = stats[0][:, 1] * f[0] + stats[1][:, 1] * f[1]
    Tt = stats[0][:, 2] * f[0] + stats[1][:, 2] * f[1]
    lse2 = (M + torch.log2(S)) * math.log(2.0)
    ent2 = lse2 - (Tt / S) * math.log(2.0)
    lp_c = stats[0][:, 3] + stats[1][:, 3] - lse2
    ok = ((labels >= 0) & (labels < V)).double()
    assert (lse2 - lse.double().cpu()).abs().max() <= LP_TOL * (1 + lse2.abs().max())
    assert (ent2 - ent.double().cpu()).abs().max() <= ENT_TOL * (1 + ent2.abs().max())
    assert (lp_c * ok - lp.double().cpu()).abs().max() <= LP_TOL * (1 + lp_c.abs().max())
    ex = picks[0] + picks[1] - lse2[ex_rows]
    assert (ex - lp2.double().cpu()).abs().max() <= LP_TOL * (1 + ex.abs().max())


@pytest.mark.parametrize("dtype", [BF, F32])
def test_zero_softcap_is_the_plain_logprob_entry_bitwise(dtype):
    R, V, temp = 9, 1000, 0.7
    logits, labels, ex_rows, ex_lab, glp, gent, gex = _lp_case(R, V, dtype, 77)
    ld, lab = logits.to(DEV), labels.to(DEV)
    ptr_, exl = _csr(ex_rows, R).to(DEV), ex_lab.to(DEV)
    glp, gex, gent = glp.to(DEV), gex.to(DEV), gent.to(DEV)
    # the ops raw functions with their default cap ...
    lp2, pk = (torch.empty(ex_rows.numel(), dtype=F32, device=DEV) for _ in range(2))
    lse, ent, lp = ops.logprob_entropy_fwd_raw(ld, lab, True, temp, ptr_, exl, lp2)
    stats = ops.logprob_entropy_shard_stats_raw(ld, lab, temp, ptr_, exl, pk)
    out = ops.logprob_entropy_bwd_raw(ld, lab, lse, ent, glp, gent, temp, ptr_, exl, gex, out=torch.empty_like(ld))
    res = [(lse, ent, lp, lp2, stats, pk, out)]
    for cap in (0.0, -3.0):                                          # ... and the three entries with a zero and a negative cap
        lse, ent, lp, lp2 = (torch.empty(n, dtype=F32, device=DEV) for n in (R, R, R, ex_rows.numel()))
        assert lib().dta_logprob_entropy_fwd(ptr(ld), ptr(lab), ptr(ptr_), ptr(exl), ptr(lse), ptr(ent), ptr(lp), ptr(lp2),
                                             R, V, ld.stride(0), temp, ops._DT[dtype], cap, None) == 0
        stats, pk = torch.empty(R, 4, device=DEV), torch.empty(ex_rows.numel(), device=DEV)
        assert lib().dta_logprob_entropy_shard_stats(ptr(ld), ptr(lab), ptr(ptr_), ptr(exl), ptr(stats), ptr(pk),
                                                     R, V, ld.stride(0), temp, ops._DT[dtype], cap, None) == 0
        out = torch.empty_like(ld)
        assert lib().dta_logprob_entropy_bwd(ptr(ld), ptr(out), ptr(lab), ptr(ptr_), ptr(exl), ptr(lse), ptr(ent), ptr(glp), ptr(gex), ptr(gent),
                                             R, V, ld.stride(0), out.stride(0), temp, ops._DT[dtype], cap, None) == 0
        torch.cuda.synchronize()
        res.append((lse, ent, lp, lp2, stats, pk, out))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
    lse = torch.empty(R, device=DEV)
    for bad in (float("nan"), float("inf")):
        assert lib().dta_logprob_entropy_fwd(ptr(ld), None, None, None, ptr(lse), None, None, None, R, V, ld.stride(0), 1.0, ops._DT[dtype],
                                             bad, None) == -1


def test_lm_head_rows_with_a_cap_matches_float64():
    """ops.lm_head_rows(softcap=...) end to end (kept and chunked logits, fork picks, gradients of h and W) against float64."""
    g = torch.Generator().manual_seed(9)
    T, H, V, cap = 70, 64, 256, 3.0
    h = torch.randn(T, H, generator=g).to(BF); Wt = (0.4 * torch.randn(V, H, generator=g)).to(BF)
    nxt = torch.randint(0, V, (T,), generator=g)
    rows = torch.tensor([3, 3, 40]); ftok = torch.tensor([5, 9, 200])
    gl, gf, ge = torch.randn(T, generator=g), torch.randn(3, generator=g), torch.randn(T, generator=g)
    h64, W64 = h.double().requires_grad_(True), Wt.double().requires_grad_(True)
    lp_all = torch.log_softmax(_cap64(h64 @ W64.T, cap), -1)
    lp_ref, lf_ref, ent_ref = lp_all.gather(-1, nxt[:, None]).squeeze(-1), lp_all[rows, ftok], -(lp_all.exp() * lp_all).sum(-1)
    ((lp_ref * gl).sum() + (lf_ref * gf).sum() + (ent_ref * ge).sum()).backward()
    for keep in (1 << 40, 0):
        hd, Wd = h.to(DEV).requires_grad_(True), Wt.to(DEV).requires_grad_(True)
        bounds = torch.searchsorted(rows, torch.arange(0, T + 32, 32)).tolist()
        lp, lf, ent = ops.lm_head_rows(hd, Wd, nxt.to(DEV), _csr(rows, T).to(DEV), ftok.to(DEV), rows.to(DEV), bounds, True, 32, keep_bytes=keep,
                                       softcap=cap, max_picks_per_row=2)
        ((lp * gl.to(DEV)).sum() + (lf * gf.to(DEV)).sum() + (ent * ge.to(DEV)).sum()).backward()
        # bf16 logits (the GEMM's output rounding) set the accuracy here, as for the uncapped operator: 0.06 on values
        assert (lp.double().cpu() - lp_ref.detach()).abs().max() < 0.06 and (lf.double().cpu() - lf_ref.detach()).abs().max() < 0.06
        assert (ent.double().cpu() - ent_ref.detach()).abs().max() < 0.06
        # bf16 logits of magnitude ~3 give p a relative error of about |x| 2^-9 = 6e-3; the bf16 roundings of dlogits and of the two GEMM
        # outputs add 2^-9 each: about 1.2e-2 in all
        assert _rel(hd.grad, h64.grad) <= 2e-2 and _rel(Wd.grad, W64.grad) <= 2e-2
    with pytest.raises(ValueError, match="picks"):
        ops.lm_head_rows(hd, Wd, nxt.to(DEV), None, ftok.new_zeros(0).to(DEV), rows.new_zeros(0).to(DEV), [0] * 8, True, 32, softcap=cap,
                         max_picks_per_row=5000)
