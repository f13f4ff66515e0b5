"""The two OLMo row kernels - the projection-wide q/k RMSNorm + RoPE (dta_wide_qk_norm_rope_fwd / _bwd) and RMSNorm-then-add
(dta_rmsnorm_add_fwd) - against float64, element by element: every output within the bound tests/olmo_ref64.py assembles from the
terms of tests/rowops_ref64.py, in bf16, f16 and fp32 storage, on rowops_ref64.rows (log-spaced row scales, an all-zero row, a
single-element row).  Shapes: rows narrower than one wave's reach, NH no multiple of 4, 1536 (no power of two), 5120, both ways to the
8192 limit; 1 / 3 / 5 / 37 tokens (a partial workgroup, several workgroups); the backward's second, ragged grid-stride pass; q and k in
place from a fused [T, Hq+2Hkv, D] buffer with the gradients landing in one buffer; a frozen weight; every output a NaN-filled arena
of tests/arena.py whose guard bands, in front and behind, must keep their bytes.  tests/test_olmo_fixture.py shows on the CPU that the
bounds hold for an honest emulation and reject the per-head arithmetic.

Each test prints its worst err / bound per output (pytest -s shows them)."""
import json

import pytest
import torch

import arena as A
import olmo_ref64 as OR
import rowops_ref64 as R
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
EPS = (1e-6, 1e-5)
TAIL = 96                         # guard elements in front of and behind every output


def _merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def _report(name, dtype, worst):
    print(f"\nWORST {name} {str(dtype).split('.')[-1]} " + json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


def _poisoned(name, n, dtype):
    """An output arena of n elements, NaN in the payload and in the guard bands."""
    return A.out_arena(name, (n,), dtype, "A", guard_rows=TAIL, device=DEV)


def _inputs(T, NH, D, dtype, seed):
    x = R.rows(T, NH * D, dtype, seed).view(T, NH, D).to(DEV)
    w = R.norm_weight(NH * D, dtype, seed + 1, False).to(DEV)
    depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    return x, w, ops.rope_cos_sin(depth, D, 1e4), R.randn((T, NH, D), dtype, seed + 3).to(DEV)


def _wide_fwd(x, w, cs, eps, label=""):
    """One forward entry call over x [T, NH, D] (any token stride) into poisoned buffers: (y, rstd)."""
    T, NH, D = x.shape
    n = T * NH * D
    yb, rb = _poisoned("y", n, x.dtype), _poisoned("rstd", T, F32)
    ops._launch("dta_wide_qk_norm_rope_fwd", (x, w, cs), ptr(x), ptr(w), ptr(cs), yb.ptr(), rb.ptr(), T, NH, D, x.stride(0), eps, ops._DT[x.dtype])
    yb.assert_guards_intact(label); rb.assert_guards_intact(label)
    return yb.view.view(T, NH, D), rb.view


def _wide_bwd(x, w, cs, dy, rstd, frozen=False, label=""):
    """One backward entry call, out of place, into poisoned buffers: (dx, dw | None).  The partials workspace is poisoned too: every
    row the kernel owns is written in full, nothing behind it."""
    T, NH, D = x.shape
    n = NH * D
    dxb = _poisoned("dx", T * n, x.dtype)
    dx = dxb.view.view(T, NH, D)
    blocks = lib().dta_wide_qk_norm_rope_bwd_blocks(T)
    pb = None if frozen else _poisoned("dw_partial", blocks * n, F32)
    ops._launch("dta_wide_qk_norm_rope_bwd", (x, w, cs, dy), ptr(x), ptr(w), ptr(cs), ptr(dy), ptr(rstd), ptr(dx), None if frozen else pb.ptr(),
                T, NH, D, x.stride(0), dy.stride(0), dy.stride(1), dx.stride(0), ops._DT[x.dtype])
    dxb.assert_guards_intact(label)
    if frozen:
        return dx, None
    pb.assert_guards_intact(label)
    part = pb.view.view(blocks, n)
    assert bool(torch.isfinite(part).all()), label + ": a row of dw_partial was left unwritten"
    return dx, ops.sum_slabs(part, w.dtype)


def _wide_case(T, NH, D, dtype, eps, worst):
    label = f"T={T} NH={NH} D={D} eps={eps}"
    x, w, cs, dy = _inputs(T, NH, D, dtype, T + NH + D)
    y, rstd = _wide_fwd(x, w, cs, eps, label)
    _merge(worst, R.check_all("wide_qk", {"y": y, "rstd": rstd}, OR.wide_fwd_ref(x, w, cs, eps, dtype), label))
    dx, dw = _wide_bwd(x, w, cs, dy, rstd, label=label)
    _merge(worst, R.check_all("wide_qk", {"dx": dx, "dw": dw}, OR.wide_bwd_ref(x, w, cs, dy, eps, dtype), label))
    dx2, dw2 = _wide_bwd(x, w, cs, dy, rstd, label=label)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2), label + ": a repeated backward differs"
    assert torch.equal(_wide_bwd(x, w, cs, dy, rstd, frozen=True, label=label)[0], dx), label + ": dx of the frozen-weight call differs"
    return x, w, cs, dy, y, dx, dw


WIDE_SHAPES = [(64, 1), (64, 3), (64, 4), (128, 1), (128, 5), (128, 8), (128, 12), (128, 40), (128, 64), (64, 128)]
# and the edges of the kernel forms: 2 048 (the longest row one wave takes) and 2 112 (the shortest the four waves of a workgroup
# share), 4 096 and 4 160 (2 and 4 groups per lane of that form)
WIDE_SHAPES += [(128, 16), (64, 33), (128, 32), (64, 65)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,NH", WIDE_SHAPES)
def test_wide_qk_norm_rope_every_form(D, NH, dtype):
    """Every kernel form (one wave or four per token x 2 / 4 groups per lane x head_dim 64 / 128) and rows that fill a fraction of a
    wave; T 1 / 3 / 5 / 37."""
    worst = {}
    for i, T in enumerate((1, 3, 5, 37)):
        _wide_case(T, NH, D, dtype, EPS[i % 2], worst)
    _report(f"wide_qk D={D} NH={NH}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,NH", [(64, 2), (128, 1)])
def test_wide_qk_norm_rope_grid_stride_backward(D, NH, dtype):
    """NH * D = 128 at T = (the backward's workgroup cap) x (4 tokens per workgroup) + 5: the grid-stride loop runs a second, ragged
    pass, and dw accumulates across the passes."""
    cap = lib().dta_wide_qk_norm_rope_bwd_blocks(1 << 30)
    T = cap * 4 + 5
    assert lib().dta_wide_qk_norm_rope_bwd_blocks(T) == cap == lib().dta_wide_qk_norm_rope_bwd_blocks(T - 5)
    worst = {}
    _wide_case(T, NH, D, dtype, 1e-6, worst)
    _report(f"wide_qk_grid_stride T={T} D={D} NH={NH}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (3, 1), (40, 8)])
@pytest.mark.parametrize("D", [64, 128])
def test_qkv_prep_wide_with_the_gradients_in_one_fused_buffer(D, Hq, Hkv, dtype):
    """ops.qkv_prep_wide: q / k read at the fused buffer's token stride; with dq, dk, dv side by side in ONE [T, Hq+2Hkv, D] buffer the
    backward runs in place on it - bit-equal to the out-of-place path (separate gradients), the v slice untouched - and a frozen
    weight gets no gradient while dx keeps its bits."""
    worst, H3 = {}, Hq + 2 * Hkv
    for i, T in enumerate((1, 5, 37)):
        eps, label = EPS[i % 2], f"T={T} Hq={Hq} Hkv={Hkv} D={D}"
        qkv = R.rows(T, H3 * D, dtype, T + H3 + D).view(T, H3, D).to(DEV)
        wq, wk = R.norm_weight(Hq * D, dtype, 5, False).to(DEV), R.norm_weight(Hkv * D, dtype, 6, False).to(DEV)
        depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(T)).to(DEV)
        cs, grads = ops.rope_cos_sin(depth, D, 1e4), R.randn((T, H3, D), dtype, 9).to(DEV)
        a = qkv.clone().requires_grad_(True)
        ws = [wq.clone().requires_grad_(True), wk.clone().requires_grad_(True)]
        q, k, v = ops.qkv_prep_wide(a, ws[0], ws[1], cs, eps, Hq, Hkv)
        assert torch.equal(v, qkv[:, Hq + Hkv:]) and v.data_ptr() == a.data_ptr() + (Hq + Hkv) * D * a.element_size()       # a view
        saved = q.grad_fn.saved_tensors
        buf = grads.clone()
        inp = torch.autograd.grad([q, k, v], [a] + ws, [buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]], retain_graph=True)
        assert inp[0].data_ptr() == buf.data_ptr(), label + ": the backward did not run in place on the gradient buffer"
        sep = [grads[:, :Hq].clone(), grads[:, Hq:Hq + Hkv].clone(), grads[:, Hq + Hkv:].clone()]     # three tensors of their own
        out = torch.autograd.grad([q, k, v], [a] + ws, sep, retain_graph=True)
        assert out[0].data_ptr() not in (buf.data_ptr(), sep[0].data_ptr())
        for x, y in zip(inp, out):
            assert torch.equal(x, y), label + ": the in-place backward differs from the out-of-place one"
        d = inp[0]
        assert torch.equal(d[:, Hq + Hkv:], grads[:, Hq + Hkv:]), label + ": v's gradient slice changed"
        for j, (lo, NH, o, w) in enumerate(((0, Hq, q, wq), (Hq, Hkv, k, wk))):
            xs, gs = qkv[:, lo:lo + NH], grads[:, lo:lo + NH]
            _merge(worst, R.check_all("qkv_prep_wide", {"y": o, "rstd": saved[4 + j]}, OR.wide_fwd_ref(xs, w, cs, eps, dtype), label))
            _merge(worst, R.check_all("qkv_prep_wide", {"dx": d[:, lo:lo + NH], "dw": inp[1 + j]}, OR.wide_bwd_ref(xs, w, cs, gs, eps, dtype), label))
        # frozen norm weights: no gradient for them, the same dx bits
        b = qkv.clone().requires_grad_(True)
        q2, k2, v2 = ops.qkv_prep_wide(b, wq, wk, cs, eps, Hq, Hkv)
        assert torch.equal(q2, q) and torch.equal(k2, k)
        buf = grads.clone()
        (d2,) = torch.autograd.grad([q2, k2, v2], [b], [buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]])
        assert torch.equal(d2, d), label + ": dx of the frozen-weight call differs"
    _report(f"qkv_prep_wide D={D} Hq={Hq} Hkv={Hkv}", dtype, worst)


# ------------------------------------------------------------------------------------------------ RMSNorm, then the residual add
def _norm_add(y, w, res, eps, want_yn, label=""):
    R_, H = y.shape
    ob, rb = _poisoned("out", R_ * H, y.dtype), _poisoned("rstd", R_, F32)
    nb = _poisoned("yn", R_ * H, y.dtype) if want_yn else None
    ops._launch("dta_rmsnorm_add_fwd", (y, w, res), ptr(y), ptr(w), ptr(res), ob.ptr(), nb.ptr() if want_yn else None, rb.ptr(), R_, H, eps,
                ops._DT[y.dtype])
    ob.assert_guards_intact(label); rb.assert_guards_intact(label)
    if want_yn:
        nb.assert_guards_intact(label)
    return ob.view.view(R_, H), (nb.view.view(R_, H) if want_yn else None), rb.view


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [32, 1032, 2048, 2056, 4096, 4104, 5120, 8192, 16384])
def test_rmsnorm_add_every_form(H, dtype):
    """The register forms (2 / 4 / 8 groups per lane), the two-pass form above 4096 up to 16384; 1 / 3 / 5 / 37 rows; yn given and NULL
    (the same out bits); the operator's backward - dy through the existing RMSNorm bound, d res = d out bitwise - where the backward
    kernel reaches (H <= 8192)."""
    worst = {}
    for i, R_ in enumerate((1, 3, 5, 37)):
        eps, label = EPS[i % 2], f"R={R_} H={H} eps={EPS[i % 2]}"
        y, res, w = (t.to(DEV) for t in (R.rows(R_, H, dtype, R_ + H), R.randn((R_, H), dtype, H + 1), R.norm_weight(H, dtype, H + 2, False)))
        out, yn, rstd = _norm_add(y, w, res, eps, True, label)
        _merge(worst, R.check_all("rmsnorm_add", {"out": out, "yn": yn, "rstd": rstd}, OR.norm_add_ref(y, w, res, eps, dtype), label))
        out2, _, rstd2 = _norm_add(y, w, res, eps, False, label)
        assert torch.equal(out, out2) and torch.equal(rstd, rstd2), label + ": out without yn differs"
        ya, ra, wa = y.clone().requires_grad_(True), res.clone().requires_grad_(True), w.clone().requires_grad_(True)
        o3 = ops.rms_norm_add(ra, ya, wa, eps)
        assert torch.equal(o3, out), label + ": the operator differs from the entry"
        g = R.randn((R_, H), dtype, H + 3).to(DEV)
        if H > 8192:
            with pytest.raises(RuntimeError, match="dta_rmsnorm_bwd failed: DTA_EUNSUPPORTED"):
                o3.backward(g)
            continue
        dres, dy, dw = torch.autograd.grad(o3, [ra, ya, wa], g, retain_graph=True)
        assert torch.equal(dres, g), label + ": d res is not d out"
        _merge(worst, R.check_all("rmsnorm_add", {"dx": dy, "dw": dw}, R.rmsnorm_bwd_ref(y, w, g, None, eps, 0.0, dtype), label))
        wf = w.clone()                                          # frozen weight: the same dy bits
        yb = y.clone().requires_grad_(True)
        (dy2,) = torch.autograd.grad(ops.rms_norm_add(res, yb, wf, eps), [yb], g)
        assert torch.equal(dy2, dy), label + ": dy of the frozen-weight call differs"
    _report(f"rmsnorm_add H={H}", dtype, worst)
