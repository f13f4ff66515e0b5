"""The row kernels (RMSNorm with / without the residual add and the weight offset, head-norm + RoPE, SwiGLU, GeGLU, dta_sum_slabs) against
float64, element by element: every output of every kernel within the bound tests/rowops_ref64.py derives from the kernel's documented
arithmetic, at every kernel form (the H thresholds of RMSNorm and one vector above them, the wide forward, HPL 1 / 4 x D 64 / 128), the
grid-stride passes no other unit test reaches, ragged unit counts, eps-sensitive / all-zero / single-element rows, bf16, f16 and fp32
storage, a frozen norm weight, and twice over for bit-identical repeats.  tests/test_rowops_ref64.py shows on the CPU that the bounds
hold for an honest emulation and reject the corruptions a whole-tensor norm lets through.  The float64 references run on the device.

Each test prints its worst err / bound per output (pytest -s shows them)."""
import itertools
import json

import pytest
import torch

import rowops_ref64 as R
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
EPS = (1e-6, 1e-5)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def _report(name, dtype, worst):
    print(f"\nWORST {name} {str(dtype).split('.')[-1]} " + json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


# ------------------------------------------------------------------------------------------------ RMSNorm
def _rms_fwd(x, delta, w, eps, off):
    R_, H = x.shape
    y, rstd = torch.empty_like(x), torch.empty(R_, dtype=F32, device=x.device)
    xo = torch.empty_like(x) if delta is not None else None
    ops._launch("dta_rmsnorm_fwd", (x, delta, w), ptr(x), ptr(delta), ptr(w), ptr(xo), ptr(y), ptr(rstd), R_, H, eps, off, ops._DT[x.dtype])
    return xo, y, rstd


def _rms_bwd(xin, w, dy, dres, rstd, off, frozen=False):
    """(dx, dw) as ops._RMSNorm.backward forms them: the per-workgroup partials summed by dta_sum_slabs; frozen: no partials, dw None."""
    R_, H = xin.shape
    dx = torch.empty_like(xin)
    part = None if frozen else torch.empty(lib().dta_rmsnorm_bwd_blocks(R_), H, dtype=F32, device=xin.device)
    ops._launch("dta_rmsnorm_bwd", (xin, w, dy, dres), ptr(xin), ptr(w), ptr(dy), ptr(dres), ptr(rstd), ptr(dx), ptr(part), R_, H, off,
                ops._DT[xin.dtype])
    return dx, (None if frozen else ops.sum_slabs(part, w.dtype))


def _rms_case(R_, H, dtype, has_delta, off, eps, worst, backward=True):
    label = f"R={R_} H={H} delta={has_delta} w_offset={off} eps={eps}"
    x = R.rows(R_, H, dtype, R_ + H)
    x, delta, w, dy, dres = _dev(x, R.delta_for(x, H + 1) if has_delta else None, R.norm_weight(H, dtype, H, bool(off)),
                                 R.randn((R_, H), dtype, H + 2), R.randn((R_, H), dtype, H + 3) if has_delta else None)
    xo, y, rstd = _rms_fwd(x, delta, w, eps, off)
    xin = xo if has_delta else x
    if has_delta:                                     # x_out first: it is the input the norm's reference takes
        _merge(worst, R.check_all("rmsnorm", {"x_out": xo}, R.rmsnorm_fwd_ref(x, delta, w, eps, off, dtype), label))
    _merge(worst, R.check_all("rmsnorm", {"y": y, "rstd": rstd}, R.rmsnorm_fwd_ref(x, delta, w, eps, off, dtype, xin=xin), label))
    if not backward:
        return
    dx, dw = _rms_bwd(xin, w, dy, dres, rstd, off)
    _merge(worst, R.check_all("rmsnorm", {"dx": dx, "dw": dw}, R.rmsnorm_bwd_ref(xin, w, dy, dres, eps, off, dtype), label))
    dx2, dw2 = _rms_bwd(xin, w, dy, dres, rstd, off)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2), label + ": a repeated backward differs"
    assert torch.equal(_rms_bwd(xin, w, dy, dres, rstd, off, frozen=True)[0], dx), label + ": dx of the frozen-weight call differs"
    return x, delta, w, dy, dres, xo, y, dx, dw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 72, 1024, 1032, 2048, 2056, 4096, 4104, 8192])
def test_rmsnorm_every_form(H, dtype):
    """Every template instance (NA 2 / 4 / 8 / 16 at and one vector above each threshold, the offset form), 1 / 3 / 6 rows (a partial
    workgroup, two workgroups), with and without delta / dres, weight gradient wanted or not."""
    worst = {}
    for i, (R_, has_delta, off) in enumerate(itertools.product((1, 3, 6), (False, True), (0.0, 1.0))):
        _rms_case(R_, H, dtype, has_delta, off, EPS[(i + i // 2) % 2], worst)
    _report("rmsnorm", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [72, 2056, 8192])
def test_rmsnorm_operator_matches_the_entry_bitwise_also_with_a_frozen_weight(H, dtype):
    """ops.add_rms_norm / ops.rms_norm through autograd: the bits of the checked entry-point calls, whether the weight wants a gradient
    or not (requires_grad False: the kernel gets no partials buffer)."""
    for has_delta, off in itertools.product((False, True), (0.0, 1.0)):
        x, delta, w, dy, dres, xo, y, dx, dw = _rms_case(6, H, dtype, has_delta, off, 1e-6, {})
        for frozen in (False, True):
            xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(not frozen)
            if has_delta:
                da = delta.clone().requires_grad_(True)
                xo2, y2 = ops.add_rms_norm(xa, da, wa, 1e-6, off)
                grads = torch.autograd.grad([xo2, y2], [xa, da] + ([] if frozen else [wa]), [dres, dy])
                assert torch.equal(xo2, xo) and torch.equal(grads[1], dx)
            else:
                y2 = ops.rms_norm(xa, wa, 1e-6, off)
                grads = torch.autograd.grad(y2, [xa] + ([] if frozen else [wa]), dy)
            assert torch.equal(y2, y) and torch.equal(grads[0], dx)
            assert frozen or torch.equal(grads[-1], dw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8200, 16384])
def test_rmsnorm_wide_forward_and_no_backward(H, dtype):
    """H > 8192: the forward's two-pass form under no_grad; the backward refuses (the library's error) and writes nothing."""
    worst = {}
    with torch.no_grad():
        for i, (R_, has_delta, off) in enumerate(itertools.product((1, 6), (False, True), (0.0, 1.0))):
            _rms_case(R_, H, dtype, has_delta, off, EPS[i % 2], worst, backward=False)
        x, w = _dev(R.rows(3, H, dtype, 1), R.norm_weight(H, dtype, 2, False))
        xo, y = ops.add_rms_norm(x, x, w, 1e-6)
        assert torch.equal(y, _rms_fwd(x, x, w, 1e-6, 0.0)[1])
    _report("rmsnorm_wide", dtype, worst)
    rstd, dy = torch.ones(3, dtype=F32, device=DEV), torch.ones_like(x)
    dx = torch.full_like(x, 7.0)
    part = torch.full((lib().dta_rmsnorm_bwd_blocks(3), H), 7.0, dtype=F32, device=DEV)
    with pytest.raises(RuntimeError, match="dta_rmsnorm_bwd failed: DTA_EUNSUPPORTED"):
        ops._launch("dta_rmsnorm_bwd", (x, w, dy), ptr(x), ptr(w), ptr(dy), None, ptr(rstd), ptr(dx), ptr(part), 3, H, 0.0, ops._DT[dtype])
    torch.cuda.synchronize()
    assert bool((dx == 7.0).all()) and bool((part == 7.0).all())
    xa = x.clone().requires_grad_(True)
    ya = ops.rms_norm(xa, w, 1e-6)
    with pytest.raises(RuntimeError, match="dta_rmsnorm_bwd failed: DTA_EUNSUPPORTED"):
        ya.backward(dy)
    assert xa.grad is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R_,H,backward", [(8197, 64, True), (16391, 64, True), (32771, 8, False)])
def test_rmsnorm_grid_stride(R_, H, backward, dtype):
    """More rows than one pass of the capped grid (backward 2048 x 4, forward 8192 x 4), ragged: some waves take a pass more than
    others, and dw sums the passes of every workgroup (n = R in its bound)."""
    worst = {}
    for i, (has_delta, off) in enumerate([(False, 0.0), (True, 1.0)]):
        _rms_case(R_, H, dtype, has_delta, off, EPS[i], worst, backward=backward)
    _report(f"rmsnorm_grid_stride R={R_}", dtype, worst)


# ------------------------------------------------------------------------------------------------ head-norm + RoPE
def _qk_inputs(T, NH, D, dtype, norm, seed):
    x = R.rows(T * NH, D, dtype, seed).view(T, NH, D)
    depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(seed + 2))
    x, w, dy, depth = _dev(x, R.norm_weight(D, dtype, seed + 1, False) if norm else None, R.randn((T, NH, D), dtype, seed + 3), depth)
    return x, w, ops.rope_cos_sin(depth, D, 1e6), dy


def _qk_case(T, NH, D, dtype, norm, eps, worst):
    label = f"T={T} NH={NH} D={D} norm={norm} eps={eps}"
    x, w, cs, dy = _qk_inputs(T, NH, D, dtype, norm, T + NH + D)
    xa, wa = x.clone().requires_grad_(True), (w.clone().requires_grad_(True) if norm else None)
    y = ops.qk_norm_rope(xa, wa, cs, eps)
    got = {"y": y, **({"rstd": y.grad_fn.saved_tensors[3]} if norm else {})}
    _merge(worst, R.check_all("qk_norm_rope" if norm else "rope", got, R.qk_fwd_ref(x, w, cs, eps, dtype), label))
    wrt = [xa, wa] if norm else [xa]
    g1 = torch.autograd.grad(y, wrt, dy, retain_graph=True)
    _merge(worst, R.check_all("qk_norm_rope" if norm else "rope", dict(zip(("dx", "dw"), g1)), R.qk_bwd_ref(x, w, cs, dy, eps, dtype), label))
    for a, b in zip(g1, torch.autograd.grad(y, wrt, dy)):
        assert torch.equal(a, b), label + ": a repeated backward differs"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("NH", [1, 3, 4, 12])
@pytest.mark.parametrize("D", [64, 128])
def test_qk_norm_rope_every_form(D, NH, dtype):
    """HPL 1 (NH 1, 3) and 4 (NH 4, 12) x D 64 / 128 x norm / RoPE only; T 1 / 5 / 33: unit counts that are no multiple of a
    workgroup's 16 (D 128) or 32 (D 64); positions up to 131 071."""
    worst = {}
    for i, (T, norm) in enumerate(itertools.product((1, 5, 33), (True, False))):
        _qk_case(T, NH, D, dtype, norm, EPS[(i // 2) % 2], worst)
    _report(f"qk_norm_rope D={D} NH={NH}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (3, 1), (14, 2)])
@pytest.mark.parametrize("D", [64, 128])
def test_qkv_prep_with_the_gradients_in_one_fused_buffer(D, Hq, Hkv, dtype):
    """ops.qkv_prep: q / k read at the fused buffer's token stride; dq, dk, dv arrive side by side in ONE [T, Hq+2Hkv, D] buffer, so dy is
    strided and dx is written in place over it.  All three returned gradients (the v slice: untouched bits), both dw, twice over."""
    worst, H3 = {}, Hq + 2 * Hkv
    for i, (T, norm) in enumerate(itertools.product((1, 5, 33), (True, False))):
        eps, label = EPS[i % 2], f"T={T} Hq={Hq} Hkv={Hkv} D={D} norm={norm}"
        qkv, w, cs, grads = _qk_inputs(T, H3, D, dtype, norm, T + H3 + D)
        wk = R.norm_weight(D, dtype, 77, False).to(DEV) if norm else None
        a = qkv.clone().requires_grad_(True)
        ws = [t.clone().requires_grad_(True) for t in (w, wk)] if norm else [None, None]
        q, k, v = ops.qkv_prep(a, ws[0], ws[1], cs, eps, Hq, Hkv)
        assert torch.equal(v, qkv[:, Hq + Hkv:])
        saved = q.grad_fn.saved_tensors
        res = []
        for rep in range(2):
            buf = grads.clone()
            got = torch.autograd.grad([q, k, v], [a] + ws * norm, [buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]], retain_graph=rep == 0)
            assert got[0].data_ptr() == buf.data_ptr(), label + ": the backward did not run in place on the gradient buffer"
            res.append(got)
        for x, y in zip(*res):
            assert torch.equal(x, y), label + ": a repeated backward differs"
        d = res[0][0]
        assert torch.equal(d[:, Hq + Hkv:], grads[:, Hq + Hkv:])
        name = "qkv_prep" if norm else "qkv_prep_rope"
        for j, (lo, NH, out) in enumerate(((0, Hq, q), (Hq, Hkv, k))):
            xs, gs, wj = qkv[:, lo:lo + NH], grads[:, lo:lo + NH], (w, wk)[j]
            got = {"y": out, **({"rstd": saved[4 + j]} if norm else {})}
            _merge(worst, R.check_all(name, got, R.qk_fwd_ref(xs, wj, cs, eps, dtype), label))
            got = {"dx": d[:, lo:lo + NH], **({"dw": res[0][1 + j]} if norm else {})}
            _merge(worst, R.check_all(name, got, R.qk_bwd_ref(xs, wj, cs, gs, eps, dtype), label))
    _report(f"qkv_prep D={D} Hq={Hq} Hkv={Hkv}", dtype, worst)


def _prep_form(form, qkv, depth, D, Hq, Hkv, dtype):
    """(q, k, v, the norm weights that take a gradient) of one q|k|v member form over the leaf qkv."""
    wn = {"head_norm": (D, D), "wide_norm": (Hq * D, Hkv * D)}.get(form, ())
    ws = [R.norm_weight(n, dtype, 5 + j, False).to(DEV).requires_grad_(True) for j, n in enumerate(wn)]
    if form == "none":
        return (*ops.qkv_prep_nope(qkv, Hq, Hkv), ws)
    if form in ("half_split", "interleaved"):
        rot = D // 2 if form == "half_split" else D
        return (*ops.qkv_prep_partial(qkv, ops.rope_cos_sin(depth, rot, 1e6), Hq, Hkv, form == "interleaved"), ws)
    prep = ops.qkv_prep_wide if form == "wide_norm" else ops.qkv_prep
    return (*prep(qkv, *(ws or (None, None)), ops.rope_cos_sin(depth, D, 1e6), 1e-6, Hq, Hkv), ws)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("form", ["none", "rope", "head_norm", "wide_norm", "half_split", "interleaved"])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (3, 1)])
@pytest.mark.parametrize("D", [64, 128])
def test_qkv_prep_backward_paths_agree_in_every_form(D, Hq, Hkv, form, dtype):
    """The two backward paths of every q|k|v member form - no rotation, RoPE alone, per-head norm + RoPE, projection-wide norm + RoPE,
    half-split partial RoPE over R = D/2, interleaved over R = D - at T = 5 (dead lane groups in the last workgroup), 4 heads per lane
    group and 1: with dq, dk, dv the slices of ONE [T, Hq+2Hkv, D] buffer the backward returns that buffer; with three tensors of
    their own it gathers into a fresh one.  The same kernels on the same grid over the same values: both results and both dw pairs are
    equal bit for bit."""
    T, H3 = 5, Hq + 2 * Hkv
    label = f"form={form} Hq={Hq} Hkv={Hkv} D={D}"
    qkv, _, _, grads = _qk_inputs(T, H3, D, dtype, False, T + H3 + D)
    depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(T + D)).to(DEV)
    a = qkv.clone().requires_grad_(True)
    q, k, v, ws = _prep_form(form, a, depth, D, Hq, Hkv, dtype)
    assert torch.equal(v, qkv[:, Hq + Hkv:])
    buf = grads.clone()
    inp = torch.autograd.grad([q, k, v], [a] + ws, [buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]], retain_graph=True)
    assert inp[0].data_ptr() == buf.data_ptr(), label + ": the backward did not hand the gradient buffer on"
    sep = [grads[:, :Hq].clone(), grads[:, Hq:Hq + Hkv].clone(), grads[:, Hq + Hkv:].clone()]         # three tensors of their own
    out = torch.autograd.grad([q, k, v], [a] + ws, sep)
    assert out[0].shape == (T, H3, D) and out[0].data_ptr() not in [buf.data_ptr()] + [s.data_ptr() for s in sep]
    assert len(inp) == len(out) == 1 + len(ws)
    for x, y in zip(inp, out):
        assert torch.equal(x, y), label + ": the in-place backward differs from the gathered one"
    assert torch.equal(inp[0][:, Hq + Hkv:], grads[:, Hq + Hkv:]), label + ": v's gradient slice changed"
    if form == "none":
        assert torch.equal(inp[0], grads), label + ": a layer without rotation changed a gradient"
    else:
        assert not torch.equal(inp[0][:, :Hq + Hkv], grads[:, :Hq + Hkv]), label + ": the q / k gradients came back untransformed"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,NH,D", [(5462, 3, 128), (16390, 4, 128), (10923, 3, 64), (32771, 4, 64)])
def test_qk_norm_rope_grid_stride_backward(T, NH, D, dtype):
    """The smallest unit count per form (HPL 1 / 4 x D 128 / 64) above one pass of the 1024 workgroups, with a ragged tail: the second
    pass runs the clamped, not-live units, and dw accumulates across the passes (n = T NH in its bound)."""
    worst = {}
    _qk_case(T, NH, D, dtype, True, 1e-6, worst)
    _report(f"qk_norm_rope_grid_stride T={T} NH={NH} D={D}", dtype, worst)


# ------------------------------------------------------------------------------------------------ SwiGLU / GeGLU
GLU = {"swiglu": (ops.swiglu, ops.swiglu_fused, R.swiglu_ref), "geglu": (ops.geglu, ops.geglu_fused, R.geglu_ref)}


def _glu_case(kind, g, u, dy, dtype, fused, worst, label):
    sep, fus, ref = GLU[kind]
    C = g.shape[1]
    if fused:                                               # gate | up side by side: ld = 2C, and the gradients come back the same way
        gu = torch.cat([g, u], 1).requires_grad_(True)
        y = fus(gu)
        run = lambda keep: (lambda d: (d[:, :C], d[:, C:]))(torch.autograd.grad(y, gu, dy, retain_graph=keep)[0])
    else:
        ga, ua = g.clone().requires_grad_(True), u.clone().requires_grad_(True)
        y = sep(ga, ua)
        run = lambda keep: torch.autograd.grad(y, [ga, ua], dy, retain_graph=keep)
    dg, du = run(True)
    for t in (y, dg, du):
        assert bool(torch.isfinite(t).all()), label
    _merge(worst, R.check_all(kind, {"y": y, "dg": dg, "du": du}, ref(g, u, dy, dtype), label))
    for a, b in zip((dg, du), run(False)):
        assert torch.equal(a, b), label + ": a repeated backward differs"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
def test_glu(kind, fused, dtype):
    worst = {}
    for rows, C in ((1, 8), (5, 72), (37, 1000)):
        g, u, dy = _dev(R.rows(rows, C, dtype, rows + C), R.randn((rows, C), dtype, C), R.randn((rows, C), dtype, C + 1))
        _glu_case(kind, g, u, dy, dtype, fused, worst, f"{kind} rows={rows} C={C} fused={fused}")
    _report(kind + (" fused" if fused else ""), dtype, worst)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
def test_glu_grid_stride(kind, fused):
    """1030 x 8192 = 8 437 760 elements: more groups of 8 than one pass of 4096 workgroups x 256 lanes."""
    worst, (rows, C) = {}, (1030, 8192)
    g, u, dy = _dev(R.rows(rows, C, BF, 1), R.randn((rows, C), BF, 2), R.randn((rows, C), BF, 3))
    _glu_case(kind, g, u, dy, BF, fused, worst, f"{kind} rows={rows} C={C} fused={fused}")
    _report(kind + " grid_stride" + (" fused" if fused else ""), BF, worst)


@pytest.mark.parametrize("dtype", [F32, F16])
def test_swiglu_over_the_gate_range(dtype):
    """Gates over +-100 and around the overflow of exp(-x) (x < -88.7 in fp32), up to +-1e4 (f16: +-6e4): everything finite, every
    element within its bound."""
    g = R.gate_range(dtype)
    u, dy = (R.randn(g.shape, F32, s).clamp(-1, 1).to(dtype) for s in (1, 2))
    worst = {}
    _glu_case("swiglu", *_dev(g, u, dy), dtype, False, worst, "swiglu gate range")
    _report("swiglu_gate_range", dtype, worst)


# ------------------------------------------------------------------------------------------------ dta_sum_slabs, flat form past one grid
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("extra", [False, True])
def test_sum_slabs_flat_grid_stride(extra, dtype):
    """2 slabs of 4100 x 2048 = 8 396 800 outputs: more groups of 4 than one pass of 8192 workgroups x 256 lanes; the float64 criterion
    of test_gpu_rowops.py::test_sum_slabs_is_the_float64_sum_rounded_once.  Among 8.4 M sums of cancelling terms one lands in f16's
    subnormal range (-4.3e-6 with this seed), where ONE rounding costs up to half the subnormal spacing, 2^-25, whatever |want| is: the
    rounding term is max(eps |want|, 2^-25) for f16 - the exact fp32 sum rounded once on the CPU misses the criterion without it."""
    g = torch.Generator().manual_seed(7)
    part = torch.randn(2, 4100, 2048, generator=g).to(DEV)
    ex = torch.randn(4100, 2048, generator=g).to(DEV) if extra else None
    got = ops.sum_slabs(part, dtype, ex)
    want64 = part.double().sum(0) + (ex.double() if extra else 0.0)
    assert got.shape == part.shape[1:] and got.dtype == dtype
    eps = {BF: 2 ** -8, F16: 2 ** -11, F32: 2 ** -23}[dtype]
    rounding = (eps * want64.abs()).clamp_min(2.0 ** -25 if dtype == F16 else 0.0)
    bound = rounding + 1e-6 * part.abs().double().sum(0) + 1e-30
    assert bool(((got.double() - want64).abs() <= bound).all())
    assert torch.equal(got, ops.sum_slabs(part, dtype, ex))
