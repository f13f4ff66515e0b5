"""The LayerNorm kernels (dta_layernorm_fwd / _bwd) against float64, element by element: every output within the bound
tests/layernorm_ref64.py derives from the kernels' documented arithmetic - at every kernel form (rows of 8 .. 8192 elements: NA 2 / 8 /
16, a ragged last vector group, the largest row), 1 .. 257 rows and a row count that makes the grid stride wrap, bf16 / f16 / fp32
storage, no / one / two deltas, dres and dw_partial given or NULL - with the zero row, the single-element row and the offset row
(8 + 0.05 randn, where a one-pass variance loses rstd) among the rows; repeated calls bit-identical; and ops.add_layer_norm under
autograd hands x and both deltas the same gradient.  The float64 references run on the device.

Each test prints its worst err / bound per output (pytest -s shows them)."""
import itertools
import json

import pytest
import torch

import layernorm_ref64 as L
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
EPS = (1e-5, 1e-6)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def _report(name, dtype, worst):
    print(f"\nWORST {name} {str(dtype).split('.')[-1]} " + json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


def _fwd(x, da, db, w, eps):
    R_, H = x.shape
    y, mean, rstd = torch.empty_like(x), torch.empty(R_, dtype=F32, device=x.device), torch.empty(R_, dtype=F32, device=x.device)
    xo = torch.empty_like(x) if da is not None else None
    ops._launch("dta_layernorm_fwd", (x, da, db, w), ptr(x), ptr(da), ptr(db), ptr(w), ptr(xo), ptr(y), ptr(mean), ptr(rstd), R_, H, eps,
                ops._DT[x.dtype])
    return xo, y, mean, rstd


def _bwd(xin, w, dy, dres, mean, rstd, frozen=False):
    """(dx, dw) as ops._LayerNorm.backward forms them: the per-workgroup partials summed by ops.sum_slabs; frozen: no partials."""
    R_, H = xin.shape
    dx = torch.empty_like(xin)
    part = None if frozen else torch.empty(lib().dta_layernorm_bwd_blocks(R_), H, dtype=F32, device=xin.device)
    ops._launch("dta_layernorm_bwd", (xin, w, dy, dres), ptr(xin), ptr(w), ptr(dy), ptr(dres), ptr(mean), ptr(rstd), ptr(dx), ptr(part), R_, H,
                ops._DT[xin.dtype])
    return dx, (None if frozen else ops.sum_slabs(part, w.dtype))


def _case(R_, H, dtype, n_delta, with_dres, eps, worst, backward=True):
    label = f"R={R_} H={H} deltas={n_delta} dres={with_dres} eps={eps}"
    x = L.rows(R_, H, dtype, R_ + H)
    x, da, db, w, dy, dres = _dev(x, L.delta_for(x, H + 1) if n_delta >= 1 else None, L.delta_for(x, H + 5) if n_delta >= 2 else None,
                                  L.R.norm_weight(H, dtype, H, False), L.R.randn((R_, H), dtype, H + 2),
                                  L.R.randn((R_, H), dtype, H + 3) if with_dres else None)
    xo, y, mean, rstd = _fwd(x, da, db, w, eps)
    xin = xo if n_delta else x
    if n_delta:                                       # x_out first: it is the input the norm's reference takes
        _merge(worst, L.check_all("layernorm", {"x_out": xo}, L.layernorm_fwd_ref(x, da, db, w, eps, dtype), label))
    _merge(worst, L.check_all("layernorm", {"y": y, "mean": mean, "rstd": rstd}, L.layernorm_fwd_ref(x, da, db, w, eps, dtype, xin=xin), label))
    again = _fwd(x, da, db, w, eps)
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip((xo, y, mean, rstd), again)), label + ": a repeated forward differs"
    if not backward:
        return
    dx, dw = _bwd(xin, w, dy, dres, mean, rstd)
    _merge(worst, L.check_all("layernorm", {"dx": dx, "dw": dw}, L.layernorm_bwd_ref(xin, w, dy, dres, eps, dtype), label))
    dx2, dw2 = _bwd(xin, w, dy, dres, mean, rstd)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2), label + ": a repeated backward differs"
    assert torch.equal(_bwd(xin, w, dy, dres, mean, rstd, frozen=True)[0], dx), label + ": dx of the frozen-weight call differs"
    return x, da, db, w, dy, dres, xo, y, dx, dw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 64, 120, 1024, 1032, 2048, 2056, 4096, 4104, 8184, 8192])
def test_layernorm_every_form(H, dtype):
    """R in {1, 3, 4, 65, 257} x no / one / two deltas x dres NULL / given; dw wanted and not (inside _case)."""
    worst = {}
    for i, (R_, n_delta, with_dres) in enumerate(itertools.product((1, 3, 4, 65, 257), (0, 1, 2), (False, True))):
        _case(R_, H, dtype, n_delta, with_dres, EPS[(i + i // 3) % 2], worst)
    _report(f"layernorm H={H}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R_,H,backward", [(8197, 64, True), (32771, 8, False)])
def test_layernorm_grid_stride(R_, H, backward, dtype):
    """More rows than one pass of the capped grid (backward 2048 x 4, forward 8192 x 4), ragged: some waves take a pass more than
    others, and dw sums the passes of every workgroup (n = R in its bound)."""
    worst = {}
    for i, (n_delta, with_dres) in enumerate([(0, False), (2, True)]):
        _case(R_, H, dtype, n_delta, with_dres, EPS[i], worst, backward=backward)
    _report(f"layernorm_grid_stride R={R_}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [120, 8192])
def test_operator_matches_the_entry_bitwise_and_both_deltas_share_the_gradient(H, dtype):
    """ops.layer_norm / ops.add_layer_norm through autograd: the bits of the checked entry-point calls, whether the weight wants a
    gradient or not; x, delta_a and delta_b receive the same gradient."""
    for n_delta in (0, 1, 2):
        x, da, db, w, dy, dres, xo, y, dx, dw = _case(6, H, dtype, n_delta, n_delta > 0, 1e-5, {})
        for frozen in (False, True):
            xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(not frozen)
            ds = [d.clone().requires_grad_(True) for d in (da, db) if d is not None]
            wl = [] if frozen else [wa]
            if n_delta:
                xo2, y2 = ops.add_layer_norm(xa, *(ds + [None])[:2], wa, 1e-5)
                grads = torch.autograd.grad([xo2, y2], [xa] + ds + wl, [dres, dy])
                assert torch.equal(xo2, xo)
            else:
                y2 = ops.layer_norm(xa, wa, 1e-5)
                grads = torch.autograd.grad(y2, [xa] + wl, dy)
            assert torch.equal(y2, y)
            for g in grads[:1 + n_delta]:
                assert torch.equal(g, dx)
            assert frozen or torch.equal(grads[-1], dw)


def test_the_offset_row_keeps_its_rstd():
    """The row the two-pass statistics are there for, at the width of the models: rstd within RSTD_C u32 (+ the second-order term),
    where E[x^2] - m^2 in fp32 is off by 1e-4 .. 1e-3 relative (test_layernorm_ref64.py)."""
    R_, H = 6, 4096
    for dtype in DTYPES:
        x, w = _dev(L.rows(R_, H, dtype, 3), L.R.norm_weight(H, dtype, 4, False))
        _, _, mean, rstd = _fwd(x, None, None, w, 1e-5)
        ref, bound = L.layernorm_fwd_ref(x, None, None, w, 1e-5, dtype)["rstd"]
        o = L.offset_row_of(R_)
        rel = float((rstd[o].double() - ref[o]).abs() / ref[o])
        print(f"offset row {dtype}: rstd off by {rel:.2e} relative, bound {float(bound[o] / ref[o]):.2e}")
        assert rel <= float(bound[o] / ref[o]) and rel < 2e-6
