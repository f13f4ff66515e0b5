"""The GEMM layer of ops.py (`_wgrad`, `_dgrad`, `_Linear` / `ops.linear`, `stack_rows`, the LM head's `_HeadRows` at its large step) against
float64, element by element, on both sides of every row count at which the code changes form:

    _wgrad      8191 rows: the plain product; 8192: the 4-slice split into fp32 slabs; 8193 / 8447: 1 / 255 left-over rows; 64 output tiles
                (the last split shape) and 72 (plain); a result whose dims are no multiple of the 16-byte vector (`.t()` view, not the
                transpose kernel); fp32 (always plain); column slices of wider buffers as operands
    _dgrad      4095 / 4096 rows: the plain product / the cached transposed copy; an `out` that is no multiple of 8 (plain); outside and
                inside a `weight_cache` scope, across an in-place weight update, and for two views that share pointer, shape and version
    ops.linear  y, dx, dw, db against float64 autograd, every `needs_input_grad` combination, stacked q|k|v rows inside a scope with a
                second pass that accumulates
    _HeadRows   8191 rows in chunks of 4096: the first chunk takes the transposed-copy dgrad, the second the plain one; kept and chunked,
                fused and non-fused accumulation of dW, a frozen head
    two steps   an engine call, an in-place update of every weight, a second call on another trie: bit-identical to a fresh model, fresh
                engine and empty caches (bf16, >= 8192 packed rows), and within 1e-4 of the oracle in fp32

References and bounds: tests/linear_ref64.py (float64 on the device; ref64_common.bound, nothing fitted).  Which form ran is ASSERTED by
spying on ops.sum_slabs / ops.transpose_2d, so a threshold that drifts fails here instead of emptying a case.  Every call is repeated and
must be bit-identical.  A form that is one library GEMM is also evaluated as that library call: see `_library_limit`.
tests/test_linear_ref64.py shows on the CPU that the bounds hold for an honest restatement and reject the corruptions a whole-tensor
norm lets through.

Each test prints its worst err / bound (pytest -s shows the WORST lines)."""
import functools
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
import linear_ref64 as R
import logprob_ref64 as L
from ref64_common import bound
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo
from oracle import trie_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
IDS = {BF: "bf16", F16: "f16", F32: "fp32"}


def _name(dtype):
    return IDS[dtype]


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)).to(dtype)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _report(name, dtype, worst):
    print(f"\nWORST {name} {_name(dtype)} " + json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


def _library_limit(what, lib_out, ref, bnd):
    """For a form that is nothing but ONE library GEMM: the library call itself at this shape.  Inside the bound (every case so far): the
    form is held to the bound, limit 1.  Were the library alone over it, the form is held to 1.25 x the library's own worst ratio (another
    tile order) and the figure is printed as a LIBRARY line: a statement about the library, not about ops.py."""
    r = R.ratio(lib_out, ref, bnd)
    if r <= 1.0:
        return 1.0
    print(f"\nLIBRARY {what}: the library call alone is at {r:.3f} x the bound; the form is held to 1.25 x that")
    return 1.25 * r


class _Spy:
    """Counts the calls of ops.<name> (looked up in the module at every call, so the product's own call sites go through it)."""

    def __init__(self, monkeypatch, name):
        self.calls, real = 0, getattr(ops, name)

        def wrapped(*a, **k):
            self.calls += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)


# ------------------------------------------------------------------------------------------------ _wgrad
SMALL = [(256, 512), (72, 200), (100, 36)]                 # (out, in); (100, 36): no multiple of the 16-bit vector
LARGE = [(2048, 2048), (2048, 2304)]                       # 64 tiles of 256 x 256: the last split shape; 72: plain
WGRAD_CASES = [(T, p) for p in SMALL for T in (8191, 8192, 8193, 8447)] + [(8193, p) for p in LARGE]


def _split_expected(T, pair, dtype):
    """Written out, not computed from ops.py's formula: split from 8192 rows on, for 16-bit types, up to 64 output tiles."""
    return dtype != F32 and T >= 8192 and pair != (2048, 2304)


@functools.lru_cache(maxsize=1)
def _wgrad_problem(dtype, T, pair):
    out_f, in_f = pair
    x, dy = _rand((T, in_f), dtype, 7 * T + in_f), _rand((T, out_f), dtype, 11 * T + out_f)
    ref, mag, n = R.wgrad_ref(x, dy)
    return x, dy, ref, bound(ref, mag, n, dtype)


def _wgrad_case(x, dy, ref, bnd, dtype, transposed, split, spy, label):
    out_f, in_f = dy.shape[1], x.shape[1]
    before = spy.calls
    got = ops._wgrad(x, dy, transposed)
    assert spy.calls - before == (1 if split else 0), f"{label}: expected the {'split' if split else 'plain'} form"
    assert got.shape == (out_f, in_f) and got.dtype == dtype
    if transposed:
        V = 16 // got.element_size()
        assert got.is_contiguous() == (out_f % V == 0 and in_f % V == 0), f"{label}: transpose kernel / .t() view"
    limit = 1.0 if split else _library_limit(label, (x.t() @ dy).t() if transposed else dy.t() @ x, ref, bnd)
    worst = R.check("wgrad.split" if split else "wgrad.plain", got, ref, bnd, label, limit)
    assert _same(got, ops._wgrad(x, dy, transposed)), f"{label}: a repeated call differs"
    return worst


@pytest.mark.parametrize("transposed", [False, True], ids=["dyTx", "xTdy"])
@pytest.mark.parametrize("T,pair", WGRAD_CASES, ids=[f"T{T}-{p[0]}x{p[1]}" for T, p in WGRAD_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_wgrad_every_form(dtype, T, pair, transposed, monkeypatch):
    spy = _Spy(monkeypatch, "sum_slabs")
    x, dy, ref, bnd = _wgrad_problem(dtype, T, pair)
    split = _split_expected(T, pair, dtype)
    assert split == (R.takes_split(T, *pair, dtype)), "linear_ref64.takes_split disagrees with the table of this test"
    label = f"_wgrad {_name(dtype)} T={T} {pair[0]}x{pair[1]} transposed={transposed}"
    worst = _wgrad_case(x, dy, ref, bnd, dtype, transposed, split, spy, label)
    print(f"\nWORST {label} ({'split' if split else 'plain'}): {worst:.3f}")


@pytest.mark.parametrize("T", [8191, 8193])
@pytest.mark.parametrize("dtype", [BF, F16], ids=_name)
def test_wgrad_strided_operands(dtype, T, monkeypatch):
    """x and dy as column slices of wider buffers (the layout of a fused q|k|v or gate|up activation): one starts on a 16-byte boundary,
    the other 6 bytes into the row."""
    spy = _Spy(monkeypatch, "sum_slabs")
    bx, bd = _rand((T, 512 + 192), dtype, 21), _rand((T, 256 + 40), dtype, 22)
    for xs, ds in ((64, 3), (3, 32)):
        x, dy = bx[:, xs:xs + 512], bd[:, ds:ds + 256]
        assert not x.is_contiguous() and not dy.is_contiguous() and (x.data_ptr() % 16 == 0) != (dy.data_ptr() % 16 == 0)
        ref, mag, n = R.wgrad_ref(x, dy)
        bnd = bound(ref, mag, n, dtype)
        for transposed in (False, True):
            label = f"_wgrad strided {_name(dtype)} T={T} x@{xs} dy@{ds} transposed={transposed}"
            worst = _wgrad_case(x, dy, ref, bnd, dtype, transposed, T >= 8192, spy, label)
            print(f"\nWORST {label}: {worst:.3f}")


# ------------------------------------------------------------------------------------------------ _dgrad
W_SHAPES = [(264, 520), (260, 520), (1024, 256)]           # (out, in); 260: no multiple of 8 - the plain form at any row count


def _cached_expected(T, wshape, dtype):
    return dtype != F32 and T >= 4096 and wshape[0] % 8 == 0 and wshape[1] % 8 == 0


@pytest.mark.parametrize("T", [4095, 4096])
@pytest.mark.parametrize("wshape", W_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_dgrad_both_forms_outside_and_inside_a_scope(dtype, wshape, T, monkeypatch):
    spy = _Spy(monkeypatch, "transpose_2d")
    out_f, in_f = wshape
    dy, w = _rand((T, out_f), dtype, 31 + T), _rand(wshape, dtype, 32, in_f ** -0.5)
    cached = _cached_expected(T, wshape, dtype)
    label = f"_dgrad {_name(dtype)} T={T} w={out_f}x{in_f}"
    name = "dgrad.cached" if cached else "dgrad.plain"
    worst = {}

    def one(tag, w_now):
        ref, mag, n = R.dgrad_ref(dy, w_now)
        bnd = bound(ref, mag, n, dtype)
        got = ops._dgrad(dy, w_now)
        assert got.shape == (T, in_f) and got.dtype == dtype
        limit = 1.0 if cached else _library_limit(label, dy @ w_now, ref, bnd)
        worst[tag] = R.check(name, got, ref, bnd, f"{label} {tag}", limit)
        return got

    assert not ops._TransposedWeights.cache and ops.weight_cache.depth == 0
    a = one("outside", w)
    assert spy.calls == (1 if cached else 0), f"{label}: expected the {'transposed-copy' if cached else 'plain'} form"
    assert _same(a, ops._dgrad(dy, w)) and not ops._TransposedWeights.cache          # outside a scope: a copy per use, none kept
    with ops.weight_cache():
        n0 = spy.calls
        b = one("inside", w)
        assert _same(b, a) and _same(b, ops._dgrad(dy, w))
        assert spy.calls - n0 == (1 if cached else 0), f"{label}: one copy per weight inside a scope"
        with torch.no_grad():
            w.add_(_rand(wshape, dtype, 33, 0.5 * in_f ** -0.5))          # an optimizer step inside the scope: the product follows the NEW weight
        c = one("updated", w)
        assert not _same(c, a) and spy.calls - n0 == (2 if cached else 0)
    assert not ops._TransposedWeights.cache
    _report(label, dtype, worst)


@pytest.mark.parametrize("order", ["slice_first", "contiguous_first"])
@pytest.mark.parametrize("dtype", [BF, F16], ids=_name)
def test_dgrad_two_views_with_one_pointer_shape_and_version(dtype, order, monkeypatch):
    """`big[:, :C]` (row pitch 2C) and the contiguous [R, C] matrix at the same address share data_ptr, shape, dtype and the version counter
    of their storage and are different matrices: inside one scope each must get ITS OWN transposed copy (the cache key carries the strides)."""
    spy = _Spy(monkeypatch, "transpose_2d")
    T, Rw, C = 4096, 264, 520
    big = _rand((Rw, 2 * C), dtype, 41, C ** -0.5)
    views = {"slice_first": big[:, :C], "contiguous_first": big.view(-1)[:Rw * C].view(Rw, C)}
    v1, v2 = views["slice_first"], views["contiguous_first"]
    assert v1.data_ptr() == v2.data_ptr() and v1.shape == v2.shape and v1._version == v2._version and v1.stride() != v2.stride()
    assert not torch.equal(v1, v2)
    dy = _rand((T, Rw), dtype, 42)
    seq = [views[order]] + [v for k, v in views.items() if k != order]
    worst = {}
    with ops.weight_cache():
        for i, w in enumerate(seq + seq):                     # both views, then both again from the cache
            ref, mag, n = R.dgrad_ref(dy, w)
            worst[f"view{i}"] = R.check("dgrad.cached", ops._dgrad(dy, w), ref, bound(ref, mag, n, dtype), f"stride collision {order} call {i}")
        assert spy.calls == 2, "one transposed copy per view, each reused once"
    _report(f"_dgrad stride collision {order}", dtype, worst)


# ------------------------------------------------------------------------------------------------ ops.linear end to end
LINEAR_CASES = [(8193, 1024, 256), (8193, 256, 1024), (4096, 520, 264)]          # (T, in, out): narrowing (xᵀ·dy), widening, the dgrad threshold


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("T,in_f,out_f", LINEAR_CASES, ids=[f"T{t}-{i}to{o}" for t, i, o in LINEAR_CASES])
@pytest.mark.parametrize("dtype", [BF, F16], ids=_name)
def test_linear_against_float64_autograd(dtype, T, in_f, out_f, bias, monkeypatch):
    slabs, transposes = _Spy(monkeypatch, "sum_slabs"), _Spy(monkeypatch, "transpose_2d")
    x, w = _rand((T, in_f), dtype, 51), _rand((out_f, in_f), dtype, 52, in_f ** -0.5)
    b = _rand((out_f,), dtype, 53, 0.5) if bias else None
    go = _rand((T, out_f), dtype, 54)
    label = f"ops.linear {_name(dtype)} T={T} {in_f}->{out_f} bias={bias}"
    # float64 autograd on the same rounded operands
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if bias else None
    y64 = F.linear(x64, w64, b64)
    y64.backward(go.double())
    refs = {"y": R.fwd_ref(x, w, b), "dx": R.dgrad_ref(go, w), "dw": R.wgrad_ref(x, go), "db": R.bias_grad_ref(go)}
    for k, t in (("y", y64.detach()), ("dx", x64.grad), ("dw", w64.grad)) + ((("db", b64.grad),) if bias else ()):
        assert torch.allclose(refs[k][0], t, rtol=1e-12, atol=1e-12), f"{label}: linear_ref64's {k} is not float64 autograd's"
    bnds = {"y": R.fwd_bound(*refs["y"], dtype)}
    for k in ("dx", "dw", "db"):
        bnds[k] = bound(*refs[k], dtype)
    split = T >= 8192                                          # (4096 rows: the plain weight gradient; both 8193-row shapes have <= 64 tiles)
    worst, first = {}, None
    for need_x, need_w in ((True, True), (True, False), (False, True)):
        xs, ws = x.clone().requires_grad_(need_x), w.clone().requires_grad_(need_w)
        bs = b.clone().requires_grad_(need_w) if bias else None
        s0, t0 = slabs.calls, transposes.calls
        with ops.weight_cache():
            y = ops.linear(xs, ws, bs)
            y.backward(go)
        assert slabs.calls - s0 == (1 if (need_w and split) else 0), f"{label}: weight-gradient form"
        # one transposed copy of w for the dgrad (16-bit, >= 4096 rows) and one transpose of the xᵀ·dy result of the narrowing layout
        assert transposes.calls - t0 == (1 if need_x else 0) + (1 if (need_w and in_f >= 2 * out_f) else 0), f"{label}: dgrad / layout form"
        assert (xs.grad is None) == (not need_x) and (ws.grad is None) == (not need_w) and (bs is None or (bs.grad is None) == (not need_w))
        got = {"y": y.detach(), "dx": xs.grad, "dw": ws.grad, "db": bs.grad if bias else None}
        lib = {"y": lambda: F.linear(x, w, b), "db": lambda: go.sum(0), "dw": lambda: go.t() @ x}
        for k, t in got.items():
            if t is None:
                continue
            library_only = k in ("y", "db") or (k == "dw" and not split)
            limit = _library_limit(f"{label} {k}", lib[k](), refs[k][0], bnds[k]) if library_only else 1.0
            worst[k] = max(worst.get(k, 0.0), R.check(f"linear.{k}", t, refs[k][0], bnds[k], label, limit))
        if first is None:
            first = got
        else:                                                  # what is computed does not depend on what else is asked for
            assert all(t is None or _same(t, first[k]) for k, t in got.items()), f"{label}: results differ between needs_input_grad combinations"
    _report(label, dtype, worst)


@pytest.mark.parametrize("dtype", [BF, F16], ids=_name)
def test_linear_on_stacked_rows_with_a_second_pass(dtype, monkeypatch):
    """w = stack_rows(wq, wk, wv) with 256 / 64 / 64 rows at 8193 packed rows inside one scope: every member's gradient within the bound of its
    row slice of the float64 dw; a second forward / backward of the same stacked weight in the scope (the recomputation pass: the fused copy
    comes from the cache) accumulates to twice the first, and the members' .grad do not overlap."""
    slabs = _Spy(monkeypatch, "sum_slabs")
    T, in_f, rows = 8193, 512, (256, 64, 64)
    x, go = _rand((T, in_f), dtype, 61), _rand((T, sum(rows)), dtype, 62)
    ws = [_rand((r, in_f), dtype, 63 + i, in_f ** -0.5).requires_grad_(True) for i, r in enumerate(rows)]
    wcat = torch.cat([w.detach() for w in ws])
    ry, rw = R.fwd_ref(x, wcat), R.wgrad_ref(x, go)
    by, bw = R.fwd_bound(*ry, dtype), bound(*rw, dtype)
    worst = {}
    with ops.weight_cache():
        w1 = ops.stack_rows(*ws)
        y = ops.linear(x, w1)
        worst["y"] = R.check("stacked.y", y.detach(), ry[0], by, "stacked", _library_limit("stacked y", F.linear(x, wcat), ry[0], by))
        y.backward(go)
        assert slabs.calls == 1
        g1 = [w.grad.clone() for w in ws]
        o = 0
        for i, (w, r) in enumerate(zip(ws, rows)):
            assert w.grad.shape == w.shape
            worst[f"dw{i}"] = R.check("stacked.dw", w.grad, rw[0][o:o + r], bw[o:o + r], f"stacked member {i}")
            o += r
        w2 = ops.stack_rows(*ws)
        assert w2.data_ptr() == w1.data_ptr(), "the second pass of a scope shares the fused copy"
        ops.linear(x, w2).backward(go)
        o = 0
        for i, (w, r) in enumerate(zip(ws, rows)):
            worst[f"2dw{i}"] = R.check("stacked.dw2", w.grad, 2 * rw[0][o:o + r], 2 * bw[o:o + r], f"stacked member {i}, second pass")
            assert _same(w.grad, g1[i] * 2), "the second pass computed other bits than the first"
            o += r
    spans = sorted((w.grad.data_ptr(), w.grad.data_ptr() + w.grad.numel() * w.grad.element_size()) for w in ws)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "the members' .grad overlap"
    keep = [w.grad.clone() for w in ws]
    ws[1].grad.zero_()
    assert _same(ws[0].grad, keep[0]) and _same(ws[2].grad, keep[2])
    _report("ops.linear stacked rows", dtype, worst)


# ------------------------------------------------------------------------------------------------ _HeadRows at the large step
HEAD_T, HEAD_H, HEAD_CHUNK = 4096 + 4095, 64, 4096
FORK_ROWS = [3, 3, 4095, 4096, 4097, 8190]                  # on both sides of row 4096
FORK_TOK = [5, 9, 77, 500, 999, 0]


@functools.lru_cache(maxsize=1)
def _head_problem(dtype, V, kind="gauss"):
    """kind "gauss": Gaussian rows.  "aligned": the rows of a chunk all equal (one row for the first 4096, another for the other 4095), with
    one label and one upstream gradient: the rounding of a dlogits element and of a chunk's product then point the same way in every row
    of the chunk - the input that separates a rounding per chunk from one rounding (tests/test_linear_ref64.py shows it on the CPU)."""
    g = torch.Generator().manual_seed(V)
    W = (torch.randn(V, HEAD_H, generator=g) * 0.2).to(dtype).to(DEV)
    rows = torch.tensor(FORK_ROWS)
    n = (HEAD_T, len(FORK_ROWS), HEAD_T)
    if kind == "gauss":
        h = torch.randn(HEAD_T, HEAD_H, generator=g) * 0.5
        nxt = torch.randint(0, V, (HEAD_T,), generator=g)
        go = [torch.randn(k, generator=g) for k in n]
    else:
        rep = torch.tensor([HEAD_CHUNK, HEAD_T - HEAD_CHUNK])
        h = (torch.randn(2, HEAD_H, generator=g) * 0.5).repeat_interleave(rep, 0)
        nxt = torch.tensor([5, 700]).repeat_interleave(rep, 0)
        go = [torch.full((n[0],), 0.731), torch.zeros(n[1]), torch.full((n[2],), -0.377)]
    fork_ptr = torch.searchsorted(rows, torch.arange(HEAD_T + 1)).to(torch.int32).to(DEV)
    bounds = np.searchsorted(rows.numpy(), np.arange(0, HEAD_T + HEAD_CHUNK, HEAD_CHUNK)).tolist()
    return h.to(dtype).to(DEV), W, nxt.to(DEV), rows.to(DEV), torch.tensor(FORK_TOK).to(DEV), fork_ptr, bounds, [t.to(DEV) for t in go]


@functools.lru_cache(maxsize=2)
def _head_reference(dtype, V, kept, kind="gauss"):
    """Everything float64 of one (dtype, V, kept / chunked): the logits as _HeadRows forms them, the forward's statistics, dlogits with
    their bound, dh and both dW bounds.  Shared by the fused / non-fused cases."""
    h, W, nxt, frows, ftok, fptr, bounds, go = _head_problem(dtype, V, kind)
    step = HEAD_T if kept else HEAD_CHUNK
    logits = torch.empty((HEAD_T, (V + 7) // 8 * 8), dtype=dtype, device=DEV)[:, :V]          # rows on the 8-element pitch the kernels read
    for s in range(0, HEAD_T, step):
        torch.mm(h[s:s + step], W.t(), out=logits[s:s + step])
    lp2 = torch.empty(len(FORK_ROWS), dtype=F32, device=DEV)
    lse, ent, lp = ops.logprob_entropy_fwd_raw(logits, nxt, True, 1.0, fptr, ftok, lp2)
    fwd = L.fwd_ref(logits, nxt, fptr, ftok, 1.0)
    dws = {ch: R.head_dw_ref(h, logits, nxt, fptr, ftok, lse, ent, go[0], go[1], go[2], chunk=ch) for ch in ((None,) if kept else (None, HEAD_CHUNK))}
    gref, gbound = dws[None][2:]
    W64 = W.double()
    dh, mag = gref @ W64, gref.abs() @ W64.abs()
    dh_bound = gbound @ W64.abs() + bound(dh, mag, V, dtype)
    return (lp, lp2, ent), fwd, dh, dh_bound, {ch: v[:2] for ch, v in dws.items()}


def _head_run(problem, kept, need_w):
    h0, W0, nxt, frows, ftok, fptr, bounds, go = problem
    h, W = h0.clone().requires_grad_(True), W0.clone().requires_grad_(need_w)
    a, b, c = ops.lm_head_rows(h, W, nxt, fptr, ftok, frows, bounds, True, HEAD_CHUNK, (1 << 40) if kept else 0)
    ((a * go[0]).sum() + (b * go[1]).sum() + (c * go[2]).sum()).backward()
    return (a.detach(), b.detach(), c.detach()), h.grad, W.grad


@pytest.mark.parametrize("fused", [False, True], ids=["sum", "fused"])
@pytest.mark.parametrize("kept", [True, False], ids=["kept", "chunked"])
@pytest.mark.parametrize("V", [1000, 1004])
@pytest.mark.parametrize("dtype", [BF, F16], ids=_name)
def test_lm_head_rows_at_the_large_step(dtype, V, kept, fused, monkeypatch):
    """dh as tests/test_gpu_logprob_bounds.py::test_public_lm_head_rows_gradient bounds it, dW by linear_ref64.head_dw_ref - with the
    chunk term only for the form that rounds per chunk.  V = 1000: the chunk (or the kept call) of >= 4096 rows multiplies against the
    transposed copy, the 4095-row chunk against W itself; V = 1004 (no multiple of 8): W itself throughout, and logits rows with padding
    behind them (this case found _HeadRows handing the kernels rows on a pitch of 1004 elements, which they refuse)."""
    monkeypatch.setattr(ops, "HEAD_WGRAD_FUSED_ACCUMULATE", fused)
    spy = _Spy(monkeypatch, "transpose_2d")
    h0, W0, nxt, frows, ftok, fptr, bounds, go = _head_problem(dtype, V)
    (lp_r, lp2_r, ent_r), fwd, dh, dh_bound, dws = _head_reference(dtype, V, kept)
    dw, dw_bound = dws[None if (kept or fused) else HEAD_CHUNK]
    label = f"_HeadRows {_name(dtype)} V={V} {'kept' if kept else 'chunked'} {'fused' if fused else 'sum'}"

    def run(need_w):
        n0 = spy.calls
        res = _head_run((h0, W0, nxt, frows, ftok, fptr, bounds, go), kept, need_w)
        assert spy.calls - n0 == (1 if V % 8 == 0 else 0), f"{label}: transposed copies in the backward"
        return res

    outs, gh, gW = run(True)
    assert _same(outs[0], lp_r) and _same(outs[1], lp2_r) and _same(outs[2], ent_r), f"{label}: the forward differs from one kernel call over its logits"
    worst = L.check_all("head", {"logprob": outs[0], "extra_logprob": outs[1], "entropy": outs[2]}, fwd, label)
    assert gh.dtype == dtype and gW.dtype == dtype and gW.shape == W0.shape
    worst["dh"] = R.check("head.dh", gh, dh, dh_bound, label)
    worst["dW"] = R.check("head.dW." + ("kept" if kept else "fused" if fused else "chunks"), gW, dw, dw_bound, label)
    outs2, gh2, gW2 = run(True)
    assert all(_same(a, b) for a, b in zip(outs, outs2)) and _same(gh, gh2) and _same(gW, gW2), f"{label}: a repeated call differs"
    outs3, gh3, gW3 = run(False)                               # a frozen head: no dW, the same dh
    assert gW3 is None and _same(gh, gh3) and all(_same(a, b) for a, b in zip(outs, outs3)), f"{label}: a frozen head changes dh"
    _report(label, dtype, worst)


def test_lm_head_chunk_sum_on_aligned_rows(monkeypatch):
    """With Gaussian rows the dlogits term of head_dw_ref's bound (every element's own bound through |h|, linear in T) leaves a rounding
    per chunk far inside it.  On aligned rows nothing averages out: the non-fused chunk sum is inside the bound WITH the chunk term and
    outside it without, and the fused accumulation (one rounding) is inside without - so a fused form that rounded per chunk fails here."""
    dtype, V = BF, 1000
    problem = _head_problem(dtype, V, "aligned")
    _, fwd, dh, dh_bound, dws = _head_reference(dtype, V, False, "aligned")
    (dw, plain), with_term = dws[None], dws[HEAD_CHUNK][1]
    worst = {}
    for fused in (False, True):
        monkeypatch.setattr(ops, "HEAD_WGRAD_FUSED_ACCUMULATE", fused)
        outs, gh, gW = _head_run(problem, False, True)
        tag = "fused" if fused else "sum"
        worst[f"dh.{tag}"] = R.check("head.aligned.dh", gh, dh, dh_bound, tag)
        worst[f"dW.{tag}/with"] = R.ratio(gW, dw, with_term)
        worst[f"dW.{tag}/plain"] = R.ratio(gW, dw, plain)
        assert _same(gW, _head_run(problem, False, True)[2])
    _report("_HeadRows aligned rows", dtype, worst)
    assert worst["dW.sum/with"] <= 1.0 and worst["dW.fused/plain"] <= 1.0
    assert worst["dW.sum/plain"] > 1.0, "the aligned rows no longer separate a rounding per chunk from one rounding"


# ------------------------------------------------------------------------------------------------ two steps with a weight update between
def _att(n):
    return [{"w_logprobs": -1.0 - 0.01 * i, "w_entropy": 0.1 + 0.003 * i} for i in range(n)]


def _sgd(model, rel=0.05):
    """In place, every parameter: a step along its gradient that moves it by `rel` of its own mean magnitude."""
    with torch.no_grad():
        for n, p in model.named_parameters():
            assert p.grad is not None, n
            lr = rel * float(p.float().abs().mean()) / max(float(p.grad.float().abs().mean()), 1e-30)
            before = p._version
            p.add_(p.grad, alpha=-lr)
            assert p._version > before


def test_two_steps_bf16_equal_a_fresh_model_and_engine_bit_for_bit():
    """Nothing per-weight (a transposed copy, stacked rows, a table, a staging buffer) may outlive an engine call: step 2 after an in-place
    update, on another trie with another row count, equals the same step on a fresh model cloned from the updated weights with empty
    caches and a fresh engine.  Both tries pack >= 8192 rows, so the split weight gradient and the transposed-copy dgrads run."""
    cfg = cases.TINY_CFGS["d128"]
    dtype = BF
    seqs1 = synth.as_tensors(synth.wide(seed=1, V=512, root=32, branches=20, depth=450))
    seqs2 = synth.as_tensors(synth.wide(seed=2, V=512, root=40, branches=23, depth=420))
    m = Qwen3TreeLM.from_named(cfg, mo.init_weights(cfg, seed=3), DEV, dtype)
    e = TreeTrainingEngine(m.config, DEV, dtype, 450); e.mode = "packed"
    t1 = TokenTrie(seqs1, _att(len(seqs1)), device=DEV); t1.backward_permute()
    loss1 = e.backward(m, t1, mo.default_loss, 2048)
    T1 = e.last_packed.plan.T
    assert T1 >= 8192 and np.isfinite(loss1)
    assert not ops._TransposedWeights.cache and not ops._StackRows._cache
    _sgd(m)
    m.zero_grad(set_to_none=True)
    t2 = TokenTrie(seqs2, _att(len(seqs2)), device=DEV); t2.backward_permute()
    loss2 = e.backward(m, t2, mo.default_loss, 2048)
    T2 = e.last_packed.plan.T
    assert T2 >= 8192 and T2 != T1 and e.last_mode.startswith("packed")
    grads2 = {n: p.grad.clone() for n, p in m.named_parameters()}

    fresh = Qwen3TreeLM.from_named(cfg, {n: p.detach().clone() for n, p in m.named_parameters()}, DEV, dtype)
    assert all(_same(p, dict(m.named_parameters())[n]) for n, p in fresh.named_parameters())
    ops.clear_weight_caches()
    e2 = TreeTrainingEngine(fresh.config, DEV, dtype, 450); e2.mode = "packed"
    t3 = TokenTrie(seqs2, _att(len(seqs2)), device=DEV); t3.backward_permute()
    loss3 = e2.backward(fresh, t3, mo.default_loss, 2048)
    print(f"\nWORST two steps bf16: rows {T1} then {T2}, loss {loss1:.6f} then {loss2:.6f} (fresh {loss3:.6f})")
    assert loss2 == loss3 and loss2 != loss1
    diff = [n for n, p in fresh.named_parameters() if not _same(p.grad, grads2[n])]
    assert not diff, f"step 2 differs from a fresh run in {diff}"


def test_two_steps_fp32_follow_the_oracle():
    """The same two steps in fp32 at a few hundred rows against the oracle's stack engine given the updated weights: loss and every
    parameter gradient at the 1e-4 bar of tests/test_gpu_properties.py::test_fp32_engine_equals_the_reference_schedule_on_random_tries."""
    cfg = cases.TINY_CFGS["d128"]
    data = [{"kind": "random_tree", "seed": 22, "n_seq": 9, "max_len": 150, "alphabet": 2, "dup": 2},
            {"kind": "random_tree", "seed": 23, "n_seq": 11, "max_len": 120, "alphabet": 2, "dup": 1}]
    seqs = [synth.make_case(d) for d in data]
    cap = max(len(s) for ss in seqs for s in ss)
    m = Qwen3TreeLM.from_named(cfg, mo.init_weights(cfg, seed=4), DEV, F32)
    e = TreeTrainingEngine(m.config, DEV, F32, cap); e.mode = "packed"
    rows = []
    for step, ss in enumerate(seqs):
        t = TokenTrie(synth.as_tensors(ss), _att(len(ss)), device=DEV); t.backward_permute()
        o = to.TokenTrieOracle([np.asarray(s, dtype=np.int64) for s in ss], _att(len(ss))); o.backward_permute()
        wo = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in m.named_parameters()}          # the oracle gets the SAME (updated) weights
        loss_o = float(mo.StackEngineOracle(cfg, wo, cap).backward(o, mo.default_loss, 2048))
        m.zero_grad(set_to_none=True)
        loss = e.backward(m, t, mo.default_loss, 2048)
        rows.append(e.last_packed.plan.T)
        assert abs(loss - loss_o) <= 1e-5 * max(abs(loss_o), 1.0), (step, loss, loss_o)
        gmax = max(float(v.grad.norm()) for v in wo.values() if v.grad is not None)
        worst = 0.0
        for n, p in m.named_parameters():
            g_o = wo[n].grad if wo[n].grad is not None else torch.zeros_like(wo[n])
            err, lim = float((p.grad.cpu() - g_o).norm()), 1e-4 * float(g_o.norm()) + 1e-6 * gmax
            worst = max(worst, err / lim)
            assert err <= lim, (step, n, err, float(g_o.norm()), gmax)
        print(f"\nWORST two steps fp32 step {step}: rows {rows[-1]}, loss {loss:.6f}, worst parameter err / bar {worst:.3f}")
        _sgd(m)
    assert rows[0] != rows[1] and min(rows) >= 100
