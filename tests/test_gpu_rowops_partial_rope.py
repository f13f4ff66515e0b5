"""The partial RoPE kernel entries (dta_rope_partial_fwd / _bwd), called directly, against float64 element by element: every output
within the bound tests/partial_rope_ref64.py assembles from the RoPE-only terms of tests/rowops_ref64.py, the pass-through elements
R .. D-1 bit for bit, in bf16, f16 and fp32 storage, on rowops_ref64.rows (log-spaced row scales, an all-zero row, a single-element
row) at depths up to 131 072.  Shapes: both head dims; every rotary dimension whose partner distance is a power of two or not (48: 3
lanes, 96: 6) and the edges R = 8 / 16 and R = D; NH 1 / 3 / 4 / 5 / 14 (one head per lane group, and four); 1 / 3 / 37 tokens (a
partial workgroup, several); the backward's second, ragged grid-stride pass; q and k in place from a fused [T, Hq+2Hkv, D] buffer with
the gradients in one buffer and the in-place backward; every output a NaN-filled arena of tests/arena.py whose guard bands, in front and
behind, must keep their bytes.
tests/test_partial_rope_ref64.py shows on the CPU that the bounds hold for an honest emulation and reject four deliberate errors.

Each test prints its worst err / bound per output (pytest -s shows them)."""
import json

import pytest
import torch

import arena as A
import partial_rope_ref64 as PR
import rowops_ref64 as R
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
TAIL = 96                         # guard elements in front of and behind every output
HALF_SPLIT = [16, 32, 48, 64, 96, 112, 128]
INTERLEAVED = [8, 32, 64, 120, 128]
CASES = [(0, D, r) for D in (64, 128) for r in HALF_SPLIT if r <= D] + [(1, D, r) for D in (64, 128) for r in INTERLEAVED if r <= D]
HEADS = (1, 3, 4, 5, 14)


def _merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def _report(name, dtype, worst):
    print(f"\nWORST {name} {str(dtype).split('.')[-1]} " + json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


def _poisoned(name, n, dtype):
    """An output arena of n elements, NaN in the payload and in the guard bands."""
    return A.out_arena(name, (n,), dtype, "A", guard_rows=TAIL, device=DEV)


def _inputs(T, NH, D, rot, dtype, seed):
    x = R.rows(T, NH * D, dtype, seed).view(T, NH, D).to(DEV)
    depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    return x, ops.rope_cos_sin(depth, rot, 1e4), R.randn((T, NH, D), dtype, seed + 3).to(DEV)


def _fwd(x, cs, pairing, label=""):
    """One forward entry call over x [T, NH, D] (any token stride) into a poisoned buffer: y."""
    T, NH, D = x.shape
    n = T * NH * D
    yb = _poisoned("y", n, x.dtype)
    ops._launch("dta_rope_partial_fwd", (x, cs), ptr(x), ptr(cs), yb.ptr(), T, NH, D, cs.shape[1], pairing, x.stride(0), ops._DT[x.dtype])
    yb.assert_guards_intact(label)
    return yb.view.view(T, NH, D)


def _bwd(cs, dy, pairing, label=""):
    """One backward entry call, out of place, into a poisoned buffer: dx."""
    T, NH, D = dy.shape
    n = T * NH * D
    dxb = _poisoned("dx", n, dy.dtype)
    dx = dxb.view.view(T, NH, D)
    ops._launch("dta_rope_partial_bwd", (cs, dy), ptr(cs), ptr(dy), ptr(dx), T, NH, D, cs.shape[1], pairing, dy.stride(0), dy.stride(1),
                dx.stride(0), ops._DT[dy.dtype])
    dxb.assert_guards_intact(label)
    return dx


def _case(T, NH, D, rot, pairing, dtype, worst):
    label = f"T={T} NH={NH} D={D} R={rot} pairing={pairing}"
    x, cs, dy = _inputs(T, NH, D, rot, dtype, T + NH + D + rot)
    y, dx = _fwd(x, cs, pairing, label), _bwd(cs, dy, pairing, label)
    _merge(worst, R.check_all("rope_partial", {"y": y}, PR.fwd_ref(x, cs, pairing, dtype), label))
    _merge(worst, R.check_all("rope_partial", {"dx": dx}, PR.bwd_ref(dy, cs, pairing, dtype), label))
    assert torch.equal(y[..., rot:], x[..., rot:]), label + ": x[..., R:] did not come through bit for bit"
    assert torch.equal(dx[..., rot:], dy[..., rot:]), label + ": dy[..., R:] did not come through bit for bit"
    inplace = dy.clone()                                         # dx is dy: a lane writes exactly the bytes it read
    ops._launch("dta_rope_partial_bwd", (cs, inplace), ptr(cs), ptr(inplace), ptr(inplace), T, NH, D, rot, pairing, inplace.stride(0),
                inplace.stride(1), inplace.stride(0), ops._DT[dtype])
    assert torch.equal(inplace, dx), label + ": the in-place backward differs from the out-of-place one"
    return x, cs, dy, y, dx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing,D,rot", CASES)
def test_rope_partial_every_form(pairing, D, rot, dtype):
    """Every rotary dimension of both pairings x NH 1 / 3 / 4 / 5 / 14 (one head per lane group and four) x T 1 / 3 / 37."""
    worst = {}
    for NH in HEADS:
        for T in (1, 3, 37):
            _case(T, NH, D, rot, pairing, dtype, worst)
    _report(f"rope_partial pairing={pairing} D={D} R={rot}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing,D,NH,rot", [(0, 128, 1, 96), (0, 64, 4, 48), (1, 128, 4, 64), (1, 64, 1, 32)])
def test_rope_partial_grid_stride_backward(pairing, D, NH, rot, dtype):
    """The backward takes at most 1024 workgroups of 4 waves; a wave holds 64 / (D/8) lane groups of HPL heads (4 when NH % 4 == 0, else
    1).  T is one pass of that grid plus a few tokens: the grid-stride loop runs a second, ragged pass."""
    hpl = 4 if NH % 4 == 0 else 1
    heads_per_pass = 1024 * 4 * (64 // (D // 8)) * hpl
    T = heads_per_pass // NH + 3
    assert T * NH > heads_per_pass and (T * NH - heads_per_pass) // hpl < 4 * (64 // (D // 8))       # a second pass of less than one workgroup
    worst = {}
    _case(T, NH, D, rot, pairing, dtype, worst)
    _report(f"rope_partial_grid_stride T={T} D={D} NH={NH} R={rot}", dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing,D,Hq,Hkv,rot", [(0, 128, 4, 2, 96), (0, 64, 3, 1, 48), (0, 128, 24, 8, 96), (0, 64, 14, 2, 32),
                                                  (1, 128, 4, 2, 64), (1, 64, 6, 2, 32), (1, 128, 32, 2, 64), (1, 128, 5, 1, 120)])
def test_qkv_prep_partial_with_the_gradients_in_one_fused_buffer(pairing, D, Hq, Hkv, rot, dtype):
    """ops.qkv_prep_partial: q / k read at the fused buffer's token stride, v a view; with dq, dk, dv side by side in ONE
    [T, Hq+2Hkv, D] buffer the backward runs in place on it - bit-equal to the out-of-place path (separate gradients), the v slice
    untouched - and the autograd path gives the numbers of the raw entries."""
    worst, H3 = {}, Hq + 2 * Hkv
    for T in (1, 5, 37):
        label = f"T={T} Hq={Hq} Hkv={Hkv} D={D} R={rot} pairing={pairing}"
        qkv = R.rows(T, H3 * D, dtype, T + H3 + D).view(T, H3, D).to(DEV)
        depth = torch.randint(0, 131072, (T,), generator=torch.Generator().manual_seed(T)).to(DEV)
        cs, grads = ops.rope_cos_sin(depth, rot, 1e4), R.randn((T, H3, D), dtype, 9).to(DEV)
        a = qkv.clone().requires_grad_(True)
        q, k, v = ops.qkv_prep_partial(a, cs, Hq, Hkv, bool(pairing))
        assert torch.equal(v, qkv[:, Hq + Hkv:]) and v.data_ptr() == a.data_ptr() + (Hq + Hkv) * D * a.element_size()       # a view
        buf = grads.clone()
        (inp,) = torch.autograd.grad([q, k, v], [a], [buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]], retain_graph=True)
        assert inp.data_ptr() == buf.data_ptr(), label + ": the backward did not run in place on the gradient buffer"
        sep = [grads[:, :Hq].clone(), grads[:, Hq:Hq + Hkv].clone(), grads[:, Hq + Hkv:].clone()]     # three tensors of their own
        (out,) = torch.autograd.grad([q, k, v], [a], sep)
        assert out.data_ptr() not in (buf.data_ptr(), sep[0].data_ptr())
        assert torch.equal(inp, out), label + ": the in-place backward differs from the out-of-place one"
        assert torch.equal(inp[:, Hq + Hkv:], grads[:, Hq + Hkv:]), label + ": v's gradient slice changed"
        for lo, NH, o in ((0, Hq, q), (Hq, Hkv, k)):
            xs, gs = qkv[:, lo:lo + NH], grads[:, lo:lo + NH]
            assert torch.equal(o, _fwd(xs, cs, pairing, label)), label + ": the operator differs from the raw forward entry"
            assert torch.equal(inp[:, lo:lo + NH], _bwd(cs, gs, pairing, label)), label + ": the operator's backward differs from the raw entry"
            _merge(worst, R.check_all("qkv_prep_partial", {"y": o}, PR.fwd_ref(xs, cs, pairing, dtype), label))
            _merge(worst, R.check_all("qkv_prep_partial", {"dx": inp[:, lo:lo + NH]}, PR.bwd_ref(gs, cs, pairing, dtype), label))
            assert torch.equal(o[..., rot:], xs[..., rot:]) and torch.equal(inp[:, lo:lo + NH, rot:], gs[..., rot:])
        # ops.rope_partial on one tensor: the same numbers
        b = qkv[:, :Hq].clone().requires_grad_(True)
        y = ops.rope_partial(b, cs, bool(pairing))
        (db,) = torch.autograd.grad(y, [b], grads[:, :Hq])
        assert torch.equal(y, q) and torch.equal(db, inp[:, :Hq]), label + ": ops.rope_partial differs from ops.qkv_prep_partial"
    _report(f"qkv_prep_partial D={D} Hq={Hq} Hkv={Hkv} R={rot} pairing={pairing}", dtype, worst)
