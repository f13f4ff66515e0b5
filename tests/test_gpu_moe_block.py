"""ops.moe_mlp - router GEMM, _MoeRouter, permutation, _MoeLinear (gathered), SwiGLU, _MoeLinear, _MoeCombine - and its whole backward
against moe_ref64.block_ref, the float64 autograd restatement of Qwen3MoeSparseMoeBlock (tests/test_moe_ref64.py holds it to
transformers' block), at shapes that leave one tile: H 144 = 128 + 16 = 2 * 64 + 16 and H 208 = 3 * 64 + 16 (a second n-tile with masked
columns, a k-tail behind full k-steps, in all three GEMM modes), E 130 with k 8 (three router slots per lane), a single token (nine of
twelve experts without a row) and k = E.

Selection.  The ids are the product's own (one ops.linear + ops.moe_router_fwd_raw call on the same inputs - the calls moe_mlp makes),
and block_ref is evaluated with them.  On the rows moe_ref64.routing_safe_rows keeps - at least two thirds of every case - no rounding
of the logits can change the top-k, and the ids must be the float64 top-k.

Bound, 16-bit: relative Frobenius error <= (r + 1) half-spacings of the format (half-spacing U[dtype] / 2: 2^-9 bf16, 2^-12 f16), r
the number of roundings to the model dtype on the tensor's longest path through ops.moe_mlp, counted from ops.py:

    out          r 4   gu (gathered GEMM) -> act (SwiGLU) -> y (down GEMM) -> out (combine); the weights' path is shorter
                       (logits -> w -> out: 3)
    d down_w     r 4   logits -> w -> dy = w * dout (combine backward) -> wgrad; its other operand act carries 2
    d gate_up_w  r 6   w (2) -> dy (3) -> dact (down dgrad, 4) -> dgu (SwiGLU backward, 5) -> wgrad (6)
    d router_w   r 6   y (3) -> dw = <dout, y> (combine backward, 4) -> dlogits (router backward, 5) -> wgrad of ops.linear (6)
    dh           r 8   dgu (5) -> sorted dx (gate/up dgrad, 6) -> scatter-back sum over the k slots (7) -> autograd's sum with the router
                       GEMM's dx (8); that other term carries dlogits (5) -> dx (6)

fp32: 1e-5, the bar tests/test_gpu_fp32.py holds fp32 gradients to.

Largest err / limit observed on the MI355X over the four shapes and both norm_topk_prob settings (for information; no limit is
derived from it; every 16-bit maximum comes from the E 130, k 8 case; no tensor needed a rounding inside block_ref):

    tensor        bf16    f16     fp32
    out           0.74    0.72    0.09
    dh            0.43    0.44    0.10
    d router_w    0.53    0.56    0.10
    d gate_up_w   0.51    0.50    0.09
    d down_w      0.74    0.72    0.09

Beyond the norms: an expert that received no row has an exactly zero d gate_up_w[e] and d down_w[e]; dtypes and shapes of the output
and of every gradient are the inputs'; and a second identical forward + backward gives identical bits everywhere (the layer
recomputation re-runs the block in the backward and depends on it)."""
import functools

import pytest
import torch

import moe_ref64 as R
from dynamictreeattn_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("out", "dh", "d router_w", "d gate_up_w", "d down_w")
ROUNDINGS = {"out": 4, "dh": 8, "d router_w": 6, "d gate_up_w": 6, "d down_w": 4}
FP32_LIMIT = 1e-5


def _limit(name, dtype):
    return FP32_LIMIT if dtype == torch.float32 else (ROUNDINGS[name] + 1) * R.U[dtype] / 2      # ref64_common.U is the doubled half-spacing


def _product(inputs, k, norm):
    """One forward + backward of ops.moe_mlp: (out, dh, d router_w, d gate_up_w, d down_w)."""
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs[:4]]
    out = ops.moe_mlp(*leaves, k, norm)
    out.backward(inputs[4].to(DEV))
    return [out.detach()] + [t.grad for t in leaves]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, norm):
    """Inputs, the product's ids, the product's results and block_ref's, once per case."""
    T, H, I, E, k = shape
    inputs = R.block_inputs(*shape, dtype)
    ids, _, _ = ops.moe_router_fwd_raw(ops.linear(inputs[0].to(DEV), inputs[1].to(DEV)), k, norm)
    ids = ids.cpu().long()
    got = _product(inputs, k, norm)
    leaves = [t.double().requires_grad_(True) for t in inputs[:4]]
    out = R.block_ref(*leaves, ids, norm)
    out.backward(inputs[4].double())
    return inputs, ids, got, [out.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "fp32"])
@pytest.mark.parametrize("shape", R.BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_against_float64(shape, dtype, norm):
    T, H, I, E, k = shape
    inputs, ids, got, ref = _case(shape, dtype, norm)
    safe = R.routing_safe_rows(inputs[0], inputs[1], k, dtype)
    assert int(safe.sum()) >= R.SAFE_SHARE * T
    top64 = torch.topk(inputs[0].double() @ inputs[1].double().t(), k, dim=-1).indices
    assert ids.shape == (T, k) and bool(((ids >= 0) & (ids < E)).all())
    assert torch.equal(ids.sort(-1).values[safe], top64.sort(-1).values[safe]), "the product's top-k on rows no rounding can reorder"
    errs = {}
    for name, a, r, leaf in zip(NAMES, got, ref, (inputs[0],) + inputs[:4]):
        assert a.dtype == dtype and a.shape == leaf.shape == r.shape, name
        assert bool(torch.isfinite(a).all()) and float(r.norm()) > 0, name
        errs[name] = float((a.double().cpu() - r).norm() / r.norm())
    print(f"moe_mlp {shape} {dtype} norm={norm}: " + ", ".join(f"{n} {errs[n]:.3g} ({errs[n] / _limit(n, dtype):.2f} of the limit)" for n in NAMES))
    for name in NAMES:
        assert errs[name] <= _limit(name, dtype), (name, errs[name], _limit(name, dtype))
    rows = torch.bincount(ids.reshape(-1), minlength=E)
    empty = rows == 0
    if T == 1:
        assert int(empty.sum()) == E - k
    for name, a in (("d gate_up_w", got[3]), ("d down_w", got[4])):
        assert bool((a[empty.to(DEV)] == 0).all()), f"{name}: an expert without a row has a gradient"
        assert bool((a[(~empty).to(DEV)].flatten(1).abs().amax(1) > 0).all()), f"{name}: an expert with rows has none"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "fp32"])
@pytest.mark.parametrize("shape", R.BLOCK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_same_bits_on_every_call(shape, dtype):
    inputs, _, got, _ = _case(shape, dtype, True)
    again = _product(inputs, shape[4], True)
    for name, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), f"{name}: two identical calls differ"
