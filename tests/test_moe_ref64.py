"""The float64 mixture-of-experts references of tests/moe_ref64.py checked on the CPU: block_ref against transformers'
Qwen3MoeSparseMoeBlock, permute_ref with dropped ids against a plain loop, and the two conditions the GPU tests put on their generated
inputs (routing_safe_rows keeps two thirds of the rows of every block case; 85 % of the router rows have the top-k margin)."""
import pytest
import torch

import moe_ref64 as R

DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.mark.parametrize("norm", [True, False])
def test_block_ref_against_transformers(norm, monkeypatch):
    """Output and the four gradients of block_ref within 1e-12 (relative Frobenius) of HF's block in float64, with the ids HF chose.
    HF's router forms its softmax with dtype=torch.float whatever the model's dtype, which alone would cap the agreement near 1e-7: for
    this comparison that one cast is lifted to float64 (the softmax the module calls is handed float64 as its dtype); every other line
    of the block runs as transformers wrote it."""
    transformers = pytest.importorskip("transformers")
    from transformers.models.qwen3_moe import modeling_qwen3_moe as M
    E, k, H, I, T = 12, 3, 48, 32, 37
    c = transformers.Qwen3MoeConfig(hidden_size=H, moe_intermediate_size=I, num_experts=E, num_experts_per_tok=k, norm_topk_prob=norm)
    c._experts_implementation = "eager"
    block = M.Qwen3MoeSparseMoeBlock(c).double()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        block.gate.weight.copy_(torch.randn(E, H, generator=g, dtype=torch.float64) * 2 / H ** 0.5)
        block.experts.gate_up_proj.copy_(torch.randn(E, 2 * I, H, generator=g, dtype=torch.float64) / H ** 0.5)
        block.experts.down_proj.copy_(torch.randn(E, H, I, generator=g, dtype=torch.float64) / I ** 0.5)
    h = torch.randn(T, H, generator=g, dtype=torch.float64)
    dout = torch.randn(T, H, generator=g, dtype=torch.float64)
    softmax = torch.nn.functional.softmax
    monkeypatch.setattr(torch.nn.functional, "softmax", lambda x, dim=None, dtype=None, **kw: softmax(x, dim=dim, dtype=torch.float64, **kw))
    hh = h.clone().requires_grad_(True)
    _, _, ids = block.gate(hh)
    out_hf = block(hh[None])[0]
    out_hf.backward(dout)
    monkeypatch.undo()
    hf = [out_hf.detach(), hh.grad, block.gate.weight.grad, block.experts.gate_up_proj.grad, block.experts.down_proj.grad]
    assert len(set(ids.reshape(-1).tolist())) > 1 and ids.shape == (T, k)
    leaves = [t.detach().clone().requires_grad_(True) for t in (h, block.gate.weight, block.experts.gate_up_proj, block.experts.down_proj)]
    out = R.block_ref(*leaves, ids, norm)
    out.backward(dout)
    for name, a, b in zip(("out", "dh", "d router_w", "d gate_up_w", "d down_w"), [out.detach()] + [t.grad for t in leaves], hf):
        assert a.dtype == torch.float64 and b.dtype == torch.float64 and a.shape == b.shape, name
        assert float(b.norm()) > 0 and float((a - b).norm() / b.norm()) <= 1e-12, (name, float((a - b).norm() / b.norm()))


@pytest.mark.parametrize("T,k,E", [(300, 2, 60), (5, 3, 4), (1, 1, 1)])
def test_permute_ref_with_dropped_ids(T, k, E):
    ids = R.dropped_ids(T, k, E)
    offs, rop, src = R.permute_ref(ids, E)
    rows = [[] for _ in range(E)]                       # the naive restatement: pairs in order, appended to their expert's list
    for p, e in enumerate(ids.reshape(-1).tolist()):
        if 0 <= e < E:
            rows[e].append(p)
    flat = [p for r in rows for p in r]
    n_valid = len(flat)
    assert 0 < n_valid < T * k or T == 1
    want_off = [0]
    for r in rows:
        want_off.append(want_off[-1] + len(r))
    want_rop = [-1] * (T * k)
    for row, p in enumerate(flat):
        want_rop[p] = row
    assert offs.tolist() == want_off and int(offs[E]) == n_valid
    assert rop.tolist() == want_rop
    assert src[:n_valid].tolist() == [p // k for p in flat]


def test_permute_ref_all_valid_unchanged():
    """All ids valid: the sort, the inverse and the offsets of the one-line argsort form."""
    import numpy as np
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 9, (77, 3), generator=g)
    offs, rop, src = R.permute_ref(ids, 9)
    order = np.argsort(ids.reshape(-1).numpy(), kind="stable")
    assert src.tolist() == (order // 3).tolist() and rop[order].tolist() == list(range(77 * 3))
    assert offs.tolist() == [0] + np.cumsum(np.bincount(ids.reshape(-1).numpy(), minlength=9)).tolist()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.BLOCK_SHAPES)
def test_routing_safe_rows_keeps_enough_rows(shape, dtype):
    T, H, I, E, k = shape
    h, router_w = R.block_inputs(*shape, dtype)[:2]
    safe = R.routing_safe_rows(h, router_w, k, dtype)
    assert safe.shape == (T,) and safe.dtype == torch.bool
    print(f"routing_safe_rows {shape} {dtype}: {int(safe.sum())} of {T}")
    assert int(safe.sum()) >= R.SAFE_SHARE * T
    if k == E:
        assert bool(safe.all())
    else:                                   # a kept row's gap survives any perturbation within the bound: move every logit by its bound
        hd, wd = h.double(), router_w.double()
        logits = hd @ wd.t()
        err = R.U[dtype] * logits.abs() + R.C32 * H ** 0.5 * R.U32 * (hd.abs() @ wd.abs().t())
        top = torch.topk(logits, k, dim=-1).indices
        sign = torch.ones_like(logits).scatter_(1, top, -1.0)           # push the selected down and the others up
        moved = torch.topk(logits + sign * err, k, dim=-1).indices
        assert torch.equal(moved.sort(-1).values[safe], top.sort(-1).values[safe])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,k", R.ROUTER_CASES)
def test_router_margin_share(E, k, dtype):
    logits, _ = R.router_logits(E, k, dtype)
    margin = R.router_ref(logits, k, True)[4]
    n = int((margin > R.MARGIN).sum())
    print(f"router margin E={E} k={k} {dtype}: {n} of {R.ROUTER_T}")
    assert n >= R.MARGIN_SHARE * R.ROUTER_T
