"""head_dim 64 through every layer on the GPU: the head-norm + RoPE kernels (alone and through the fused q/k/v preparation)
against the fp32 torch restatement, an UNMODIFIED transformers.Qwen2ForCausalLM at the Qwen2.5-0.5B head geometry (14 / 2
heads, D = 64) through TreeTrainingEngine in packed and stack mode against the reference fixture tests/golden/engine_qwen2_d64.pt,
and a Qwen3TreeLM with head norms at D = 64 in fp32 against the oracle's gradients."""
import numpy as np
import pytest
import torch

import cases
import hostmirror
import test_qwen2_d64_fixture as fx
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo
from oracle import trie_oracle as to
from test_gpu_engine import REF_BF16_BOUND, REF_BF16_MEDIAN
from test_gpu_rowops import _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64


def _pair(fn_gpu, fn_ref, inputs, dtype):
    """Values and input gradients of the kernel vs the fp32 restatement: the bounds of tests/test_gpu_rowops.py and, which its _pair
    does not have, 1e-5 for the fp32 cases here (so this one stays)."""
    g = torch.Generator().manual_seed(0)
    gi = [x.detach().to(dtype).to(DEV).requires_grad_(True) for x in inputs]
    ri = [x.detach().to(dtype).float().requires_grad_(True) for x in inputs]
    yg = fn_gpu(*gi); yr = fn_ref(*ri)
    do = torch.randn(yr.shape, generator=g).to(dtype)
    yg.backward(do.to(DEV)); yr.backward(do.float())
    tol = {torch.bfloat16: 8e-3, torch.float16: 2e-3, torch.float32: 1e-5}[dtype]
    assert _rel(yg, yr) <= tol
    for a, b in zip(gi, ri):
        assert _rel(a.grad, b.grad) <= (max(tol, 1e-5) if dtype == torch.float32 else (1e-2 if a.dim() == 1 else tol)), a.shape


# ------------------------------------------------------------------------------------------------ head-norm + RoPE
@pytest.mark.parametrize("T,NH,norm,dtype", [(1, 1, True, torch.bfloat16), (33, 14, True, torch.bfloat16), (257, 8, True, torch.float16),
                                             (50, 2, False, torch.bfloat16), (129, 14, False, torch.float16), (70, 4, True, torch.float32)])
def test_qk_norm_rope_d64(T, NH, norm, dtype):
    """cos/sin rows {cos[32], sin[32]}, rotate-half partner i + 32, RMS mean over 64, dw rows 64 wide; 4-head groups and single heads."""
    g = torch.Generator().manual_seed(T * 7 + NH)
    x = torch.randn(T, NH, D, generator=g); w = (1 + 0.2 * torch.randn(D, generator=g)).to(dtype) if norm else None
    cs = ops.rope_cos_sin(torch.randint(0, 16384, (T,), generator=g), D, 1e6)
    ref = lambda a, b=None: hostmirror._cpu_qk_norm_rope(a, b, cs.float(), 1e-6)
    if norm:
        _pair(lambda a, b: ops.qk_norm_rope(a, b, cs.to(DEV), 1e-6), ref, [x, w], dtype)
    else:
        _pair(lambda a: ops.qk_norm_rope(a, None, cs.to(DEV), 1e-6), ref, [x], dtype)


@pytest.mark.parametrize("T,Hq,Hkv,norm,dtype", [(1, 2, 1, True, torch.bfloat16), (300, 14, 2, False, torch.bfloat16),
                                                  (129, 14, 2, True, torch.float16), (77, 8, 4, True, torch.float32)])
def test_qkv_prep_d64(T, Hq, Hkv, norm, dtype):
    """The fused preparation: q/k read in place from [T, Hq+2Hkv, 64], one gradient buffer; and the in-place backward on the
    attention's gradient layout gives the same bits as three separate gradient tensors."""
    g = torch.Generator().manual_seed(T + Hq)
    qkv = torch.randn(T, Hq + 2 * Hkv, D, generator=g)
    ws = [(1 + 0.2 * torch.randn(D, generator=g)) for _ in range(2)] if norm else []
    cs = ops.rope_cos_sin(torch.randint(0, 16384, (T,), generator=g), D, 1e6)

    def glue(fn, csx):
        def f(a, *w):
            q, k, v = fn(a, w[0] if w else None, w[1] if w else None, csx, 1e-6, Hq, Hkv)
            return torch.cat([q, 2.0 * k, 0.5 * v], dim=1)
        return f
    _pair(glue(ops.qkv_prep, cs.to(DEV)), glue(hostmirror._cpu_qkv_prep, cs.float()), [qkv] + ws, dtype)
    grads = torch.randn(T, Hq + 2 * Hkv, D, generator=g).to(dtype).to(DEV)
    res = []
    for fused in (False, True):
        a = qkv.to(dtype).to(DEV).requires_grad_()
        wd = [w.to(dtype).to(DEV).requires_grad_() for w in ws] or [None, None]
        q, k, v = ops.qkv_prep(a, wd[0], wd[1], cs.to(DEV), 1e-6, Hq, Hkv)
        buf = grads.clone()
        views = (buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:])
        torch.autograd.backward([q, k, v], list(views) if fused else [t.clone() for t in views])
        res.append([a.grad] + [w.grad for w in wd if w is not None])
    for x, y in zip(*res):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("mode,bs", [("packed", 2048), ("stack", 64), ("stack", 2048)])
def test_unmodified_qwen2_d64_through_the_engine_on_the_gpu(mode, bs):
    """transformers.Qwen2ForCausalLM with head_dim 64 and 14 / 2 heads (q/k/v biases, no q/k norm), bf16 on the HIP kernels, against the
    REFERENCE engine's fp32 run (engine_qwen2_d64.pt), with the tolerances of
    test_gpu_engine.test_unmodified_huggingface_model_through_the_engine_on_the_gpu.  The stack mode's grad-KV stacks are fp32
    (accumulate == 2 in the dK/dV kernel)."""
    pytest.importorskip("transformers")
    hf = fx.hf_qwen2_d64().to(device=DEV, dtype=torch.bfloat16).train()
    g = fx.gold()
    gold_grads = fx.gold_grads(g)
    assert any(n.endswith("k_proj.bias") for n in gold_grads) and not any("q_norm" in n for n in gold_grads)
    seqs = synth.as_tensors(synth.make_case(fx.QWEN2_D64_DATA))
    maxlen = max(map(len, seqs))
    t = TokenTrie(seqs); t.forward_permute()
    out = TreeTrainingEngine(hf.config, DEV, torch.bfloat16, maxlen, forward_only=True).forward(hf, t)
    for a, b in zip(out, g["fwd_forward"]):
        assert a.dtype == torch.float32 and a.shape == b.shape
        assert (a.cpu() - b).abs().max() < 0.08 and (a.cpu() - b).abs().mean() < 0.015
    t = TokenTrie(seqs, fx.att(len(seqs))); t.backward_permute()
    e = TreeTrainingEngine(hf.config, DEV, torch.bfloat16, maxlen); e.mode = mode
    loss = e.backward(hf, t, mo.default_loss, bs)
    assert e.last_mode.startswith(mode)
    assert abs(loss - g["bwd_bs2048_loss"]) < 1e-2 * abs(loss)
    named = dict(hf.named_parameters())
    assert set(gold_grads) <= set(named)
    ratios = {n: mo.grad_ratio(gold_grads[n], named[n].grad.float().cpu()) for n in gold_grads}
    assert max(ratios.values()) <= REF_BF16_BOUND, max(ratios.items(), key=lambda kv: kv[1])
    assert float(np.median(list(ratios.values()))) <= REF_BF16_MEDIAN


@pytest.mark.parametrize("mode,bs", [("packed", 2048), ("stack", 64)])
def test_qwen3_treelm_d64_fp32_vs_oracle(mode, bs):
    """Qwen3TreeLM with head_dim 64 (per-head q/k RMSNorm on: the D = 64 head-norm kernels with weights) in fp32 on the HIP path
    against the oracle's fp32 gradients (oracle/model_oracle.py, D-generic)."""
    cfg = dict(cases.TINY_CFGS["d128"], head_dim=64, num_attention_heads=6, num_key_value_heads=2)
    case = cases.engine_cases()["d128_minitau"]
    w = mo.init_weights(cfg, seed=case["wseed"])
    seqs = synth.make_case(case["data"])
    att = lambda: fx.att(len(seqs))
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    t_o = to.TokenTrieOracle([np.asarray(s, dtype=np.int64) for s in seqs], att()); t_o.backward_permute()
    loss_o = mo.StackEngineOracle(cfg, wo, max(map(len, seqs))).backward(t_o, mo.default_loss, 2048)
    model = Qwen3TreeLM.from_named(cfg, w, DEV, torch.float32)
    t = TokenTrie(synth.as_tensors(seqs), att()); t.backward_permute()
    e = TreeTrainingEngine(model.config, DEV, torch.float32, max(map(len, seqs))); e.mode = mode
    loss = e.backward(model, t, mo.default_loss, bs)
    assert e.last_mode.startswith(mode)
    assert abs(loss - float(loss_o)) <= 1e-5 * abs(float(loss_o))
    ratios = {n: mo.grad_ratio(wo[n].grad, p.grad.cpu()) for n, p in model.named_parameters()}
    assert any("q_norm" in n for n in ratios)
    worst = max(ratios.items(), key=lambda kv: kv[1])
    assert worst[1] <= 1e-4, worst
