"""Llama-3 / Mistral / Mixtral through the engine on the GPU: UNMODIFIED transformers models (tests/test_llama_family_fixture.py:
llama3, llama3 with o_proj / MLP biases, yarn, Mistral with every layer sliding, Mixtral) in packed mode and the block-wise stack walk.

* fp32 against HF's own eager attention in float64 on the card (the protocol of
  test_gpu_engine_window.test_qwen3_layer_types_fp32_against_hf_eager; the fixtures' fp16-packed gradients cannot carry 1e-4): logprobs
  within 1e-4, loss within 1e-5, every gradient within max(1e-4, 1.5 x control) and 1e-3, where the control is the same engine on the
  same model with the feature off (default RoPE, no window, no biases; for Mixtral the dense-MLP model).
* bf16 against the fixtures the reference computed (loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN, logprobs 0.08 / 0.015).
* the gradient name set is the model's named_parameters(); tree equals dense on the device."""
import numpy as np
import pytest
import torch

import test_llama_family_fixture as fx
from dynamictreeattn_amd import dense, synth
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo
from test_gpu_engine import REF_BF16_BOUND, REF_BF16_MEDIAN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("packed", 2048), ("stack", 16)]


def _hf_dense(model, seqs, att):
    """HF's own eager forward / backward per sequence (the reference's dense.py arithmetic: logprobs[:len-1], entropy[:len] - at
    this weight scale the entropy varies along a sequence, so its last row counts): logprobs, loss sum; grads in .grad."""
    lps, total = [], 0.0
    for s, a in zip(seqs, att):
        ids = s.to(DEV)[None]
        logits = model(input_ids=ids, use_cache=False).logits[0]
        lsm = torch.log_softmax(logits if logits.dtype == torch.float64 else logits.float(), -1)
        lp, ent = lsm[:-1].gather(-1, ids[0, 1:, None])[:, 0], -(lsm.exp() * lsm).sum(-1)
        loss = mo.default_loss(lp, ent, a)
        loss.backward()
        total += float(loss.detach())
        lps.append(lp.detach().float().cpu())
    return lps, total


def _seqs(case):
    return synth.as_tensors(fx.seqs_of(case))


def _control_model(case):
    """The model of `case` with the feature off, in fp32: default RoPE / no window / no biases; Mixtral: a MistralForCausalLM (dense MLP)."""
    import transformers
    if case == "mixtral":
        geo = {k: v for k, v in fx.MIXTRAL.items() if not k.startswith("num_local") and k != "num_experts_per_tok"}
        c = transformers.MistralConfig(**geo, max_position_embeddings=256, sliding_window=fx.WINDOW,
                                       rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
        c._attn_implementation = "eager"
        m = transformers.MistralForCausalLM(c)
        w = fx.weights(m, 25, fx.CASE_STD["mixtral"])
        with torch.no_grad():
            for n, p in m.named_parameters():
                p.copy_(w[n])
        return m.float().train()
    if case == "llama3_bias":
        m = transformers.LlamaForCausalLM(fx.hf_config("llama3"))              # the same rope, no bias parameters at all
        w = fx.weights(m, fx.CASES[case][5])
        with torch.no_grad():
            for n, p in m.named_parameters():
                p.copy_(w[n])
        return m.float().train()
    return fx.hf_model(case, off=True)


def _fp32_run(model32, case, mode, monkeypatch):
    """The engine in fp32 on `model32` against HF eager in float64 on the same state dict: (logprob error, loss, reference loss, ratios)."""
    ref = type(model32)(model32.config).double().to(DEV).train()
    ref.load_state_dict({k: v.double() for k, v in model32.state_dict().items()})
    mine = model32.to(DEV)
    seqs = _seqs(case)
    att = fx.att(len(seqs))
    lps, loss_r = _hf_dense(ref, seqs, att)
    t = TokenTrie(seqs); t.forward_permute()
    out = TreeTrainingEngine(mine.config, DEV, torch.float32, max(map(len, seqs)), forward_only=True).forward(mine, t)
    lp_err = max(float((a.cpu() - b).abs().max()) for a, b in zip(out, lps))
    t = TokenTrie(seqs, att); t.backward_permute()
    e = TreeTrainingEngine(mine.config, DEV, torch.float32, max(map(len, seqs))); e.mode = mode
    if mode == "stack":
        monkeypatch.setattr(e, "_stack_block_rows", lambda *a: 16)
    loss = e.backward(mine, t, mo.default_loss, 16)
    assert e.last_mode.startswith(mode), e.last_mode
    rg = dict(ref.named_parameters())
    assert {n for n, p in mine.named_parameters() if p.grad is not None} == set(rg)            # lm_head, o_proj.bias, mlp biases, experts
    return lp_err, loss, loss_r, {n: mo.grad_ratio(rg[n].grad.float(), p.grad) for n, p in mine.named_parameters()}


@pytest.mark.parametrize("mode", ["packed", "stack"])
@pytest.mark.parametrize("case", list(fx.CASES))
def test_fp32_against_hf_eager_in_float64(case, mode, monkeypatch):
    pytest.importorskip("transformers")
    lp_err, loss, loss_r, ratios = _fp32_run(fx.hf_model(case), case, mode, monkeypatch)
    print(f"{case}/{mode}: logprob err {lp_err:.2e}, loss rel {abs(loss - loss_r) / abs(loss_r):.2e}, worst ratio "
          f"{max(ratios.items(), key=lambda kv: kv[1])}")
    assert lp_err < 1e-4
    assert abs(loss - loss_r) <= 1e-5 * abs(loss_r)
    _, _, loss_c, control = _fp32_run(_control_model(case), case, mode, monkeypatch)
    assert abs(loss_c - loss_r) > 1e-5 * abs(loss_r)                  # the feature changes the loss: a pass is not an inert case
    bad = {n: (r, control.get(n)) for n, r in ratios.items() if r > max(1e-4, 1.5 * control.get(n, 0.0))}
    print(f"{case}/{mode}: control worst {max(control.values()):.2e}; above the rule: {bad}")
    assert not bad, bad
    assert max(ratios.values()) <= 1e-3


@pytest.mark.parametrize("mode,bs", MODES)
@pytest.mark.parametrize("case", list(fx.CASES))
def test_bf16_against_the_reference_fixture(case, mode, bs, monkeypatch):
    pytest.importorskip("transformers")
    hf = fx.hf_model(case).to(device=DEV, dtype=torch.bfloat16).train()
    g = fx.gold(case)
    gold_grads = fx.gold_grads(g)
    seqs = _seqs(case)
    maxlen = max(map(len, seqs))
    t = TokenTrie(seqs); t.forward_permute()
    out = TreeTrainingEngine(hf.config, DEV, torch.bfloat16, maxlen, forward_only=True).forward(hf, t)
    err = torch.cat([(a.cpu() - b).abs() for a, b in zip(out, g["fwd_dense"])])
    t = TokenTrie(seqs, fx.att(len(seqs))); t.backward_permute()
    e = TreeTrainingEngine(hf.config, DEV, torch.bfloat16, maxlen); e.mode = mode
    if mode == "stack":
        monkeypatch.setattr(e, "_stack_block_rows", lambda *a, b=bs: b)
    loss = e.backward(hf, t, mo.default_loss, bs)
    assert e.last_mode.startswith(mode), e.last_mode
    named = dict(hf.named_parameters())
    assert {n for n, p in named.items() if p.grad is not None} == set(gold_grads)
    ratios = {n: mo.grad_ratio(gold_grads[n], named[n].grad.float().cpu()) for n in gold_grads}
    print(f"{case}/{mode}: logprob err max {float(err.max()):.4f} mean {float(err.mean()):.4f}, loss rel "
          f"{abs(loss - g['bwd_dense_loss']) / abs(loss):.2e}, ratio max {max(ratios.values()):.4f} median {float(np.median(list(ratios.values()))):.4f}")
    assert float(err.max()) < 0.08 and float(err.mean()) < 0.015
    assert abs(loss - g["bwd_dense_loss"]) < 1e-2 * abs(loss)
    assert max(ratios.values()) <= REF_BF16_BOUND, max(ratios.items(), key=lambda kv: kv[1])
    assert float(np.median(list(ratios.values()))) <= REF_BF16_MEDIAN


def test_tree_equals_dense_on_the_device_llama3():
    """dense.backward (one pass per sequence, the stack form) against engine.backward (one packed pass) on the llama3 case in fp32."""
    pytest.importorskip("transformers")
    seqs = _seqs("llama3")
    att = fx.att(len(seqs))
    a = fx.hf_model("llama3").to(DEV)
    loss_d = dense.backward(a, seqs, att, mo.default_loss)
    b = fx.hf_model("llama3").to(DEV)
    t = TokenTrie(seqs, att); t.backward_permute()
    e = TreeTrainingEngine(b.config, DEV, torch.float32, max(map(len, seqs))); e.mode = "packed"
    loss_t = e.backward(b, t, mo.default_loss, 2048)
    assert abs(loss_t - loss_d) <= 1e-5 * abs(loss_d)
    gd = dict(a.named_parameters())
    ratios = {n: mo.grad_ratio(gd[n].grad, p.grad) for n, p in b.named_parameters()}
    assert max(ratios.values()) <= 1e-4, max(ratios.items(), key=lambda kv: kv[1])
