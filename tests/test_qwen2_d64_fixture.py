"""Qwen2 at head_dim 64 (the Qwen2.5-0.5B head geometry: 14 query / 2 kv heads, a GQA group of 7, q/k/v biases, no q/k head
norm, tied head): the tiny configuration behind tests/golden/engine_qwen2_d64.pt (scripts/make_golden.py qwen2_d64, the
REFERENCE engine in fp32 on the CPU), its fixture checks, and the product engine on the CPU stand-ins against it.
tests/test_gpu_engine_d64.py runs the same model on the HIP kernels."""
import os

import pytest
import torch

import cases
import hostmirror
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(GOLD, "engine_qwen2_d64.pt")
CPU = torch.device("cpu")

# head_dim 64 with the 0.5B head counts (q/o projections 896 wide); hidden 16 and intermediate 32 keep the fixture small (~170 KB of
# fp16-packed gradients) - the attention geometry, not the hidden width, is what this configuration is for
QWEN2_D64 = dict(vocab_size=512, hidden_size=16, intermediate_size=32, num_hidden_layers=2, num_attention_heads=14,
                 num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6, rope_theta=1000000.0)
QWEN2_D64_DATA = cases.QWEN2_DATA


def hf_qwen2_d64():
    """transformers.Qwen2ForCausalLM of QWEN2_D64 (explicit head_dim 64) with the seeded weights of cases.qwen2_weights (fp32, eager)."""
    import transformers
    cfg = QWEN2_D64
    c = transformers.Qwen2Config(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                                 num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                                 num_key_value_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], tie_word_embeddings=True,
                                 max_position_embeddings=40960, rms_norm_eps=cfg["rms_norm_eps"],
                                 rope_parameters={"rope_type": "default", "rope_theta": cfg["rope_theta"]})
    c._attn_implementation = "eager"
    m = transformers.Qwen2ForCausalLM(c)
    w = cases.qwen2_weights(cfg, seed=9)
    missing, unexpected = m.load_state_dict({**w, "lm_head.weight": w["model.embed_tokens.weight"]}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    assert m.model.layers[0].self_attn.head_dim == 64
    return m.float().train()


def att(n):
    return [{"w_logprobs": -1.0 - 0.01 * i, "w_entropy": 0.1 + 0.003 * i} for i in range(n)]


def gold():
    return torch.load(FIXTURE, weights_only=True)


def gold_grads(g):
    return {n: q.float() * s_ for n, (q, s_) in g["bwd_bs2048_grads_fp16_scaled"].items()}


def test_qwen2_d64_fixture_names_and_shapes():
    g = gold()
    grads = gold_grads(g)
    L, Hq, Hkv, D, H = (QWEN2_D64[k] for k in ("num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim", "hidden_size"))
    assert set(g) >= {"fwd_forward", "bwd_bs2048_loss", "bwd_dense_loss", "bwd_bs2048_grads_fp16_scaled", "grad_norms"}
    assert not any("q_norm" in n or "k_norm" in n for n in grads)
    for l in range(L):
        p = f"model.layers.{l}.self_attn."
        assert grads[p + "q_proj.weight"].shape == (Hq * D, H) and grads[p + "o_proj.weight"].shape == (H, Hq * D)
        assert grads[p + "q_proj.bias"].shape == (Hq * D,)
        assert grads[p + "k_proj.bias"].shape == (Hkv * D,) and grads[p + "v_proj.bias"].shape == (Hkv * D,)
    assert len(grads) == 2 + 12 * L                                   # embed (tied head), final norm, 12 tensors per layer
    assert abs(g["bwd_bs2048_loss"] - g["bwd_dense_loss"]) < 1e-4 * abs(g["bwd_dense_loss"])
    seqs = synth.make_case(QWEN2_D64_DATA)
    assert len(g["fwd_forward"]) == len(seqs)


def test_qwen2_d64_engine_on_cpu_matches_the_reference_fixture(monkeypatch):
    """The product engine with its device steps replaced by the CPU stand-ins of tests/hostmirror.py (fp32) reproduces the reference
    engine's logprobs, loss and every gradient at head_dim 64 (the host logic sizes everything from D)."""
    pytest.importorskip("transformers")
    hostmirror.install(monkeypatch)
    hf = hf_qwen2_d64()
    g = gold()
    seqs = synth.as_tensors(synth.make_case(QWEN2_D64_DATA))
    maxlen = max(map(len, seqs))
    t = TokenTrie(seqs, device=CPU); t.forward_permute()
    out = TreeTrainingEngine(hf.config, CPU, torch.float32, maxlen, forward_only=True).forward(hf, t)
    for a, b in zip(out, g["fwd_forward"]):
        assert torch.allclose(a, b, atol=2e-5)
    t = TokenTrie(seqs, att(len(seqs)), device=CPU); t.backward_permute()
    loss = TreeTrainingEngine(hf.config, CPU, torch.float32, maxlen).backward(hf, t, mo.default_loss, 2048)
    assert abs(loss - g["bwd_bs2048_loss"]) < 2e-5 * abs(loss)
    named = dict(hf.named_parameters())
    for n, gg in gold_grads(g).items():
        assert mo.grad_ratio(gg, named[n].grad) <= 1e-3, n                   # fp16-packed golden: 5e-4 per element
        assert abs(float(named[n].grad.norm()) - g["grad_norms"][n]) <= 2e-5 * g["grad_norms"][n] + 1e-9, n
