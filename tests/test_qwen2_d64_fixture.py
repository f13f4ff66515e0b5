"""Qwen2 at head_dim 64 (the Qwen2.5-0.5B head geometry: 14 query / 2 kv heads, a GQA group of 7, q/k/v biases, no q/k head
norm, tied head): the tiny configuration behind tests/golden/engine_qwen2_d64.pt (scripts/make_golden.py qwen2_d64, the
REFERENCE engine in fp32 on the CPU), its fixture checks, and the product engine on the CPU stand-ins against it.
tests/test_gpu_engine_d64.py runs the same model on the HIP kernels."""
import functools
import os

import pytest
import torch

import cases
import family
from dynamictreeattn_amd import synth
from family import att  # noqa: F401  (re-exported: the GPU tests read it here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(GOLD, "engine_qwen2_d64.pt")

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


def gold():
    return torch.load(FIXTURE, weights_only=True)


gold_grads = functools.partial(family.gold_grads, key="bwd_bs2048_grads_fp16_scaled")      # this fixture's gradients are the engine run's


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
    family.check_cpu_engine_matches_fixture(hf_qwen2_d64(), synth.as_tensors(synth.make_case(QWEN2_D64_DATA)), gold(), monkeypatch,
                                            fwd_key="fwd_forward", loss_key="bwd_bs2048_loss", grads_key="bwd_bs2048_grads_fp16_scaled",
                                            mode=None, atol=2e-5, loss_rtol=2e-5, norm_rtol=2e-5)
