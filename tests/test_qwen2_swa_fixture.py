"""Qwen2 with sliding-window layers: the tiny configuration behind tests/golden/engine_qwen2_swa.pt (scripts/make_golden.py
qwen2_swa: the REFERENCE's dense per-sequence path in fp32 on the CPU, whose HF eager attention applies the sliding-window mask
kv_idx > q_idx - sliding_window) and the checks of the fixture.  Layer 0 attends in full, layers 1 and 2 through a window of 24
tokens (use_sliding_window, max_window_layers = 1) on tau2-shaped sequences of up to ~4 windows whose forks lie both inside and
outside the window.  tests/test_gpu_engine_window.py runs the product engine on it."""
import os

import pytest
import torch

import cases
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import _windows_of
from family import _m, att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden.py read them here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(GOLD, "engine_qwen2_swa.pt")
WINDOW = 24
QWEN2_SWA = dict(vocab_size=512, hidden_size=16, intermediate_size=32, num_hidden_layers=3, num_attention_heads=14,
                 num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6, rope_theta=1000000.0)
QWEN2_SWA_DATA = {"kind": "tau2", "seed": 6, "V": 512, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 128}


def hf_config(cls_name="Qwen2Config", attn="eager"):
    import transformers
    cfg = QWEN2_SWA
    kw = dict(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
              num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
              num_key_value_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], tie_word_embeddings=True,
              max_position_embeddings=40960, rms_norm_eps=cfg["rms_norm_eps"],
              rope_parameters={"rope_type": "default", "rope_theta": cfg["rope_theta"]},
              use_sliding_window=True, sliding_window=WINDOW)
    if cls_name == "Qwen2Config":
        kw["max_window_layers"] = 1
    else:                                                  # Qwen3: the same layers named explicitly
        kw["layer_types"] = ["full_attention"] + ["sliding_attention"] * (cfg["num_hidden_layers"] - 1)
    c = getattr(transformers, cls_name)(**kw)
    c._attn_implementation = attn
    return c


def hf_qwen2_swa(attn="eager"):
    """transformers.Qwen2ForCausalLM of QWEN2_SWA with the seeded weights of cases.qwen2_weights (fp32)."""
    import transformers
    m = transformers.Qwen2ForCausalLM(hf_config("Qwen2Config", attn))
    w = cases.qwen2_weights(QWEN2_SWA, seed=11)
    missing, unexpected = m.load_state_dict({**w, "lm_head.weight": w["model.embed_tokens.weight"]}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    return m.float().train()


def gold():
    return torch.load(FIXTURE, weights_only=True)


def test_qwen2_swa_fixture_names_and_shapes():
    g = gold()
    grads = gold_grads(g)
    L, Hq, Hkv, D, H = (QWEN2_SWA[k] for k in ("num_hidden_layers", "num_attention_heads", "num_key_value_heads", "head_dim", "hidden_size"))
    assert set(g) >= {"fwd_dense", "bwd_dense_loss", "bwd_dense_grads_fp16_scaled", "grad_norms", "window", "layer_types"}
    assert g["window"] == WINDOW and list(g["layer_types"]) == ["full_attention", "sliding_attention", "sliding_attention"]
    for l in range(L):
        p = f"model.layers.{l}.self_attn."
        assert grads[p + "q_proj.weight"].shape == (Hq * D, H) and grads[p + "k_proj.bias"].shape == (Hkv * D,)
    assert len(grads) == 2 + 12 * L
    seqs = synth.make_case(QWEN2_SWA_DATA)
    assert len(g["fwd_dense"]) == len(seqs)
    for lp, s in zip(g["fwd_dense"], seqs):
        assert lp.shape == (len(s) - 1,) and lp.dtype == torch.float32
    assert max(map(len, seqs)) > 3 * WINDOW                           # sequences a few windows long
    assert os.path.getsize(FIXTURE) < 400_000


def test_qwen2_swa_fixture_config_windows():
    pytest.importorskip("transformers")
    for cls in ("Qwen2Config", "Qwen3Config"):
        c = hf_config(cls)
        assert _windows_of(_m(c)) == [0, WINDOW, WINDOW], cls
