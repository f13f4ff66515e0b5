"""Llama-3 / Mistral / Mixtral: the tiny configurations behind tests/golden/engine_llama3.pt, engine_mistral.pt and engine_mixtral.pt
(scripts/make_golden_llama.py: the REFERENCE's dense per-sequence path over unmodified HF models in fp32 on the CPU, eager attention)
and the checks of the fixtures and of the model layer's configuration rules.

* llama3 / llama3_bias / yarn: LlamaForCausalLM, head_dim 64, 4 / 2 heads, untied lm_head; rope_type llama3 (factor 8, low 1, high 4,
  original 32: sequences of up to 128 tokens reach all three frequency bands), the same with attention_bias and mlp_bias, and
  rope_type yarn (factor 4, max_position_embeddings = 4 x 32).
* mistral: MistralForCausalLM, sliding_window 24 on all 3 layers, sequences longer than 3 windows.
* mixtral: MixtralForCausalLM, 4 experts, top 2, head_dim 64, sliding_window 24.

The matrices are drawn at STD (not the usual 0.02, where a run that ignores the feature would still pass the bf16 bounds): every
record also holds `fwd_dense_off`, HF's logprobs with the feature off (default RoPE, sliding_window None, biases zeroed), and the
fixture must keep max |fwd_dense - fwd_dense_off| >= 0.4, 5x the bf16 forward tolerance.  tests/test_gpu_engine_llama.py runs the
product engine on them."""
import os

import pytest
import torch

import family
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import _windows_of, check_supported, make_config
from dynamictreeattn_amd.tree_training_engine import _mlp_elems_per_token
from family import _m, att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden_llama.py read them here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
WINDOW = 24
STD = 0.2                  # the matrices' scale in the Llama cases (hidden 16: the per-element logit scale of std 0.1 at hidden 64)
CASE_STD = {"mistral": 0.12, "mixtral": 0.08}     # hidden 32; lowered until HF's own bf16 run sits inside the bf16 bounds
ROUTER_STD = 1.0          # wide router rows: top-2 margins that a bf16 run does not flip
MIN_GAP = 0.4
LLAMA = dict(vocab_size=256, hidden_size=16, intermediate_size=32, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2,
             head_dim=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
LLAMA3_ROPE = {"rope_type": "llama3", "rope_theta": 10000.0, "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
               "original_max_position_embeddings": 32}
YARN_ROPE = {"rope_type": "yarn", "rope_theta": 10000.0, "factor": 4.0, "original_max_position_embeddings": 32}
MISTRAL = dict(vocab_size=512, hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2,
               head_dim=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
MIXTRAL = dict(vocab_size=512, hidden_size=32, intermediate_size=48, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
               head_dim=64, rms_norm_eps=1e-5, tie_word_embeddings=False, num_local_experts=4, num_experts_per_tok=2)
LLAMA_DATA = {"kind": "tau2", "seed": 8, "V": 256, "G": 3, "sys_len": 30, "turns": 4, "lo": 14, "hi": 30, "cap": 128}
WINDOW_DATA = {"kind": "tau2", "seed": 6, "V": 512, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 128}
# case -> (fixture file, record name, HF class stem, geometry, data, weight seed)
CASES = {"llama3": ("engine_llama3.pt", "llama3", "Llama", LLAMA, LLAMA_DATA, 21),
         "llama3_bias": ("engine_llama3.pt", "llama3_bias", "Llama", LLAMA, LLAMA_DATA, 22),
         "yarn": ("engine_llama3.pt", "yarn", "Llama", LLAMA, LLAMA_DATA, 23),
         "mistral": ("engine_mistral.pt", None, "Mistral", MISTRAL, WINDOW_DATA, 24),
         "mixtral": ("engine_mixtral.pt", None, "Mixtral", MIXTRAL, WINDOW_DATA, 25)}


def hf_config(case, off=False, attn="eager"):
    """The case's HF configuration; `off`: the same model with the feature switched off (default RoPE / no window; the biases of
    llama3_bias stay parameters and are zeroed by hf_model)."""
    import transformers
    _, _, stem, geo, _, _ = CASES[case]
    kw = dict(geo, max_position_embeddings=256, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    if stem == "Llama":
        rope = YARN_ROPE if case == "yarn" else LLAMA3_ROPE
        if not off:
            kw["rope_parameters"] = dict(rope)
            kw["max_position_embeddings"] = 128 if case == "yarn" else 256
        if case == "llama3_bias":
            kw.update(attention_bias=True, mlp_bias=True, rope_parameters=dict(rope))     # the feature of this record is the biases
    else:
        kw["sliding_window"] = None if off else WINDOW
    c = getattr(transformers, stem + "Config")(**kw)
    c._attn_implementation = attn
    if stem == "Mixtral":
        c._experts_implementation = "eager"
    return c


def weights(model, seed, std=STD):
    """Seeded fp32 weights for every parameter of `model`, by name in named_parameters order: norms 1 + N(0, 0.1), biases N(0, 0.1),
    router rows N(0, ROUTER_STD), every other matrix N(0, std)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        if n.endswith("norm.weight"):
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
        elif n.endswith(".bias"):
            v = 0.1 * torch.randn(p.shape, generator=g)
        elif n.endswith("mlp.gate.weight"):
            v = ROUTER_STD * torch.randn(p.shape, generator=g)
        else:
            v = std * torch.randn(p.shape, generator=g)
        out[n] = v
    return out


def hf_model(case, off=False, attn="eager"):
    """The unmodified transformers model of `case` with the seeded weights (fp32, train mode)."""
    import transformers
    stem, seed = CASES[case][2], CASES[case][5]
    m = getattr(transformers, stem + "ForCausalLM")(hf_config(case, off, attn))
    w = weights(m, seed, CASE_STD.get(case, STD))
    return family.load_weights(m, {n: torch.zeros_like(v) if off and n.endswith(".bias") else v for n, v in w.items()})


def seqs_of(case):
    return synth.make_case(CASES[case][4])


def gold(case):
    file, rec = CASES[case][:2]
    g = torch.load(os.path.join(GOLD, file), weights_only=True)
    return g[rec] if rec is not None else g


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_names_shapes_and_feature_gap(case):
    pytest.importorskip("transformers")
    g = gold(case)
    grads = gold_grads(g)
    model = hf_model(case)
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {n: tuple(v.shape) for n, v in grads.items()}
    assert "lm_head.weight" in grads
    assert ("model.layers.0.self_attn.o_proj.bias" in grads) == (case == "llama3_bias")
    assert ("model.layers.0.mlp.down_proj.bias" in grads) == (case == "llama3_bias")
    assert ("model.layers.0.mlp.experts.gate_up_proj" in grads) == (case == "mixtral")
    seqs = seqs_of(case)
    assert len(g["fwd_dense"]) == len(g["fwd_dense_off"]) == len(seqs)
    for lp, off, s in zip(g["fwd_dense"], g["fwd_dense_off"], seqs):
        assert lp.shape == off.shape == (len(s) - 1,) and lp.dtype == torch.float32
    longest = max(map(len, seqs))
    assert (longest > 3 * WINDOW) if case in ("mistral", "mixtral") else (100 <= longest <= 128)
    gap = max(float((a - b).abs().max()) for a, b in zip(g["fwd_dense"], g["fwd_dense_off"]))
    assert gap >= MIN_GAP, gap                 # a run that ignores the feature cannot pass the bf16 forward bound (0.08)
    assert all(v > 0 for v in g["grad_norms"].values())


def test_fixture_files_are_small():
    for file in {c[0] for c in CASES.values()}:
        assert os.path.getsize(os.path.join(GOLD, file)) < 400_000, file
    assert set(torch.load(os.path.join(GOLD, "engine_llama3.pt"), weights_only=True)) == {"llama3", "llama3_bias", "yarn"}


# ---------------------------------------------------------------------------------------------------------------- configuration rules
def test_windows_of_mistral_and_mixtral_configs():
    tr = pytest.importorskip("transformers")
    for case, cls in (("mistral", tr.MistralConfig), ("mixtral", tr.MixtralConfig)):
        c = hf_config(case)
        assert isinstance(c, cls) and _windows_of(_m(c)) == [WINDOW] * c.num_hidden_layers
        assert _windows_of(_m(hf_config(case, off=True))) == [0] * c.num_hidden_layers
    assert _windows_of(_m(hf_config("llama3"))) == [0, 0, 0]
    import test_qwen2_swa_fixture as swa                           # the Qwen2 / Qwen3 rules are unchanged
    for cls in ("Qwen2Config", "Qwen3Config"):
        assert _windows_of(_m(swa.hf_config(cls))) == [0, swa.WINDOW, swa.WINDOW]


def test_check_supported_accepts_the_supported_configs():
    pytest.importorskip("transformers")
    import test_qwen2_d64_fixture as d64
    import test_qwen2_swa_fixture as swa
    import test_qwen3_moe_fixture as moe
    for case in CASES:
        check_supported(hf_config(case))
        check_supported(hf_config(case, off=True))
    for c in (swa.hf_config("Qwen2Config"), swa.hf_config("Qwen3Config"), moe.hf_config(), d64.hf_qwen2_d64().config,
              make_config(moe.QWEN3_MOE), make_config(dict(LLAMA, rope_parameters=dict(LLAMA3_ROPE)))):
        check_supported(c)


@pytest.mark.parametrize("field,change", [
    ("rope_type", dict(rope_parameters={"rope_type": "dynamic", "rope_theta": 1e4, "factor": 2.0})),
    ("rope_type", dict(rope_parameters={"rope_type": "longrope", "rope_theta": 1e4, "short_factor": [1.0] * 32, "long_factor": [2.0] * 32})),
    ("rope_type", dict(rope_parameters={"rope_type": "proportional", "rope_theta": 1e4})),
    ("rope_type", dict(rope_parameters={"rope_type": "ntk-by-parts", "rope_theta": 1e4})),
    ("nested", dict(rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": 1e4},
                                     "sliding_attention": {"rope_type": "default", "rope_theta": 1e6}})),
    ("partial_rotary_factor", dict(partial_rotary_factor=0.5)),
    ("partial_rotary_factor", dict(rope_parameters={"rope_type": "default", "rope_theta": 1e4, "partial_rotary_factor": 0.25})),
    ("hidden_act", dict(hidden_act="gelu")),
    ("attention_dropout", dict(attention_dropout=0.1)),
    ("router_jitter_noise", dict(router_jitter_noise=0.01)),
    ("attn_logit_softcapping", dict(attn_logit_softcapping=50.0)),
    ("final_logit_softcapping", dict(final_logit_softcapping=30.0)),
    ("attention_sinks", dict(attention_sinks=True)),
])
def test_check_supported_refuses_and_names_the_field(field, change):
    c = make_config(dict(LLAMA, rope_parameters={"rope_type": "default", "rope_theta": 1e4}, **{k: v for k, v in change.items() if k != "rope_parameters"}))
    if "rope_parameters" in change:
        c.rope_parameters = change["rope_parameters"]
    with pytest.raises(ValueError, match=field):
        check_supported(c)


def test_attention_dropout_is_refused_in_training_mode_only():
    c = make_config(dict(LLAMA, attention_dropout=0.1))
    check_supported(c, training=False)
    with pytest.raises(ValueError, match="attention_dropout"):
        check_supported(c, training=True)


def test_mixtral_footprint_uses_the_mapped_fields():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.model import Qwen3TreeLM, is_moe_layer
    from dynamictreeattn_amd.tree_training_engine import _has_moe
    c = hf_config("mixtral")
    E, k, H, I = c.num_local_experts, c.num_experts_per_tok, c.hidden_size, c.intermediate_size
    assert all(is_moe_layer(c, l) for l in range(c.num_hidden_layers)) and _has_moe(c)
    assert _mlp_elems_per_token(c, 0) == k * (3 * I + H) + 2 * E
    assert not _has_moe(hf_config("llama3")) and _mlp_elems_per_token(hf_config("llama3"), 0) == 4 * LLAMA["intermediate_size"]
    mine = Qwen3TreeLM(dict(MIXTRAL, rope_theta=1e4))                     # the container follows the same mapping
    assert tuple(mine.model.layers[0].mlp.experts.gate_up_proj.shape) == (E, 2 * I, H)
    assert mine.model.layers[0].mlp.gate.norm_topk_prob is True


# ---------------------------------------------------------------------------------------------------------------- the engine on the CPU
@pytest.mark.parametrize("case", ["llama3", "llama3_bias", "yarn"])
def test_llama_engine_on_cpu_matches_the_reference_fixture(case, monkeypatch):
    """The product engine with its device steps replaced by the CPU stand-ins of tests/hostmirror.py (fp32) reproduces the reference's
    dense logprobs, loss and every gradient: the scaled RoPE table, the o_proj / MLP biases and the untied head are host-side plumbing."""
    pytest.importorskip("transformers")
    g = gold(case)
    named = family.check_cpu_engine_matches_fixture(hf_model(case), synth.as_tensors(seqs_of(case)), g, monkeypatch)
    assert set(named) == set(gold_grads(g))
