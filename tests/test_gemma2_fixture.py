"""Gemma-2: the tiny configurations behind tests/golden/engine_gemma2.pt (scripts/make_golden_gemma.py: the REFERENCE's dense
per-sequence path over an unmodified transformers Gemma2ForCausalLM in fp32 on the CPU, eager attention), the checks of the fixture and
of the model layer's configuration rules, and the float64 soft-cap reference (tests/softcap_ref64.py) against torch autograd.

* gemma2:      4 layers (sliding, full, sliding, full - HF's default layer_types), 4 / 2 heads, head_dim 64, query_pre_attn_scalar 32,
               sliding_window 24, attn_logit_softcapping 4, final_logit_softcapping 3, GeGLU, the four `1 + w` sandwich norms, tied head.
* gemma2_d128: the same sizes with head_dim 128 and 2 / 1 heads (caps 2 and 1.5, matrices at 0.12 - see CASE_STD), so that both kernel
               widths see a capped and a windowed layer.

Every record also holds HF's logprobs with ONE feature removed - fwd_dense_off_attn_cap, fwd_dense_off_final_cap, fwd_dense_off_window
(a window wider than every sequence) and fwd_dense_off_act (silu instead of gelu_pytorch_tanh) - and the fixture must keep each
max |fwd_dense - fwd_dense_off_*| >= 0.4 (MIN_GAP of tests/test_llama_family_fixture.py): 5x the bf16 forward tolerance, so a run that
ignores a feature cannot pass.  tests/test_gpu_engine_gemma.py runs the product engine on them."""
import os

import pytest
import torch

import family
import softcap_ref64 as SR
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import _windows_of, check_supported, make_config
from family import _m, att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden_gemma.py read them here)
from test_llama_family_fixture import LLAMA, MIN_GAP

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILE = "engine_gemma2.pt"
WINDOW = 24
STD, NORM_STD = 0.15, 0.1          # matrices N(0, STD); norm weights N(0, NORM_STD) (Gemma multiplies by 1 + w)
# gemma2_d128: matrices at 0.12 and caps 2.0 / 1.5.  At STD HF's OWN bf16 run of this geometry has a median gradient ratio of 0.03 or
# more, outside the 0.0255 the GPU tests apply (0.022 at 0.12); at 0.12 the caps 4 / 3 leave feature gaps of 0.25 / 0.21, below MIN_GAP.
CASE_STD = {"gemma2_d128": 0.12}
GEMMA2 = dict(vocab_size=256, hidden_size=32, intermediate_size=64, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2,
              head_dim=64, query_pre_attn_scalar=32, sliding_window=WINDOW, rms_norm_eps=1e-6, attn_logit_softcapping=4.0,
              final_logit_softcapping=3.0, max_position_embeddings=256)
GEMMA2_D128 = dict(GEMMA2, num_attention_heads=2, num_key_value_heads=1, head_dim=128, attn_logit_softcapping=2.0, final_logit_softcapping=1.5)
DATA = {"kind": "tau2", "seed": 6, "V": 256, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 128}
# case -> (record name, geometry, data, weight seed)
CASES = {"gemma2": ("gemma2", GEMMA2, DATA, 31), "gemma2_d128": ("gemma2_d128", GEMMA2_D128, DATA, 34)}
# feature removed -> the configuration change that removes it
OFF = {"attn_cap": dict(attn_logit_softcapping=None), "final_cap": dict(final_logit_softcapping=None),
       "window": dict(sliding_window=4096), "act": dict(hidden_activation="silu")}
CONTROL = dict(attn_logit_softcapping=None, final_logit_softcapping=None, sliding_window=4096)     # both caps off, no effective window


def hf_config(case, off=None, attn="eager", **change):
    """The case's Gemma2Config; `off`: one of OFF (that feature removed) or "control" (both caps None and the window wider than
    every sequence); further fields through `change`."""
    import transformers
    kw = dict(CASES[case][1])
    kw.update(CONTROL if off == "control" else OFF[off] if off else {})
    kw.update(change)
    c = transformers.Gemma2Config(**kw)
    c._attn_implementation = attn
    return c


def weights(model, seed, std=STD):
    """Seeded fp32 weights for every parameter of `model`, by name in named_parameters order: norm weights N(0, NORM_STD), every
    matrix N(0, std)."""
    g = torch.Generator().manual_seed(seed)
    return {n: (NORM_STD if n.endswith("norm.weight") else std) * torch.randn(p.shape, generator=g) for n, p in model.named_parameters()}


def hf_model(case, off=None, attn="eager", **change):
    """The unmodified transformers Gemma2ForCausalLM of `case` with the seeded weights (fp32, train mode)."""
    import transformers
    m = transformers.Gemma2ForCausalLM(hf_config(case, off, attn, **change))
    return family.load_weights(m, weights(m, CASES[case][3], CASE_STD.get(case, STD)))


def seqs_of(case):
    return synth.make_case(CASES[case][2])


def gold(case):
    return torch.load(os.path.join(GOLD, FILE), weights_only=True)[CASES[case][0]]


# ---------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_names_shapes_and_feature_gaps(case):
    pytest.importorskip("transformers")
    g = gold(case)
    grads = gold_grads(g)
    model = hf_model(case)
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {n: tuple(v.shape) for n, v in grads.items()}
    assert "lm_head.weight" not in grads                                   # tied head
    assert "model.layers.0.pre_feedforward_layernorm.weight" in grads and "model.layers.3.post_feedforward_layernorm.weight" in grads
    seqs = seqs_of(case)
    assert len(seqs) == 12 and max(map(len, seqs)) > 3 * WINDOW
    assert len(g["fwd_dense"]) == len(seqs)
    for off in OFF:
        other = g["fwd_dense_off_" + off]
        assert len(other) == len(seqs)
        for lp, o, s in zip(g["fwd_dense"], other, seqs):
            assert lp.shape == o.shape == (len(s) - 1,) and lp.dtype == torch.float32
        gap = max(float((a - b).abs().max()) for a, b in zip(g["fwd_dense"], other))
        assert gap >= MIN_GAP, (off, gap)          # a run that ignores the feature cannot pass the bf16 forward bound (0.08)
    assert all(v > 0 for v in g["grad_norms"].values())
    assert os.path.getsize(os.path.join(GOLD, FILE)) < (1 << 20)           # two records, five forward sets each; the limit for a committed file


# ---------------------------------------------------------------------------------------------------------------- configuration rules
@pytest.mark.parametrize("case", list(CASES))
def test_check_supported_accepts_gemma2(case):
    pytest.importorskip("transformers")
    check_supported(hf_config(case))                                          # refused before Gemma-2 support: the caps and the activation
    for off in ("attn_cap", "final_cap", "window", "control"):
        check_supported(hf_config(case, off))
    check_supported(hf_config(case, attn_logit_softcapping=0.0, final_logit_softcapping=0.0))       # 0 = no cap


def test_windows_of_gemma2():
    tr = pytest.importorskip("transformers")
    c = hf_config("gemma2")
    assert isinstance(c, tr.Gemma2Config) and c.model_type == "gemma2"
    assert _windows_of(_m(c)) == [WINDOW, 0, WINDOW, 0]
    assert _windows_of(_m(hf_config("gemma2_d128"))) == [WINDOW, 0, WINDOW, 0]


@pytest.mark.parametrize("field,change", [
    ("head_dim", dict(head_dim=256)),
    ("hidden_activation", dict(hidden_activation="gelu")),
    ("hidden_activation", dict(hidden_activation="silu")),
    ("query_pre_attn_scalar", dict(query_pre_attn_scalar=None)),
    ("query_pre_attn_scalar", dict(query_pre_attn_scalar=0)),
    ("attn_logit_softcapping", dict(attn_logit_softcapping=-1.0)),
])
def test_check_supported_refuses_gemma2_and_names_the_field(field, change):
    pytest.importorskip("transformers")
    c = hf_config("gemma2")
    d = make_config(dict(GEMMA2, model_type="gemma2", hidden_activation="gelu_pytorch_tanh"))    # a plain namespace works the same way
    check_supported(c); check_supported(d)
    cfgs = [d]
    for k, v in change.items():
        if v is None:
            delattr(d, k)                                                      # missing altogether (Gemma2Config itself always carries the field)
        else:
            setattr(c, k, v); setattr(d, k, v)
            cfgs = [c, d]
    for cfg in cfgs:
        with pytest.raises(ValueError, match=field):
            check_supported(cfg)


@pytest.mark.parametrize("field,change", [
    ("attn_logit_softcapping", dict(attn_logit_softcapping=50.0)),
    ("final_logit_softcapping", dict(final_logit_softcapping=30.0)),
    ("hidden_act", dict(hidden_act="gelu")),
])
@pytest.mark.parametrize("model_type", [None, "llama", "gemma", "gemma3_text"])
def test_soft_cap_fields_stay_refused_on_other_model_types(field, change, model_type):
    kw = dict(LLAMA, rope_parameters={"rope_type": "default", "rope_theta": 1e4}, **change)
    if model_type is not None:
        kw["model_type"] = model_type
    with pytest.raises(ValueError, match=field):
        check_supported(make_config(kw))


def test_gemma2_footprint_counts_the_sandwich_norms():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    c = hf_config("gemma2")
    e = TreeTrainingEngine(c, torch.device("cpu"), torch.float32, 128)
    plain = make_config({k: v for k, v in c.to_dict().items() if k != "model_type"})
    mk = lambda cfg: type("M", (), {"config": cfg, "named_modules": lambda self: iter(())})()
    assert e._per_token_layer_bytes(mk(c)) - e._per_token_layer_bytes(mk(plain)) == 2 * 2 * c.hidden_size


# ---------------------------------------------------------------------------------------------------------------- float64 reference
@pytest.mark.parametrize("softcap", [0.0, 2.0, 0.25])
@pytest.mark.parametrize("hq,hkv", [(4, 2), (2, 1)])
def test_softcap_reference_matches_autograd(hq, hkv, softcap):
    """tests/softcap_ref64.py (closed-form backward with the capped derivative) against torch autograd of the plain formula, float64;
    a window and an ancestor-style mask; softcap 0.25 saturates tanh (|z| / c up to ~16)."""
    g = torch.Generator().manual_seed(hq + int(8 * softcap))
    Tq, Tk, D = 37, 50, 16
    q, do = (torch.randn(Tq, hq, D, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(Tk, hkv, D, generator=g, dtype=torch.float64) for _ in range(2))
    qi, kj = (Tk - Tq) + torch.arange(Tq)[:, None], torch.arange(Tk)[None, :]
    vis = (kj <= qi) & (qi - kj < 20) & ((kj % 7 != 3) | (kj == qi))
    scale = 0.4
    qa, ka, va = (x.clone().requires_grad_(True) for x in (q, k, v))
    out, lse = SR.plain_capped_attention(qa, ka, va, vis, scale, softcap)
    dq, dk, dv = torch.autograd.grad(out, (qa, ka, va), do)
    ref = SR.reference_cap(q, k, v, vis, do, out.detach(), scale, softcap)
    for name, want in (("out", out.detach()), ("lse", lse.detach()), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.allclose(ref[name], want, rtol=1e-11, atol=1e-12), (name, float((ref[name] - want).abs().max()))
    assert all(bool(torch.isfinite(ref[x]).all()) for x in ref)
    if softcap == 0.0:                                  # no cap: the terms of reference_vis, exactly
        import test_gpu_attention_window as W
        base = W.reference_vis(q, k, v, vis, do, out.detach(), scale)
        assert set(base) == set(ref)
        for x in base:
            assert torch.equal(base[x], ref[x]), x
    else:                                               # the cap's own F part makes the bound terms larger, never smaller
        base = SR.reference_cap(q, k, v, vis, do, out.detach(), scale, 0.0)
        ch = SR.cap_changes(ref, SR.reference_cap(q, k, v, vis, do, None, scale, 0.0), torch.bfloat16)
        assert set(ch) == {"out", "lse", "dq", "dk", "dv"} and all(v > 0 for v in ch.values())
        assert bool((ref["out_F"] > 0).all()) and base["out_F"].shape == ref["out_F"].shape


# ---------------------------------------------------------------------------------------------------------------- the engine on the CPU
@pytest.mark.parametrize("case", list(CASES))
def test_gemma2_engine_on_cpu_matches_the_reference_fixture(case, monkeypatch):
    """The product engine with its device steps replaced by CPU stand-ins (fp32) reproduces the reference's dense logprobs, loss and
    every gradient: the layer wiring (sandwich norms with offset 1, GeGLU, the scaled embedding, query_pre_attn_scalar, per-layer
    windows, both caps) is host-side plumbing around the kernels."""
    pytest.importorskip("transformers")
    g = gold(case)
    named = family.check_cpu_engine_matches_fixture(hf_model(case), synth.as_tensors(seqs_of(case)), g, monkeypatch)
    assert set(named) == set(gold_grads(g))
