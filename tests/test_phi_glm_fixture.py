"""Phi-3 / Phi-4 and GLM-4: the tiny configurations behind tests/golden/engine_phi3.pt and engine_glm4.pt
(scripts/make_golden_phi_glm.py: the REFERENCE's dense per-sequence path over unmodified transformers Phi3ForCausalLM /
Glm4ForCausalLM models in fp32 on the CPU, eager attention), the checks of the fixtures, of longrope's frequencies, of the model
layer's configuration rules, and the engine on the CPU against the fixtures in packed mode and in the block-wise walk.

Every model has 2 layers, vocabulary 256 and head_dim passed explicitly, so that the hidden size (and with it the fixture) stays small:

* phi3_a:  Phi3ForCausalLM, 4 / 2 heads of 128, rotary dimension 96 (partial_rotary_factor 0.75), rope_type longrope with
           original_max_position_embeddings 16, max_position_embeddings 64 and short_factor != long_factor, tied head.  Every
           sequence is longer than 16: HF rotates by the long factors, scaled by sqrt(1 + ln 4 / ln 16).
* phi3_b:  3 / 1 heads of 64, rotary dimension 48, plain RoPE, sliding_window 8 on every layer.
* phi3_c:  2 / 1 heads of 128, the whole head rotated: the fused qkv_proj / gate_up_proj modules alone (Phi-4 14B, Phi-3-medium).
* glm4_a:  Glm4ForCausalLM, 4 / 2 heads of 128, rotary dimension 64, interleaved pairs, q/k/v biases, four norms per layer.
* glm4_b:  6 / 2 heads of 64, rotary dimension 32.

Phi3Config checks the length of short_factor / long_factor against hidden_size // num_attention_heads, which is not the head_dim of a
configuration that passes head_dim explicitly; hf_config builds phi3_a with plain RoPE and puts the longrope fields into
config.rope_parameters afterwards (the model reads them from there when it is built).

Every record also holds HF's logprobs with ONE feature removed (OFF) and the fixture must keep each max |fwd_dense - fwd_dense_off_*|
>= 0.4 (MIN_GAP of tests/test_llama_family_fixture.py): a run that ignores the feature cannot pass the bf16 forward bound.
tests/test_gpu_engine_phi_glm.py runs the product engine on these cases."""
import contextlib
import copy
import os

import pytest
import torch

import family
import partial_rope_host
from dynamictreeattn_amd import model as M
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd.model import _windows_of, check_supported, ensure_supported, is_glm4, is_phi3, make_config, rope_of, rotary_dim
from family import _m, att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden_phi_glm.py read them here)
from test_llama_family_fixture import LLAMA, MIN_GAP

GOLD = os.path.join(os.path.dirname(__file__), "golden")
STD, NORM_STD = 0.1, 0.1           # matrices and biases N(0, STD); norm weights 1 + N(0, NORM_STD)
WINDOW = 8
ORIG_MAX = 16
BASE = dict(vocab_size=256, intermediate_size=64, num_hidden_layers=2, rms_norm_eps=1e-5, max_position_embeddings=256, pad_token_id=None,
            eos_token_id=None, bos_token_id=None)
DEFAULT_ROPE = {"rope_type": "default", "rope_theta": 10000.0}
SHORT = [1.0 + 0.02 * i for i in range(48)]
LONG = [1.5 + 0.1 * i for i in range(48)]
LONGROPE = {"rope_type": "longrope", "rope_theta": 10000.0, "partial_rotary_factor": 0.75, "short_factor": SHORT, "long_factor": LONG,
            "original_max_position_embeddings": ORIG_MAX}
PHI3_A = dict(BASE, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=True,
              max_position_embeddings=64, rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.75))
PHI3_B = dict(BASE, hidden_size=48, num_attention_heads=3, num_key_value_heads=1, head_dim=64, tie_word_embeddings=False,
              sliding_window=WINDOW, rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.75))
PHI3_C = dict(BASE, hidden_size=32, num_attention_heads=2, num_key_value_heads=1, head_dim=128, tie_word_embeddings=False,
              rope_parameters=dict(DEFAULT_ROPE))
GLM4_A = dict(BASE, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=False,
              attention_bias=True, rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.5))
GLM4_B = dict(GLM4_A, hidden_size=48, num_attention_heads=6, num_key_value_heads=2, head_dim=64)
DATA = {"kind": "tau2", "seed": 6, "V": 256, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 128}
DATA_A = dict(DATA, sys_len=18, turns=3, lo=6, hi=12, cap=64)              # every sequence longer than ORIG_MAX, none longer than 64
# case -> (fixture file, HF class stem, geometry, data, weight seed)
CASES = {"phi3_a": ("engine_phi3.pt", "Phi3", PHI3_A, DATA_A, 31), "phi3_b": ("engine_phi3.pt", "Phi3", PHI3_B, DATA, 32),
         "phi3_c": ("engine_phi3.pt", "Phi3", PHI3_C, DATA, 33),
         "glm4_a": ("engine_glm4.pt", "Glm4", GLM4_A, DATA, 41), "glm4_b": ("engine_glm4.pt", "Glm4", GLM4_B, DATA, 42)}
ROTARY = {"phi3_a": 96, "phi3_b": 48, "phi3_c": 128, "glm4_a": 64, "glm4_b": 32}
# feature removed -> the configuration change that removes it ("longrope": the factors are left out by hf_config; "interleaved" is
# not a configuration: hf_run_with swaps HF's rotation for the half-split one while the model runs)
OFF = {"longrope": {}, "window": dict(sliding_window=None), "interleaved": {},
       "partial": lambda kw: dict(rope_parameters=dict(kw["rope_parameters"], partial_rotary_factor=1.0))}


def offs_of(case):
    return {"phi3_a": ["longrope"], "phi3_b": ["window", "partial"], "phi3_c": []}.get(case, ["partial", "interleaved"])


def hf_config(case, off=None, attn="eager", **change):
    """The case's Phi3Config / Glm4Config; `off`: one of OFF (that feature removed); further fields through `change`."""
    import transformers
    kw = copy.deepcopy(CASES[case][2])
    if off:
        kw.update(OFF[off](kw) if callable(OFF[off]) else copy.deepcopy(OFF[off]))
    kw.update(change)
    c = getattr(transformers, CASES[case][1] + "Config")(**kw)
    if case == "phi3_a" and off != "longrope" and "rope_parameters" not in change:
        c.rope_parameters.update(copy.deepcopy(LONGROPE))                  # (see the module docstring)
        c.original_max_position_embeddings = ORIG_MAX
    c._attn_implementation = attn
    return c


def weights(model, seed, std=STD):
    """Seeded fp32 weights for every parameter of `model`, by name in named_parameters order: norm weights 1 + N(0, NORM_STD), every
    matrix and bias N(0, std)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        if n.endswith(("norm.weight", "layernorm.weight")):
            out[n] = 1.0 + NORM_STD * torch.randn(p.shape, generator=g)
        else:
            out[n] = std * torch.randn(p.shape, generator=g)
    return out


def hf_model(case, off=None, attn="eager", **change):
    """The unmodified transformers model of `case` with the seeded weights (fp32, train mode)."""
    import transformers
    m = getattr(transformers, CASES[case][1] + "ForCausalLM")(hf_config(case, off, attn, **change))
    return family.load_weights(m, weights(m, CASES[case][4]))


@contextlib.contextmanager
def hf_run_with(off):
    """off == "interleaved": while the block runs, transformers' GLM-4 rotates in half-split pairs (Phi-3's apply_rotary_pos_emb)."""
    if off != "interleaved":
        yield
        return
    from transformers.models.glm4 import modeling_glm4
    from transformers.models.phi3 import modeling_phi3
    real = modeling_glm4.apply_rotary_pos_emb

    def half_split(q, k, cos, sin, unsqueeze_dim=1):
        n = cos.shape[-1] // 2                                             # GLM-4 keeps the table's first half; Phi-3's takes it whole
        return modeling_phi3.apply_rotary_pos_emb(q, k, torch.cat([cos[..., :n], cos[..., :n]], -1), torch.cat([sin[..., :n], sin[..., :n]], -1),
                                                  unsqueeze_dim)
    modeling_glm4.apply_rotary_pos_emb = half_split
    try:
        yield
    finally:
        modeling_glm4.apply_rotary_pos_emb = real


def llama_control(case):
    """Llama-shaped wiring of the same sizes (separate projections, the whole head rotated, default RoPE, no window, no bias) with
    weights from the same helper: the control of the fp32 GPU test - what the engine's gradients deviate by on a model of this size
    without any of these families' features."""
    import transformers
    geo = {k: v for k, v in CASES[case][2].items() if k not in ("sliding_window", "rope_parameters", "attention_bias")}
    c = transformers.LlamaConfig(**geo, rope_parameters=dict(DEFAULT_ROPE))
    c._attn_implementation = "eager"
    m = transformers.LlamaForCausalLM(c)
    return family.load_weights(m, weights(m, CASES[case][4]))


def seqs_of(case):
    return synth.make_case(CASES[case][3])


def gold(case):
    return torch.load(os.path.join(GOLD, CASES[case][0]), weights_only=True)[case]


# ---------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_names_shapes_and_feature_gaps(case):
    pytest.importorskip("transformers")
    g = gold(case)
    grads = gold_grads(g)
    model = hf_model(case)
    c = model.config
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {n: tuple(v.shape) for n, v in grads.items()}
    assert ("lm_head.weight" in grads) == (case != "phi3_a")                  # phi3_a: tied head
    H3 = (c.num_attention_heads + 2 * c.num_key_value_heads) * c.head_dim
    if case.startswith("phi3"):
        assert grads["model.layers.0.self_attn.qkv_proj.weight"].shape == (H3, c.hidden_size)
        assert grads["model.layers.1.mlp.gate_up_proj.weight"].shape == (2 * c.intermediate_size, c.hidden_size)
    else:
        assert grads["model.layers.0.self_attn.q_proj.bias"].shape == (c.num_attention_heads * c.head_dim,)
        assert "model.layers.1.post_self_attn_layernorm.weight" in grads and "model.layers.1.post_mlp_layernorm.weight" in grads
        assert grads["model.layers.1.mlp.gate_up_proj.weight"].shape == (2 * c.intermediate_size, c.hidden_size)
    assert c.num_hidden_layers == 2 and c.vocab_size % 8 == 0 and rotary_dim(c) == ROTARY[case]
    seqs = seqs_of(case)
    lens = list(map(len, seqs))
    assert len(seqs) >= 9 and len(g["fwd_dense"]) == len(seqs)
    if case == "phi3_a":
        assert min(lens) > ORIG_MAX and max(lens) <= 64                      # HF takes the long factors for every sequence
    else:
        assert max(lens) > 3 * WINDOW
    assert {k for k in g if k.startswith("fwd_dense_off_")} == {"fwd_dense_off_" + o for o in offs_of(case)}
    for off in offs_of(case):
        gap = max(float((a - b).abs().max()) for a, b in zip(g["fwd_dense"], g["fwd_dense_off_" + off]))
        assert gap >= MIN_GAP, (off, gap)
    assert all(v > 0 for v in g["grad_norms"].values())
    assert os.path.getsize(os.path.join(GOLD, CASES[case][0])) < (1 << 20)


@pytest.mark.parametrize("case", list(CASES))
def test_hf_eager_in_fp32_reproduces_the_fixture(case):
    """HF's own eager forward / backward per sequence (family.hf_dense) gives the fixture's logprobs, loss and gradients."""
    pytest.importorskip("transformers")
    g = gold(case)
    hf = hf_model(case)
    seqs = synth.as_tensors(seqs_of(case))
    lps, loss = family.hf_dense(hf, seqs, att(len(seqs)), device="cpu")
    assert max(float((a - b).abs().max()) for a, b in zip(lps, g["fwd_dense"])) < 1e-4
    assert abs(loss - g["bwd_dense_loss"]) < 1e-4 * abs(loss)
    from oracle import model_oracle as mo
    for n, gg in gold_grads(g).items():
        assert mo.grad_ratio(gg, dict(hf.named_parameters())[n].grad) <= 1e-3, n


# ---------------------------------------------------------------------------------------------------------------- the engine on the CPU
@pytest.mark.parametrize("mode", ["packed", "stack"])
@pytest.mark.parametrize("case", list(CASES))
def test_engine_on_cpu_matches_the_reference_fixture(case, mode, monkeypatch):
    """The product engine with its device steps replaced by CPU stand-ins (fp32) reproduces the reference's dense logprobs, loss and
    every gradient, in one packed pass and in the block-wise walk: the layer wiring (fused modules, the rotary dimension's table,
    the long factors chosen from the trie, GLM-4's four norms, the window on every Phi-3 layer) is host-side plumbing."""
    pytest.importorskip("transformers")
    g = gold(case)
    partial_rope_host.install(monkeypatch)
    named = family.check_cpu_engine_matches_fixture(hf_model(case), synth.as_tensors(seqs_of(case)), g, monkeypatch, mode=mode)
    assert set(named) == set(gold_grads(g))


def _cpu_forward(hf, seqs, monkeypatch, **attrs):
    import hostmirror
    from dynamictreeattn_amd.token_trie import TokenTrie
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    if hostmirror._cpu_stack_attention is not partial_rope_host._cpu_stack_attention:
        partial_rope_host.install(monkeypatch)
    hostmirror.install(monkeypatch)
    cpu = torch.device("cpu")
    t = TokenTrie(seqs, device=cpu); t.forward_permute()
    e = TreeTrainingEngine(hf.config, cpu, torch.float32, max(map(len, seqs)), forward_only=True)
    for k, v in attrs.items():
        setattr(e, k, v)
    return e.forward(hf, t)


def test_a_feature_left_out_misses_the_fixture(monkeypatch):
    """The rotary dimension is not inert: glm4_a with the whole head rotated is off the fixture by the recorded gap and equals the
    fwd_dense_off_partial record."""
    pytest.importorskip("transformers")
    g = gold("glm4_a")
    hf = hf_model("glm4_a", "partial")
    out = _cpu_forward(hf, synth.as_tensors(seqs_of("glm4_a")), monkeypatch)
    assert max(float((a - b).abs().max()) for a, b in zip(out, g["fwd_dense"])) >= MIN_GAP
    assert max(float((a - b).abs().max()) for a, b in zip(out, g["fwd_dense_off_partial"])) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- longrope
def test_longrope_frequencies_are_transformers_bit_for_bit():
    pytest.importorskip("transformers")
    from transformers.modeling_rope_utils import _compute_longrope_parameters
    c = hf_config("phi3_a")
    rp = M._rope_dict(c)
    for long, seq_len in ((False, None), (False, ORIG_MAX), (True, ORIG_MAX + 1), (True, 64)):
        inv_hf, att_hf = _compute_longrope_parameters(c, "cpu", seq_len=seq_len)
        inv, factor = ops.longrope_inv_freq(96, rp, c.max_position_embeddings, long)
        assert inv.dtype == torch.float32 and inv.shape == (48,) and torch.equal(inv, inv_hf)
        assert float(factor) == float(att_hf) == (1 + torch.log(torch.tensor(4.0, dtype=torch.float64)) / torch.log(torch.tensor(16.0, dtype=torch.float64))).sqrt().item()
        assert torch.equal(rope_of(c, long=long)[0], inv_hf) and rope_of(c, long=long) is rope_of(c, long=long)    # cached per (config, set)
    assert not torch.equal(rope_of(c)[0], rope_of(c, long=True)[0])
    rot = hf_model("phi3_a").model.rotary_emb
    assert torch.equal(rope_of(c)[0], rot.original_inv_freq) and float(rope_of(c)[1]) == float(rot.attention_scaling)
    # an explicit attention_factor and an explicit factor go before the derived ones, as in transformers
    assert ops.longrope_inv_freq(96, dict(rp, attention_factor=1.5), 64, False)[1] == 1.5
    assert ops.longrope_inv_freq(96, dict(rp, factor=1.0), 64, False)[1] == 1.0
    for bad, field in ((dict(rp, short_factor=SHORT[:40]), "short_factor"), ({k: v for k, v in rp.items() if k != "long_factor"}, "long_factor"),
                       ({k: v for k, v in rp.items() if k != "original_max_position_embeddings"}, "original_max_position_embeddings")):
        with pytest.raises(ValueError, match=field):
            ops.longrope_inv_freq(96, bad, 64, field == "long_factor")
    # rope_inv_freq keeps its refusal, and ROPE_TYPES its members
    assert "longrope" not in ops.ROPE_TYPES
    with pytest.raises(ValueError, match="longrope"):
        ops.rope_inv_freq(96, rp, 64)


def test_partial_tables_are_the_hf_rotary_buffers():
    pytest.importorskip("transformers")
    for case in ("phi3_b", "phi3_c", "glm4_a", "glm4_b"):
        m = hf_model(case)
        inv, factor = rope_of(m.config)
        assert inv.shape == (ROTARY[case] // 2,) and torch.equal(inv, m.model.rotary_emb.inv_freq) and float(factor) == 1.0
        assert ops.rope_cos_sin(torch.arange(5), ROTARY[case], rope_of(m.config)).shape == (5, ROTARY[case])


def test_longrope_set_of_a_trie(monkeypatch):
    """TreeTrainingEngine.longrope_factors: "auto" takes the set from the trie's sequence lengths and refuses a trie with sequences on
    both sides of original_max_position_embeddings, naming it and the attribute; "short" / "long" force one set."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.token_trie import TokenTrie
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    import hostmirror
    partial_rope_host.install(monkeypatch)
    hostmirror.install(monkeypatch)
    hf = hf_model("phi3_a")
    cpu = torch.device("cpu")
    e = TreeTrainingEngine(hf.config, cpu, torch.float32, 64)
    assert e.longrope_factors == "auto"
    g = torch.Generator().manual_seed(3)
    mk = lambda n, head: torch.cat([head, torch.randint(0, 256, (n - len(head),), generator=g)])
    head = torch.randint(0, 256, (6,), generator=g)
    short, long = [mk(n, head) for n in (9, 16, 12)], [mk(n, head) for n in (17, 40)]
    trie = lambda seqs: TokenTrie(seqs, device=cpu)
    assert e._longrope_long(hf, trie(short)) is False and e._longrope_long(hf, trie(long)) is True
    with pytest.raises(ValueError, match="original_max_position_embeddings.*longrope_factors"):
        e._longrope_long(hf, trie(short + long))
    e.longrope_factors = "long"
    assert e._longrope_long(hf, trie(short + long)) is True and e._longrope_long(hf, trie(short)) is True
    e.longrope_factors = "short"
    assert e._longrope_long(hf, trie(long)) is False
    e.longrope_factors = "both"
    with pytest.raises(ValueError, match="longrope_factors"):
        e._longrope_long(hf, trie(long))
    other = TreeTrainingEngine(hf_config("phi3_b"), cpu, torch.float32, 64)
    other.longrope_factors = "long"
    assert other._longrope_long(_m(hf_config("phi3_b")), trie(short + long)) is False       # not a longrope model: nothing to choose
    # the engine's forward: short sequences match HF (short factors), the mixed trie runs under "long" on the long table
    out = _cpu_forward(hf, short, monkeypatch)
    lps, _ = family.hf_dense(hf, short, att(len(short)), device="cpu")
    assert max(float((a - b).abs().max()) for a, b in zip(out, lps)) < 1e-4
    with pytest.raises(ValueError, match="longrope_factors"):
        _cpu_forward(hf, short + long, monkeypatch)
    out = _cpu_forward(hf, short + long, monkeypatch, longrope_factors="long")
    forced = hf_model("phi3_a")
    forced.model.rotary_emb.original_inv_freq = rope_of(hf.config, long=True)[0].clone()    # HF with the long table for every length
    lps, _ = family.hf_dense(forced, short + long, att(5), device="cpu")
    assert max(float((a - b).abs().max()) for a, b in zip(out, lps)) < 1e-4
    lps_auto, _ = family.hf_dense(hf_model("phi3_a"), short, att(3), device="cpu")
    assert max(float((a - b).abs().max()) for a, b in zip(out[:3], lps_auto)) > 1e-3        # and that is not what the short table gives


# ---------------------------------------------------------------------------------------------------------------- configuration rules
@pytest.mark.parametrize("case", list(CASES))
def test_check_supported_accepts_the_cases(case):
    pytest.importorskip("transformers")
    c = hf_config(case)
    assert (is_phi3(c), is_glm4(c)) == (case.startswith("phi3"), case.startswith("glm4")) and c.model_type == case[:4]
    check_supported(c)
    for off in offs_of(case):
        check_supported(hf_config(case, off))
    ensure_supported(hf_model(case))
    assert M.is_longrope(c) == (case == "phi3_a")


def test_predicates_are_keyed_on_the_model_type_alone():
    assert not is_phi3(make_config(dict(LLAMA))) and not is_glm4(make_config(dict(LLAMA)))
    assert is_phi3(make_config(dict(LLAMA, model_type="phi3"))) and not is_phi3(make_config(dict(LLAMA, model_type="phi")))
    assert is_glm4(make_config(dict(LLAMA, model_type="glm4"))) and not is_glm4(make_config(dict(LLAMA, model_type="glm")))
    d = make_config(dict(LLAMA, head_dim=128, partial_rotary_factor=0.5, rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.75)))
    assert rotary_dim(d) == 96                                                # rope_parameters first, then the configuration
    assert rotary_dim(make_config(dict(LLAMA, head_dim=128, partial_rotary_factor=0.5))) == 64
    assert rotary_dim(make_config(dict(LLAMA, head_dim=128))) == 128


def test_windows_of_phi3_slide_on_every_layer():
    pytest.importorskip("transformers")
    assert _windows_of(_m(hf_config("phi3_b"))) == [WINDOW, WINDOW]
    assert _windows_of(_m(hf_config("phi3_b", "window"))) == [0, 0]
    assert _windows_of(_m(hf_config("phi3_a"))) == [0, 0] and _windows_of(_m(hf_config("glm4_a"))) == [0, 0]
    assert _windows_of(_m(make_config(dict(PHI3_B, model_type="phi3")))) == [WINDOW, WINDOW]


PHI3_REFUSALS = [
    ("head_dim", dict(head_dim=96)),                                           # Phi-3-mini
    ("head_dim", dict(head_dim=256)),
    ("partial_rotary_factor", dict(rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.6875))),      # 88 of 128: no multiple of 16
    ("partial_rotary_factor", dict(rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.0))),
    ("resid_pdrop", dict(resid_pdrop=0.1)),
    ("embd_pdrop", dict(embd_pdrop=0.05)),
    ("hidden_act", dict(hidden_act="gelu")),
    ("attention_dropout", dict(attention_dropout=0.1)),
    ("rope_type", dict(rope_parameters=dict(DEFAULT_ROPE, rope_type="dynamic", factor=2.0))),
    ("short_factor", dict(rope_parameters=dict(LONGROPE, short_factor=SHORT[:32]))),
    ("long_factor", dict(rope_parameters={k: v for k, v in LONGROPE.items() if k != "long_factor"})),
    ("original_max_position_embeddings", dict(rope_parameters={k: v for k, v in LONGROPE.items() if k != "original_max_position_embeddings"})),
]
GLM4_REFUSALS = [
    ("head_dim", dict(head_dim=96)),
    ("partial_rotary_factor", dict(rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.53125))),     # 68 of 128: no multiple of 8
    ("hidden_act", dict(hidden_act="gelu")),
    ("rope_type", dict(rope_parameters=dict(LONGROPE, partial_rotary_factor=0.75))),                       # longrope is Phi-3's
]


def _refused(geo, model_type, field, change):
    d = make_config(dict(geo, model_type=model_type, hidden_act="silu"))
    check_supported(d)
    for k, v in change.items():
        setattr(d, k, v)
    with pytest.raises(ValueError, match=field):
        check_supported(d)
    return d


@pytest.mark.parametrize("field,change", PHI3_REFUSALS)
def test_check_supported_refuses_phi3_and_names_the_field(field, change):
    d = _refused(dict(PHI3_A, rope_parameters=dict(LONGROPE)), "phi3", field, change)
    if field in ("resid_pdrop", "embd_pdrop", "attention_dropout"):
        check_supported(d, training=False)                                    # an evaluation-mode model has no dropout
    if field == "head_dim" and change["head_dim"] == 96:
        with pytest.raises(ValueError, match="Phi-3-mini"):
            check_supported(d)


@pytest.mark.parametrize("field,change", GLM4_REFUSALS)
def test_check_supported_refuses_glm4_and_names_the_field(field, change):
    _refused(GLM4_A, "glm4", field, change)


def test_accepted_rotary_dimensions():
    for mt, geo, step in (("phi3", PHI3_C, 16), ("glm4", GLM4_A, 8)):
        for D in (64, 128):
            for R in range(8, D + 1, 8):
                d = make_config(dict(geo, model_type=mt, head_dim=D, hidden_act="silu", rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=R / D)))
                assert rotary_dim(d) == R
                if R % step == 0:
                    check_supported(d)
                else:
                    with pytest.raises(ValueError, match="partial_rotary_factor"):
                        check_supported(d)


@pytest.mark.parametrize("model_type", [None, "llama", "mistral", "qwen3", "olmo2", "gemma2", "glm", "phi"])
def test_the_same_settings_on_any_other_model_type_stay_refused(model_type):
    kw = dict(LLAMA, head_dim=128, hidden_act="silu")
    if model_type is not None:
        kw["model_type"] = model_type
    if model_type == "gemma2":
        kw.update(hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=128)
    with pytest.raises(ValueError, match="partial_rotary_factor"):
        check_supported(make_config(dict(kw, rope_parameters=dict(DEFAULT_ROPE, partial_rotary_factor=0.75))))
    with pytest.raises(ValueError, match="partial_rotary_factor"):
        check_supported(make_config(dict(kw, partial_rotary_factor=0.5)))
    with pytest.raises(ValueError, match="rope_type"):
        check_supported(make_config(dict(kw, rope_parameters=dict(LONGROPE, partial_rotary_factor=1.0, short_factor=[1.0] * 64, long_factor=[2.0] * 64))))


def test_glm4_footprint_counts_the_two_post_branch_norm_outputs():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    c = hf_config("glm4_a")
    e = TreeTrainingEngine(c, torch.device("cpu"), torch.float32, 128)
    plain = make_config({k: v for k, v in c.to_dict().items() if k != "model_type"})
    mk = lambda cfg: type("M", (), {"config": cfg, "named_modules": lambda self: iter(())})()
    assert e._per_token_layer_bytes(mk(c)) == e._per_token_layer_bytes(mk(plain)) + 2 * 2 * c.hidden_size
    p = hf_config("phi3_c")
    assert e._per_token_layer_bytes(mk(p)) == e._per_token_layer_bytes(mk(make_config({k: v for k, v in p.to_dict().items() if k != "model_type"})))


def test_lora_on_the_fused_modules_stays_refused():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import lora
    hf = hf_model("phi3_c")
    lora.attach(hf, 4, 8.0, ("o_proj", "down_proj"), seed=1)
    lora.check_supported(hf)
    for parent, name in (("self_attn", "qkv_proj"), ("mlp", "gate_up_proj")):
        hf = hf_model("phi3_c")
        p = getattr(hf.model.layers[0], parent)
        setattr(p, name, lora.LoraLinear(getattr(p, name), 4, 8.0))
        with pytest.raises(ValueError, match=name + ".*adapter on this module is not supported"):
            lora.check_supported(hf)
