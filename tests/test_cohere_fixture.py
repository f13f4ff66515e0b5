"""Cohere / Cohere2: the tiny configurations behind tests/golden/engine_cohere.pt (scripts/make_golden_cohere.py: the REFERENCE's
dense per-sequence path over unmodified transformers CohereForCausalLM / Cohere2ForCausalLM models in fp32 on the CPU, eager
attention), the checks of the fixture, of the model layer's configuration rules, and the engine on the CPU against the fixture in
packed mode and in the block-wise walk.

Every model has vocabulary 256, intermediate size 64 and head_dim passed explicitly; the hidden sizes of the two cohere2 cases are
small so that the four records stay under 1 MiB together:

* cohere_a:   CohereForCausalLM, 2 layers, hidden 64, 4 / 2 heads of 128, tied head, logit_scale 0.25.
* cohere_b:   hidden 48, 6 / 2 heads of 64, attention_bias (q, k, v and o), untied head, logit_scale 0.3 (no power of two).
* cohere2_a:  Cohere2ForCausalLM, 4 layers [sliding, sliding, sliding, full], hidden 8, 4 / 2 heads of 128, sliding_window 8: the
              full layer applies no RoPE.
* cohere2_b:  2 layers [sliding, full], hidden 8, 3 / 1 heads of 64, logit_scale 0.125.  Both cohere2 cases have an untied head.

The embedding rows carry a common offset (EMBED_OFFSET), so that the rows the first norm sees are far from centred: a norm without
the mean subtraction computes something else.

Every record also holds HF's logprobs with ONE feature removed (OFF) and the fixture must keep each max |fwd_dense - fwd_dense_off_*|
>= 0.4 (MIN_GAP of tests/test_llama_family_fixture.py): a run that ignores the feature cannot pass the bf16 forward bound.
tests/test_gpu_engine_cohere.py runs the product engine on these cases."""
import contextlib
import copy
import os

import pytest
import torch

import cohere_host
import family
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import (_cfg_of, _windows_of, check_supported, ensure_supported, is_cohere, is_glm4, is_olmo, is_phi3, logit_scale_of,
                                       make_config, rope_of)
from family import _m, att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden_cohere.py read them here)
from test_llama_family_fixture import LLAMA, MIN_GAP

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILE = "engine_cohere.pt"
NORM_STD, EMBED_OFFSET = 0.1, 0.3        # norm weights 1 + N(0, NORM_STD); embedding rows N(0, std) + EMBED_OFFSET
# case -> (std of the matrices and biases, of q_proj / k_proj, of v_proj / o_proj, of an untied lm_head).  The q / k scale sets how sharp the attention is
# (the score's spread grows with qk_std^2 hidden sqrt(head_dim)) - sharp enough for the rotation, the window and the table-less layers
# to move the weights - and the v / o scale how far the attention branch moves the stream.  The head's scale sets the spread of the
# logits: at hidden 8 / 16 and a logit scale of 0.25 / 0.125 a head at the matrices' scale leaves every logprob within 0.1 of
# -log(256), and no feature could move one by MIN_GAP.  Each was lowered until HF's own bf16 run sits inside the bf16 bounds
# (scripts/make_golden_cohere.py asserts both conditions).
CASE_STD = {"cohere_a": (0.1, 0.15, 0.2, 0.1), "cohere_b": (0.1, 0.15, 0.2, 0.1), "cohere2_a": (0.1, 0.3, 0.3, 1.0), "cohere2_b": (0.1, 0.25, 0.3, 2.0)}
WINDOW = 8
BASE = dict(vocab_size=256, intermediate_size=64, layer_norm_eps=1e-5, max_position_embeddings=256, pad_token_id=None, eos_token_id=None,
            bos_token_id=None, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
COHERE_A = dict(BASE, num_hidden_layers=2, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=True,
                logit_scale=0.25)
COHERE_B = dict(BASE, num_hidden_layers=2, hidden_size=48, num_attention_heads=6, num_key_value_heads=2, head_dim=64, tie_word_embeddings=False,
                attention_bias=True, logit_scale=0.3)
COHERE2_A = dict(BASE, num_hidden_layers=4, hidden_size=8, num_attention_heads=4, num_key_value_heads=2, head_dim=128, tie_word_embeddings=False,
                 logit_scale=0.25, sliding_window=WINDOW, layer_types=["sliding_attention"] * 3 + ["full_attention"])
COHERE2_B = dict(BASE, num_hidden_layers=2, hidden_size=8, num_attention_heads=3, num_key_value_heads=1, head_dim=64, tie_word_embeddings=False,
                 logit_scale=0.125, sliding_window=WINDOW, layer_types=["sliding_attention", "full_attention"])
DATA = {"kind": "tau2", "seed": 6, "V": 256, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 128}
# case -> (HF class stem, geometry, data, weight seed)
CASES = {"cohere_a": ("Cohere", COHERE_A, DATA, 51), "cohere_b": ("Cohere", COHERE_B, DATA, 52),
         "cohere2_a": ("Cohere2", COHERE2_A, DATA, 53), "cohere2_b": ("Cohere2", COHERE2_B, DATA, 54)}
# feature removed -> the configuration change that removes it; {} = not a configuration: hf_run_with patches the running HF model
OFF = {"logit_scale": dict(logit_scale=1.0), "window": dict(sliding_window=4096), "centering": {}, "interleaved": {}, "nope": {}}


def offs_of(case):
    return ["logit_scale", "centering", "interleaved"] + (["window", "nope"] if case.startswith("cohere2") else [])


def hf_config(case, off=None, attn="eager", **change):
    """The case's CohereConfig / Cohere2Config; `off`: one of OFF (that feature removed); further fields through `change`."""
    import transformers
    kw = copy.deepcopy(CASES[case][1])
    if off:
        kw.update(copy.deepcopy(OFF[off]))
    kw.update(change)
    c = getattr(transformers, CASES[case][0] + "Config")(**kw)
    c._attn_implementation = attn
    return c


def weights(model, seed, std, qk_std, vo_std, head_std):
    """Seeded fp32 weights for every parameter of `model`, by name in named_parameters order: norm weights 1 + N(0, NORM_STD), the
    embedding rows EMBED_OFFSET + N(0, std), q_proj / k_proj weights N(0, qk_std), v_proj / o_proj weights N(0, vo_std), an untied
    lm_head N(0, head_std), every other matrix and bias N(0, std)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        if n.endswith(("norm.weight", "layernorm.weight")):
            out[n] = 1.0 + NORM_STD * torch.randn(p.shape, generator=g)
        elif n.endswith(("q_proj.weight", "k_proj.weight")):
            out[n] = qk_std * torch.randn(p.shape, generator=g)
        elif n.endswith(("v_proj.weight", "o_proj.weight")):
            out[n] = vo_std * torch.randn(p.shape, generator=g)
        elif n == "lm_head.weight":
            out[n] = head_std * torch.randn(p.shape, generator=g)
        else:
            out[n] = std * torch.randn(p.shape, generator=g) + (EMBED_OFFSET if n.endswith("embed_tokens.weight") else 0.0)
    return out


def hf_model(case, off=None, attn="eager", **change):
    """The unmodified transformers model of `case` with the seeded weights (fp32, train mode)."""
    import transformers
    m = getattr(transformers, CASES[case][0] + "ForCausalLM")(hf_config(case, off, attn, **change))
    return family.load_weights(m, weights(m, CASES[case][3], *CASE_STD[case]))


def _modeling(stem):
    import importlib
    return importlib.import_module(f"transformers.models.{stem.lower()}.modeling_{stem.lower()}")


@contextlib.contextmanager
def hf_run_with(off, model=None):
    """While the block runs, transformers' Cohere and Cohere2 compute without one feature: "centering" - the norm without the mean
    subtraction; "interleaved" - half-split rotation pairs (i, i + D/2) on the same frequencies; "nope" (`model`: the Cohere2 model) -
    its full-attention layers rotate too (their mask stays the causal one).  Any other `off` is a configuration: nothing is patched."""
    undo = []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    if off == "centering":
        def uncentred(self, hidden_states):
            x = hidden_states.to(torch.float32)
            x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
            return (self.weight.to(torch.float32) * x).to(hidden_states.dtype)
        for stem in ("Cohere", "Cohere2"):
            patch(getattr(_modeling(stem), stem + "LayerNorm"), "forward", uncentred)
    elif off == "interleaved":
        def half_split(q, k, cos, sin, unsqueeze_dim=1):
            c, s = cos[..., ::2].unsqueeze(unsqueeze_dim), sin[..., ::2].unsqueeze(unsqueeze_dim)       # the table repeats every frequency twice
            cos2, sin2 = torch.cat([c, c], -1), torch.cat([s, s], -1)
            rot = lambda x: torch.cat([-x[..., x.shape[-1] // 2:], x[..., :x.shape[-1] // 2]], -1)
            qf, kf = q.float(), k.float()
            return (qf * cos2 + rot(qf) * sin2).to(q.dtype), (kf * cos2 + rot(kf) * sin2).to(k.dtype)
        for stem in ("Cohere", "Cohere2"):
            patch(_modeling(stem), "apply_rotary_pos_emb", half_split)
    elif off == "nope":
        for layer in model.model.layers:
            if layer.self_attn.sliding_window is None:
                patch(layer.self_attn, "sliding_window", 1 << 20)          # Cohere2Attention rotates when this is set; eager attention ignores it
    try:
        yield
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)


def llama_control(case):
    """Llama-shaped wiring of the same sizes (RMSNorm, sequential block, rotate-half RoPE, no window, no bias, no logit scale) with
    weights from the same helper: the control of the fp32 GPU test - what the engine's gradients deviate by on a model of this size
    without any of this family's features."""
    import transformers
    geo = {k: v for k, v in CASES[case][1].items() if k not in ("sliding_window", "layer_types", "attention_bias", "logit_scale", "layer_norm_eps")}
    heads = geo.pop("num_attention_heads")
    # (LlamaConfig wants hidden_size to be a multiple of the head count when it is built, also with an explicit head_dim: cohere2_b's
    # 3 heads at hidden 8 go in afterwards)
    c = transformers.LlamaConfig(**geo, num_attention_heads=geo["num_key_value_heads"], rms_norm_eps=1e-5)
    c.num_attention_heads = heads
    c._attn_implementation = "eager"
    m = transformers.LlamaForCausalLM(c)
    return family.load_weights(m, weights(m, CASES[case][3], *CASE_STD[case]))


def seqs_of(case):
    return synth.make_case(CASES[case][2])


def gold(case):
    return torch.load(os.path.join(GOLD, FILE), weights_only=True)[case]


# ---------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_names_shapes_and_feature_gaps(case):
    pytest.importorskip("transformers")
    g = gold(case)
    grads = gold_grads(g)
    model = hf_model(case)
    c = model.config
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {n: tuple(v.shape) for n, v in grads.items()}
    assert ("lm_head.weight" in grads) == (case != "cohere_a")                # cohere_a ties the head
    assert ("model.layers.0.self_attn.o_proj.bias" in grads) == (case == "cohere_b")
    assert not any("post_attention_layernorm" in n or "q_norm" in n for n in grads)      # one norm per layer, no q/k norm
    assert sum(n.endswith("layernorm.weight") for n in grads) == c.num_hidden_layers and "model.norm.weight" in grads
    assert c.vocab_size % 8 == 0 and c.hidden_size % 8 == 0
    seqs = seqs_of(case)
    assert len(seqs) >= 9 and len(g["fwd_dense"]) == len(seqs) and max(map(len, seqs)) > 3 * WINDOW
    assert {k for k in g if k.startswith("fwd_dense_off_")} == {"fwd_dense_off_" + o for o in offs_of(case)}
    for off in offs_of(case):
        assert g["fwd_dense_off_" + off].shape == (sum(len(s) - 1 for s in seqs),)                     # the sequences' logprobs, concatenated
        gap = _dist(g["fwd_dense"], g["fwd_dense_off_" + off])
        assert gap >= MIN_GAP, (off, gap)
    assert all(v > 0 for v in g["grad_norms"].values())
    assert os.path.getsize(os.path.join(GOLD, FILE)) < (1 << 20)


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
    every gradient, in one packed pass and in the block-wise walk: the layer wiring (one norm, two pending updates joined in the next
    norm, the table-less full layers, the windows, the biases, the logit scale on its way to the head) is host-side plumbing."""
    pytest.importorskip("transformers")
    g = gold(case)
    cohere_host.install(monkeypatch)
    named = family.check_cpu_engine_matches_fixture(hf_model(case), synth.as_tensors(seqs_of(case)), g, monkeypatch, mode=mode)
    assert set(named) == set(gold_grads(g))


def _cpu_forward(hf, seqs, monkeypatch):
    import hostmirror
    from dynamictreeattn_amd.token_trie import TokenTrie
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    cohere_host.install(monkeypatch)
    hostmirror.install(monkeypatch)
    cpu = torch.device("cpu")
    t = TokenTrie(seqs, device=cpu); t.forward_permute()
    return TreeTrainingEngine(hf.config, cpu, torch.float32, max(map(len, seqs)), forward_only=True).forward(hf, t)


def _dist(out, rec):
    """max |out - rec| of per-sequence logprobs against a record: fwd_dense (a list) or a fwd_dense_off_* (one concatenated tensor)."""
    return float((torch.cat(list(out)) - (rec if isinstance(rec, torch.Tensor) else torch.cat(list(rec)))).abs().max())


def test_a_logit_scale_left_out_misses_the_fixture(monkeypatch):
    """The logit scale is not inert: cohere_b run with logit_scale 1.0 is off the fixture by the recorded gap and equals the
    fwd_dense_off_logit_scale record."""
    pytest.importorskip("transformers")
    g = gold("cohere_b")
    out = _cpu_forward(hf_model("cohere_b", "logit_scale"), synth.as_tensors(seqs_of("cohere_b")), monkeypatch)
    assert _dist(out, g["fwd_dense"]) >= MIN_GAP and _dist(out, g["fwd_dense_off_logit_scale"]) < 1e-4


def test_centring_left_out_misses_the_fixture(monkeypatch):
    """cohere_a with a norm that does not subtract the mean (the stand-in replaced by an uncentred one) is off the fixture by the
    recorded gap and equals the fwd_dense_off_centering record."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import ops
    g = gold("cohere_a")
    cohere_host.install(monkeypatch)

    def uncentred(x, da, db, w, eps):
        x = x + (da if da is not None else 0) + (db if db is not None else 0)
        xf = x.float()
        return x, (w.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps))).to(x.dtype)
    monkeypatch.setattr(ops, "add_layer_norm", uncentred)
    out = _cpu_forward_installed(hf_model("cohere_a"), synth.as_tensors(seqs_of("cohere_a")), monkeypatch)
    assert _dist(out, g["fwd_dense"]) >= MIN_GAP and _dist(out, g["fwd_dense_off_centering"]) < 1e-4


def _cpu_forward_installed(hf, seqs, monkeypatch):
    """_cpu_forward without installing cohere_host again (the caller has, and has replaced one of its stand-ins)."""
    import hostmirror
    from dynamictreeattn_amd.token_trie import TokenTrie
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    hostmirror.install(monkeypatch)
    cpu = torch.device("cpu")
    t = TokenTrie(seqs, device=cpu); t.forward_permute()
    return TreeTrainingEngine(hf.config, cpu, torch.float32, max(map(len, seqs)), forward_only=True).forward(hf, t)


def test_rotating_full_layers_misses_the_fixture(monkeypatch):
    """NoPE is not inert: cohere2_a with its full-attention layer typed as rotating (the engine hands every layer a table when the
    model is typed cohere, not cohere2 - here by a model whose layer hands the table on) equals the fwd_dense_off_nope record."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import model as M
    g = gold("cohere2_a")
    cohere_host.install(monkeypatch)
    real = M._cohere_layer_forward
    table = {}

    def always_rotate(layer, res, da, db, cos_sin, *rest):
        if cos_sin is not None:
            table["cs"] = cos_sin
        return real(layer, res, da, db, table["cs"], *rest)
    monkeypatch.setattr(M, "_cohere_layer_forward", always_rotate)
    out = _cpu_forward_installed(hf_model("cohere2_a"), synth.as_tensors(seqs_of("cohere2_a")), monkeypatch)
    assert _dist(out, g["fwd_dense"]) >= MIN_GAP and _dist(out, g["fwd_dense_off_nope"]) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- configuration rules
@pytest.mark.parametrize("case", list(CASES))
def test_check_supported_accepts_the_cases(case):
    pytest.importorskip("transformers")
    c = hf_config(case)
    assert is_cohere(c) and c.model_type == CASES[case][0].lower()
    assert not (is_phi3(c) or is_glm4(c) or is_olmo(c))
    check_supported(c)
    for off in offs_of(case):
        check_supported(hf_config(case, off))
    hf = hf_model(case)
    ensure_supported(hf)
    assert logit_scale_of(hf) == c.logit_scale and _cfg_of(hf)[3] == 1e-5
    assert torch.equal(rope_of(c)[0], hf.model.rotary_emb.inv_freq) and rope_of(c)[0].shape == (c.head_dim // 2,)


def test_eps_comes_from_layer_norm_eps():
    d = make_config(dict(COHERE_A, model_type="cohere", hidden_act="silu", layer_norm_eps=3e-4, rms_norm_eps=1e-6))
    assert _cfg_of(_m(d))[3] == 3e-4
    assert _cfg_of(_m(make_config(dict(LLAMA, layer_norm_eps=3e-4))))[3] != 3e-4           # nobody else reads the field


def test_predicates_are_keyed_on_the_model_type_alone():
    assert not is_cohere(make_config(dict(LLAMA)))
    assert is_cohere(make_config(dict(LLAMA, model_type="cohere"))) and is_cohere(make_config(dict(LLAMA, model_type="cohere2")))
    assert not is_cohere(make_config(dict(LLAMA, model_type="cohere3"))) and not is_cohere(make_config(dict(LLAMA, logit_scale=0.25, layer_norm_eps=1e-5)))
    assert logit_scale_of(_m(make_config(dict(LLAMA, logit_scale=0.25)))) == 1.0           # the field on any other model type is not read
    assert logit_scale_of(_m(make_config(dict(LLAMA, model_type="cohere", logit_scale=0.25)))) == 0.25


def test_windows_of_cohere2_follow_the_layer_types():
    pytest.importorskip("transformers")
    assert _windows_of(_m(hf_config("cohere2_a"))) == [8, 8, 8, 0]
    assert _windows_of(_m(hf_config("cohere2_b"))) == [8, 0]
    assert _windows_of(_m(hf_config("cohere2_a", "window"))) == [4096, 4096, 4096, 0]
    assert _windows_of(_m(hf_config("cohere_a"))) == [0, 0] and _windows_of(_m(hf_config("cohere_b"))) == [0, 0]


COHERE_REFUSALS = [
    ("head_dim", dict(head_dim=96)),
    ("head_dim", dict(head_dim=256)),
    ("hidden_size", dict(hidden_size=60)),                                     # off 8
    ("hidden_size.*Command-R\\+", dict(hidden_size=12288)),                    # Command-R+ / Command-A
    ("use_qk_norm.*Command-R\\+", dict(use_qk_norm=True)),
    ("logit_scale", dict(logit_scale=0.0)),
    ("logit_scale", dict(logit_scale=-0.25)),
    ("logit_scale", dict(logit_scale=float("inf"))),
    ("logit_scale", dict(logit_scale=float("nan"))),
    ("logit_scale", dict(logit_scale=None)),
    ("hidden_act", dict(hidden_act="gelu")),
    ("attention_dropout", dict(attention_dropout=0.1)),
    ("rope_type", dict(rope_parameters={"rope_type": "dynamic", "rope_theta": 10000.0, "factor": 2.0})),
]
COHERE2_REFUSALS = COHERE_REFUSALS + [
    ("layer_types", dict(layer_types=["sliding_attention", "chunked_attention", "sliding_attention", "full_attention"])),
    ("layer_types", dict(layer_types=["sliding_attention", "full_attention"])),                             # two entries for four layers
    ("layer_types", dict(layer_types=None)),
    ("sliding_window", dict(sliding_window=None)),
    ("sliding_window", dict(sliding_window=0)),
]


def _refused(geo, model_type, field, change):
    d = make_config(dict(geo, model_type=model_type, hidden_act="silu"))
    check_supported(d)
    for k, v in change.items():
        setattr(d, k, v)
    with pytest.raises(ValueError, match=field):
        check_supported(d)
    return d


@pytest.mark.parametrize("field,change", COHERE_REFUSALS)
def test_check_supported_refuses_cohere_and_names_the_field(field, change):
    d = _refused(COHERE_A, "cohere", field, change)
    if field == "attention_dropout":
        check_supported(d, training=False)


@pytest.mark.parametrize("field,change", COHERE2_REFUSALS)
def test_check_supported_refuses_cohere2_and_names_the_field(field, change):
    _refused(COHERE2_A, "cohere2", field, change)


def test_attention_bias_and_a_full_only_cohere2_are_accepted():
    check_supported(make_config(dict(COHERE_B, model_type="cohere", hidden_act="silu")))
    d = make_config(dict(COHERE2_B, model_type="cohere2", hidden_act="silu", layer_types=["full_attention"] * 2, sliding_window=None))
    check_supported(d)                                                        # no layer slides: no window needed
    assert _windows_of(_m(d)) == [0, 0]


def test_cohere_footprint_counts_one_norm_per_layer():
    """The footprint rule: a Cohere layer keeps the joined stream and ONE norm output - two hidden rows fewer than a pre-norm layer."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    c = hf_config("cohere_a")
    e = TreeTrainingEngine(c, torch.device("cpu"), torch.float32, 128)
    plain = make_config({k: v for k, v in c.to_dict().items() if k != "model_type"})
    mk = lambda cfg: type("M", (), {"config": cfg, "named_modules": lambda self: iter(())})()
    assert e._per_token_layer_bytes(mk(c)) == e._per_token_layer_bytes(mk(plain)) - 2 * 2 * c.hidden_size


def test_parameter_tree_of_a_cohere_configuration():
    """Qwen3TreeLM on a cohere / cohere2 configuration: HF's names - one norm per layer, no q/k norms, tied head."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.model import Qwen3TreeLM
    for case in ("cohere_a", "cohere2_b"):
        hf = hf_model(case)
        own = Qwen3TreeLM(make_config(dict(CASES[case][1], model_type=hf.config.model_type, hidden_act="silu")))
        theirs = {n: tuple(p.shape) for n, p in hf.named_parameters() if n != "lm_head.weight"}      # (Qwen3TreeLM ties the head)
        assert {n: tuple(p.shape) for n, p in own.named_parameters()} == theirs
    plain = Qwen3TreeLM(make_config(dict(COHERE_A, model_type="llama")))
    assert "model.layers.0.post_attention_layernorm.weight" in dict(plain.named_parameters())


# ---------------------------------------------------------------------------------------------------------------- LoRA
def test_lora_on_all_seven_projections_matches_hf(monkeypatch):
    """lora.attach on the seven projections of cohere_a: lora.check_supported accepts them, and the CPU engine reproduces HF's own
    dense run of the adapted model (family.hf_dense, computed here) - logprobs, loss, and every adapter's gradient; the base is frozen."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import lora
    from oracle import model_oracle as mo
    targets = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
    seqs = synth.as_tensors(seqs_of("cohere_a"))[:5]
    models = []
    for _ in range(2):
        hf = hf_model("cohere_a")
        lora.attach(hf, 4, 8.0, targets, seed=3)
        with torch.no_grad():
            g = torch.Generator().manual_seed(9)
            for n, p in hf.named_parameters():
                if "lora_B" in n:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g))          # (B starts at zero: the adapters would be inert)
        lora.check_supported(hf)
        ensure_supported(hf)
        models.append(hf)
    ref, mine = models
    lps, loss_r = family.hf_dense(ref, seqs, att(len(seqs)), device="cpu")
    cohere_host.install(monkeypatch)
    import hostmirror
    hostmirror.install(monkeypatch)
    out, loss, _ = family.run_engine(mine, seqs, att(len(seqs)), torch.float32, "packed", 2048, monkeypatch, device=family.CPU)
    assert _dist(out, lps) < 1e-4 and abs(loss - loss_r) < 1e-4 * abs(loss_r)
    rg = {n: p.grad for n, p in ref.named_parameters() if p.requires_grad}
    got = {n: p.grad for n, p in mine.named_parameters() if p.grad is not None}
    assert set(got) == set(rg) and all("lora_" in n for n in rg) and len(rg) == 2 * 7 * 2
    for n in rg:
        assert mo.grad_ratio(rg[n], got[n]) <= 1e-3, n
