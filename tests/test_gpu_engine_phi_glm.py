"""Phi-3 / Phi-4 and GLM-4 through the engine on the GPU: UNMODIFIED transformers Phi3ForCausalLM / Glm4ForCausalLM models
(tests/test_phi_glm_fixture.py: fused qkv_proj / gate_up_proj, rotary dimensions 96 and 48 of 128 and 64 in half-split pairs, longrope,
a window on every layer; interleaved pairs over 64 and 32 elements, q/k/v biases, four norms per layer) in packed mode and the
block-wise stack walk - the protocol of tests/family.py with the numeric bounds of tests/test_gpu_engine_olmo.py.

* fp32 against HF's own eager attention in float64 on the card: logprobs within 1e-4, loss within 1e-5, every gradient within
  max(1e-4, 1.5 x control) and 1e-3, where the control is the same engine on Llama-shaped wiring of the same sizes
  (test_phi_glm_fixture.llama_control).
* bf16 against the fixture the reference computed (loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN, logprobs 0.08 / 0.015).
* tree equals dense on the device; per-layer recomputation with kept attention outputs gives the gradients of the plain pass bit
  for bit.
* longrope: a trie of sequences up to original_max_position_embeddings matches HF on the short factors, one of longer sequences on
  the long factors; a mixed trie is refused under "auto" and under "long" equals HF with the long table forced.
* LoRA adapters on o_proj / down_proj of phi3_a."""
import pytest
import torch

import family
import test_phi_glm_fixture as fx
from dynamictreeattn_amd import lora, synth
from dynamictreeattn_amd.model import rope_of
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("packed", 2048), ("stack", 16)]


def _seqs(case):
    return synth.as_tensors(fx.seqs_of(case))


def _fp32_run(model32, case, mode, monkeypatch):
    """family.fp32_against_hf64 on the case's sequences: (logprob error, loss, reference loss, ratios)."""
    seqs = _seqs(case)
    lp_err, loss, loss_r, ratios, names = family.fp32_against_hf64(model32, seqs, family.att(len(seqs)), mode, monkeypatch)
    return lp_err, loss, loss_r, ratios


def _control_of(name, control):
    """The control's ratio for parameter `name`: its namesake's; for a fused module the worst of the modules it fuses (its gradient
    is their gradients stacked); for a bias its weight's; 0 for a parameter the Llama wiring has no counterpart of (GLM-4's two
    post-branch norms), which leaves the 1e-4 floor."""
    parts = {"qkv_proj": ("q_proj", "k_proj", "v_proj"), "gate_up_proj": ("gate_proj", "up_proj")}
    name = name.replace(".bias", ".weight")
    for fused, members in parts.items():
        if fused in name:
            return max(control[name.replace(fused, m_)] for m_ in members)
    return control.get(name, 0.0)


@pytest.mark.parametrize("mode", ["packed", "stack"])
@pytest.mark.parametrize("case", list(fx.CASES))
def test_fp32_against_hf_eager_in_float64(case, mode, monkeypatch):
    pytest.importorskip("transformers")
    lp_err, loss, loss_r, ratios = _fp32_run(fx.hf_model(case), case, mode, monkeypatch)
    print(f"{case}/{mode}: logprob err {lp_err:.2e}, loss rel {abs(loss - loss_r) / abs(loss_r):.2e}, worst ratio "
          f"{max(ratios.items(), key=lambda kv: kv[1])}")
    assert lp_err < 1e-4
    assert abs(loss - loss_r) <= 1e-5 * abs(loss_r)
    lp_c, loss_c, loss_cr, control = _fp32_run(fx.llama_control(case), case, mode, monkeypatch)
    assert abs(loss_c - loss) > 1e-5 * abs(loss)                      # these families' wiring changes the loss: not an inert case
    assert lp_c < 1e-4 and abs(loss_c - loss_cr) <= 1e-5 * abs(loss_cr)
    ctl = {n: _control_of(n, control) for n in ratios}
    bad = {n: (r, ctl[n]) for n, r in ratios.items() if r > max(1e-4, 1.5 * ctl[n])}
    print(f"{case}/{mode}: control worst {max(control.values()):.2e}; above the rule: {bad}")
    assert not bad, bad
    assert max(ratios.values()) <= 1e-3


@pytest.mark.parametrize("mode,bs", MODES)
@pytest.mark.parametrize("case", list(fx.CASES))
def test_bf16_against_the_reference_fixture(case, mode, bs, monkeypatch):
    pytest.importorskip("transformers")
    hf = fx.hf_model(case).to(device=DEV, dtype=torch.bfloat16).train()
    g = fx.gold(case)
    named = family.check_bf16_against_fixture(hf, _seqs(case), g, mode, bs, monkeypatch, label=case)
    assert set(named) == set(fx.gold_grads(g))


@pytest.mark.parametrize("case", list(fx.CASES))
def test_tree_equals_dense_on_the_device(case):
    """dense.backward (one pass per sequence, the stack form) against engine.backward (one packed pass) in fp32."""
    pytest.importorskip("transformers")
    family.check_tree_equals_dense(fx.hf_model(case).to(DEV), fx.hf_model(case).to(DEV), _seqs(case))


@pytest.mark.parametrize("case", list(fx.CASES))
def test_recomputation_with_kept_attention_outputs_changes_nothing(case, monkeypatch):
    pytest.importorskip("transformers")
    family.check_recompute_is_bitwise(fx.hf_model(case).to(device=DEV, dtype=torch.bfloat16).train(), _seqs(case), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- longrope
def _longrope_seqs():
    g = torch.Generator().manual_seed(3)
    head = torch.randint(0, 256, (6,), generator=g)
    mk = lambda n: torch.cat([head, torch.randint(0, 256, (n - 6,), generator=g)])
    return [mk(n) for n in (9, 16, 12, 14)], [mk(n) for n in (17, 40, 33)]


def _forward(hf, seqs, **attrs):
    t = TokenTrie(seqs); t.forward_permute()
    e = TreeTrainingEngine(hf.config, DEV, torch.float32, max(map(len, seqs)), forward_only=True)
    for k, v in attrs.items():
        setattr(e, k, v)
    return [o.cpu() for o in e.forward(hf, t)]


def _hf64(seqs, force_long=False):
    ref = fx.hf_model("phi3_a").double().to(DEV)
    if force_long:                                 # HF with the long table for every length
        ref.model.rotary_emb.original_inv_freq = rope_of(ref.config, long=True)[0].to(DEV)
    return ref, family.hf_dense(ref, seqs, family.att(len(seqs)))


@pytest.mark.parametrize("which", ["short", "long"])
def test_longrope_trie_on_one_side_matches_hf(which, monkeypatch):
    """Sequences all up to original_max_position_embeddings (16): HF's short factors; all longer: the long ones - logprobs, loss and
    gradients of the fp32 engine under "auto" against HF eager in float64."""
    pytest.importorskip("transformers")
    short, long = _longrope_seqs()
    seqs = short if which == "short" else long
    ref, (lps, loss_r) = _hf64(seqs)
    hf = fx.hf_model("phi3_a").to(DEV)
    out, loss, e = family.run_engine(hf, seqs, family.att(len(seqs)), torch.float32, "packed", 2048, monkeypatch)
    assert e.longrope_factors == "auto"
    assert max(float((a - b).abs().max()) for a, b in zip(out, lps)) < 1e-4
    assert abs(loss - loss_r) <= 1e-5 * abs(loss_r)
    from oracle import model_oracle as mo
    rg = dict(ref.named_parameters())
    assert max(mo.grad_ratio(rg[n].grad.float(), p.grad) for n, p in hf.named_parameters()) <= 1e-3
    # and the other set is another model: forcing it misses the bound
    other = _forward(hf, seqs, longrope_factors="long" if which == "short" else "short")
    assert max(float((a - b).abs().max()) for a, b in zip(other, lps)) > 1e-3


def test_longrope_mixed_trie_is_refused_under_auto_and_runs_under_long():
    pytest.importorskip("transformers")
    short, long = _longrope_seqs()
    seqs = short + long
    hf = fx.hf_model("phi3_a").to(DEV)
    with pytest.raises(ValueError, match="original_max_position_embeddings.*longrope_factors"):
        _forward(hf, seqs)
    out = _forward(hf, seqs, longrope_factors="long")
    _, (lps, _) = _hf64(seqs, force_long=True)
    assert max(float((a - b).abs().max()) for a, b in zip(out, lps)) < 1e-4
    _, (lps_hf, _) = _hf64(short)                                     # HF's own choice for the short ones is the other table
    assert max(float((a - b).abs().max()) for a, b in zip(out[:len(short)], lps_hf)) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- LoRA
@pytest.mark.parametrize("mode,bs", MODES)
def test_lora_adapters_on_o_proj_and_down_proj_of_phi3(mode, bs, monkeypatch):
    """Adapters on the two single projections of a Phi-3 layer: with B = 0 the loss is the plain model's bit for bit, the adapters and
    only they get gradients; with B set, logprobs, loss and adapter gradients are within the bounds of tests/test_gpu_engine_lora.py
    (1e-4, 1e-5, max(1e-4, 1.5 x control) and 1e-3) of HF's own forward over the wrapped modules in float64."""
    pytest.importorskip("transformers")
    seqs = _seqs("phi3_a")
    att = family.att(len(seqs))
    plain = fx.hf_model("phi3_a").to(device=DEV, dtype=torch.bfloat16).train()
    _, loss_plain, _ = family.run_engine(plain, seqs, att, torch.bfloat16, mode, bs, monkeypatch, forward=False)
    hf = fx.hf_model("phi3_a")
    params = lora.attach(hf, 4, 8.0, ("o_proj", "down_proj"), seed=1)
    hf = hf.to(device=DEV, dtype=torch.bfloat16).train()
    lora.check_supported(hf)
    adapters = {n for n, p in hf.named_parameters() if p.requires_grad}
    assert len(adapters) == len(params) == 2 * 2 * hf.config.num_hidden_layers
    _, loss, e = family.run_engine(hf, seqs, att, torch.bfloat16, mode, bs, monkeypatch, forward=False)
    assert e.last_mode.startswith(mode)
    assert loss == loss_plain                                           # B = 0: the adapted model IS the plain one
    got = {n for n, p in hf.named_parameters() if p.grad is not None}
    assert got == adapters and all(p.grad is None for n, p in hf.named_parameters() if n not in adapters)
    assert all(bool(torch.isfinite(p.grad).all()) for n, p in hf.named_parameters() if n in adapters)
    assert any(float(p.grad.float().abs().max()) > 0 for n, p in hf.named_parameters() if "lora_B" in n)
    # B set: fp32 engine against HF's forward of the wrapped modules in float64
    m32 = fx.hf_model("phi3_a")
    lora.attach(m32, 4, 8.0, ("o_proj", "down_proj"), seed=1)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in m32.named_parameters():
            if "lora_B" in n:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    sd = {k: v.clone() for k, v in m32.state_dict().items()}
    ref = fx.hf_model("phi3_a")
    lora.attach(ref, 4, 8.0, ("o_proj", "down_proj"), seed=1)
    ref.load_state_dict(sd)
    ref = ref.double().to(DEV).train()
    lp_err, loss32, loss_r, ratios, _ = family.fp32_against_hf64(m32.to(DEV).train(), seqs, att, mode, monkeypatch, ref64=ref)
    print(f"phi3_a LoRA/{mode}: logprob err {lp_err:.2e}, loss rel {abs(loss32 - loss_r) / abs(loss_r):.2e}, worst ratio {max(ratios.values()):.2e}")
    assert lp_err < 1e-4 and abs(loss32 - loss_r) <= 1e-5 * abs(loss_r)
    assert abs(loss32 - loss_plain) > 1e-5 * abs(loss32)                # B set: not the plain model any more
    control = family.fp32_against_hf64(fx.hf_model("phi3_a"), seqs, att, mode, monkeypatch)[3]      # the plain model, every weight trainable
    bad = {n: r for n, r in ratios.items() if r > max(1e-4, 1.5 * max(control.values()))}
    assert set(ratios) == adapters and not bad and max(ratios.values()) <= 1e-3, bad
