"""OLMo-2 / OLMo-3 through the engine on the GPU: UNMODIFIED transformers Olmo2ForCausalLM / Olmo3ForCausalLM models
(tests/test_olmo_fixture.py: head_dim 64 with 4 / 2 heads, head_dim 128 with 2 / 1 heads, and OLMo-3 with alternating sliding layers
and YaRN on the full layers' own RoPE table; projection-wide q/k norms, post-norm layers, untied head) in packed mode and the
block-wise stack walk - the protocol and the numeric bounds of tests/test_gpu_engine_gemma.py.

* fp32 against HF's own eager attention in float64 on the card: logprobs within 1e-4, loss within 1e-5, every gradient within
  max(1e-4, 1.5 x control) and 1e-3, where the control is the same engine on Llama-shaped wiring of the same sizes
  (test_olmo_fixture.llama_control).
* bf16 against the fixture the reference computed (loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN, logprobs 0.08 / 0.015).
* the gradient name set is the model's named_parameters() with lm_head.weight (untied); tree equals dense on the device;
  per-layer recomputation with kept attention outputs gives the gradients of the plain pass bit for bit; LoRA adapters on
  q_proj / v_proj; for olmo3, the full layers forced onto the sliding layers' table miss the fp32 logprob bound."""
import pytest
import torch

import family
import test_olmo_fixture as fx
from dynamictreeattn_amd import lora, synth
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("packed", 2048), ("stack", 16)]


def _seqs(case):
    return synth.as_tensors(fx.seqs_of(case))


def _engine(model, seqs, dtype, mode, bs, monkeypatch, forward=True):
    return family.run_engine(model, seqs, family.att(len(seqs)), dtype, mode, bs, monkeypatch, forward=forward)


def _fp32_run(model32, case, mode, monkeypatch):
    """family.fp32_against_hf64 on the case's sequences: (logprob error, loss, reference loss, ratios)."""
    seqs = _seqs(case)
    lp_err, loss, loss_r, ratios, names = family.fp32_against_hf64(model32, seqs, family.att(len(seqs)), mode, monkeypatch)
    assert "lm_head.weight" in names[1]      # untied head
    return lp_err, loss, loss_r, ratios


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
    assert abs(loss_c - loss) > 1e-5 * abs(loss)                      # OLMo's wiring changes the loss: not an inert case
    assert lp_c < 1e-4 and abs(loss_c - loss_cr) <= 1e-5 * abs(loss_cr)
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
    named = family.check_bf16_against_fixture(hf, _seqs(case), g, mode, bs, monkeypatch, label=case)
    assert set(named) == set(fx.gold_grads(g)) and "lm_head.weight" in named


@pytest.mark.parametrize("case", list(fx.CASES))
def test_tree_equals_dense_on_the_device(case):
    """dense.backward (one pass per sequence, the stack form) against engine.backward (one packed pass) in fp32."""
    pytest.importorskip("transformers")
    family.check_tree_equals_dense(fx.hf_model(case).to(DEV), fx.hf_model(case).to(DEV), _seqs(case))


@pytest.mark.parametrize("case", list(fx.CASES))
def test_recomputation_with_kept_attention_outputs_changes_nothing(case, monkeypatch):
    """checkpoint_layers = True: every layer is recomputed in the backward (an OLMo layer hands on no pending update: the
    recomputation back-propagates through its one output); with kept attention outputs the recomputation replays them - loss and
    gradients are those of the plain packed pass, bit for bit."""
    pytest.importorskip("transformers")
    family.check_recompute_is_bitwise(fx.hf_model(case).to(device=DEV, dtype=torch.bfloat16).train(), _seqs(case), monkeypatch)


@pytest.mark.parametrize("mode,bs", MODES)
def test_lora_adapters_on_olmo(mode, bs, monkeypatch):
    pytest.importorskip("transformers")
    seqs = _seqs("olmo3")
    plain = fx.hf_model("olmo3").to(device=DEV, dtype=torch.bfloat16).train()
    _, loss_plain, _ = _engine(plain, seqs, torch.bfloat16, mode, bs, monkeypatch, forward=False)
    hf = fx.hf_model("olmo3")
    params = lora.attach(hf, 4, 8.0, ("q_proj", "v_proj"), seed=1)
    hf = hf.to(device=DEV, dtype=torch.bfloat16).train()
    lora.check_supported(hf)
    adapters = {n for n, p in hf.named_parameters() if p.requires_grad}
    assert len(adapters) == len(params) == 2 * 2 * hf.config.num_hidden_layers
    for n, p in hf.named_parameters():                                  # B = 0: the adapted model IS the plain one
        if n in adapters and "lora_B" in n:
            assert not bool(p.any())
    _, loss, e = _engine(hf, seqs, torch.bfloat16, mode, bs, monkeypatch, forward=False)
    assert e.last_mode.startswith(mode)
    assert loss == loss_plain
    got = {n for n, p in hf.named_parameters() if p.grad is not None}
    assert got == adapters and all(p.grad is None for n, p in hf.named_parameters() if n not in adapters)
    assert all(bool(torch.isfinite(p.grad).all()) for n, p in hf.named_parameters() if n in adapters)
    assert any(float(p.grad.float().abs().max()) > 0 for n, p in hf.named_parameters() if "lora_B" in n)       # B receives a real gradient


def test_olmo3_on_the_sliding_table_misses_the_fp32_bound(monkeypatch):
    """The per-layer table is not inert: the fp32 engine is within 1e-4 of the fixture's logprobs, and with the full layers forced
    onto the sliding layers' table it is not."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import model as M
    hf = fx.hf_model("olmo3").to(DEV)
    g = fx.gold("olmo3")
    seqs = _seqs("olmo3")
    maxlen = max(map(len, seqs))

    def forward():
        t = TokenTrie(seqs); t.forward_permute()
        out = TreeTrainingEngine(hf.config, DEV, torch.float32, maxlen, forward_only=True).forward(hf, t)
        return max(float((a.cpu() - b).abs().max()) for a, b in zip(out, g["fwd_dense"]))

    assert forward() < 1e-4
    real = M.rope_of
    monkeypatch.setattr(M, "rope_of", lambda c, layer_type=None: real(c, "sliding_attention" if layer_type else None))
    err = forward()
    print(f"olmo3 with every layer on the sliding table: logprob err {err:.3f}")
    assert not err < 1e-4
