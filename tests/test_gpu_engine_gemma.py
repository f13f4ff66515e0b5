"""Gemma-2 through the engine on the GPU: UNMODIFIED transformers Gemma2ForCausalLM models (tests/test_gemma2_fixture.py: head_dim 64
with 4 / 2 heads and head_dim 128 with 2 / 1 heads; soft-capped attention and final logits, alternating sliding layers, GeGLU, the four
`1 + w` sandwich norms, scaled embedding, tied head) in packed mode and the block-wise stack walk - the protocol of
tests/family.py.

* fp32 against HF's own eager attention in float64 on the card: logprobs within 1e-4, loss within 1e-5, every gradient within
  max(1e-4, 1.5 x control) and 1e-3, where the control is the same engine on the same weights with both caps None and the window wider
  than every sequence (the uncapped kernels); the control's loss must differ from the capped loss by more than 1e-5 relative.
* bf16 against the fixture the reference computed (loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN, logprobs 0.08 / 0.015).
* the gradient name set is the model's named_parameters() (tied head: no lm_head); tree equals dense on the device;
  per-layer recomputation with kept attention outputs (the AttentionTape carrying the cap) gives the gradients of the plain pass;
  LoRA adapters on q_proj / v_proj; the dta_mi355x transformers attention backend honours `softcap` and `scaling`."""
import pytest
import torch

import family
import test_gemma2_fixture as fx
from dynamictreeattn_amd import lora, synth

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
    assert "lm_head.weight" not in names[1]      # tied head
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
    lp_c, loss_c, loss_cr, control = _fp32_run(fx.hf_model(case, "control"), case, mode, monkeypatch)
    assert abs(loss_c - loss) > 1e-5 * abs(loss)                      # the caps and the window change the loss: not an inert case
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
    assert set(named) == set(fx.gold_grads(g))


@pytest.mark.parametrize("case", list(fx.CASES))
def test_tree_equals_dense_on_the_device(case):
    """dense.backward (one pass per sequence, the stack form) against engine.backward (one packed pass) in fp32."""
    pytest.importorskip("transformers")
    family.check_tree_equals_dense(fx.hf_model(case).to(DEV), fx.hf_model(case).to(DEV), _seqs(case))


@pytest.mark.parametrize("case", list(fx.CASES))
def test_recomputation_with_kept_attention_outputs_changes_nothing(case, monkeypatch):
    """checkpoint_layers = True: every layer is recomputed in the backward; with kept attention outputs the recomputation replays them
    (the forward attention kernel runs once per layer) and the CAPPED backward runs on the replayed output - loss and gradients are
    those of the plain packed pass, bit for bit, as for Qwen3 in test_gpu_engine.test_partial_recomputation_changes_nothing."""
    pytest.importorskip("transformers")
    family.check_recompute_is_bitwise(fx.hf_model(case).to(device=DEV, dtype=torch.bfloat16).train(), _seqs(case), monkeypatch)


@pytest.mark.parametrize("mode,bs", MODES)
def test_lora_adapters_on_gemma2(mode, bs, monkeypatch):
    pytest.importorskip("transformers")
    seqs = _seqs("gemma2")
    plain = fx.hf_model("gemma2").to(device=DEV, dtype=torch.bfloat16).train()
    _, loss_plain, _ = _engine(plain, seqs, torch.bfloat16, mode, bs, monkeypatch, forward=False)
    hf = fx.hf_model("gemma2")
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


@pytest.mark.parametrize("case", list(fx.CASES))
def test_hf_backend_honours_softcap_and_scaling(case):
    """attn_implementation="dta_mi355x" on the tiny Gemma-2 model against HF eager (fp32): Gemma-2's attention passes `softcap` and
    `scaling` (query_pre_attn_scalar ** -0.5, not head_dim ** -0.5) and a sliding window on alternating layers."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import hf_attention
    name = hf_attention.register()
    eager = fx.hf_model(case).to(DEV)
    mine = fx.hf_model(case, attn=name).to(DEV)
    s = max(_seqs(case), key=len).to(DEV)[None]
    assert s.shape[1] > 3 * fx.WINDOW
    a, b = eager(input_ids=s, use_cache=False).logits, mine(input_ids=s, use_cache=False).logits
    assert float((a - b).abs().max()) < 1e-4
    off = fx.hf_model(case, "attn_cap").to(DEV)(input_ids=s, use_cache=False).logits              # dropping the cap is far outside that
    assert float((a - off).abs().max()) > 1e-2
    a.float().pow(2).mean().backward(); b.float().pow(2).mean().backward()
    q_eager = eager.model.layers[2].self_attn.q_proj.weight.grad
    q_mine = mine.model.layers[2].self_attn.q_proj.weight.grad
    assert float((q_eager - q_mine).norm() / q_eager.norm()) < 1e-4
