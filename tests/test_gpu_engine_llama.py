"""Llama-3 / Mistral / Mixtral through the engine on the GPU: UNMODIFIED transformers models (tests/test_llama_family_fixture.py:
llama3, llama3 with o_proj / MLP biases, yarn, Mistral with every layer sliding, Mixtral) in packed mode and the block-wise stack walk.

* fp32 against HF's own eager attention in float64 on the card (tests/family.py: fp32_against_hf64, the protocol every family
  shares; the fixtures' fp16-packed gradients cannot carry 1e-4): logprobs
  within 1e-4, loss within 1e-5, every gradient within max(1e-4, 1.5 x control) and 1e-3, where the control is the same engine on the
  same model with the feature off (default RoPE, no window, no biases; for Mixtral the dense-MLP model).
* bf16 against the fixtures the reference computed (loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN, logprobs 0.08 / 0.015).
* the gradient name set is the model's named_parameters(); tree equals dense on the device."""
import pytest
import torch

import family
import test_llama_family_fixture as fx
from dynamictreeattn_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("packed", 2048), ("stack", 16)]


def _seqs(case):
    return synth.as_tensors(fx.seqs_of(case))


def _control_model(case):
    """The model of `case` with the feature off, in fp32: default RoPE / no window / no biases; Mixtral: a MistralForCausalLM (dense MLP)."""
    import transformers
    if case == "mixtral":
        geo = {k: v for k, v in fx.MIXTRAL.items() if not k.startswith("num_local") and k != "num_experts_per_tok"}
        c = transformers.MistralConfig(**geo, max_position_embeddings=256, sliding_window=fx.WINDOW,
                                       rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
        c._attn_implementation = "eager"
        m = transformers.MistralForCausalLM(c)
        return family.load_weights(m, fx.weights(m, 25, fx.CASE_STD["mixtral"]))
    if case == "llama3_bias":
        m = transformers.LlamaForCausalLM(fx.hf_config("llama3"))              # the same rope, no bias parameters at all
        return family.load_weights(m, fx.weights(m, fx.CASES[case][5]))
    return fx.hf_model(case, off=True)


def _fp32_run(model32, case, mode, monkeypatch):
    """family.fp32_against_hf64 on the case's sequences: (logprob error, loss, reference loss, ratios); the engine's gradient names
    are the model's named_parameters() (lm_head, o_proj.bias, mlp biases, experts)."""
    seqs = _seqs(case)
    return family.fp32_against_hf64(model32, seqs, family.att(len(seqs)), mode, monkeypatch)[:4]


@pytest.mark.parametrize("mode", ["packed", "stack"])
@pytest.mark.parametrize("case", list(fx.CASES))
def test_fp32_against_hf_eager_in_float64(case, mode, monkeypatch):
    pytest.importorskip("transformers")
    lp_err, loss, loss_r, ratios = _fp32_run(fx.hf_model(case), case, mode, monkeypatch)
    print(f"{case}/{mode}: logprob err {lp_err:.2e}, loss rel {abs(loss - loss_r) / abs(loss_r):.2e}, worst ratio "
          f"{max(ratios.items(), key=lambda kv: kv[1])}")
    assert lp_err < 1e-4
    assert abs(loss - loss_r) <= 1e-5 * abs(loss_r)
    _, _, loss_c, control = _fp32_run(_control_model(case), case, mode, monkeypatch)
    assert abs(loss_c - loss_r) > 1e-5 * abs(loss_r)                  # the feature changes the loss: a pass is not an inert case
    bad = {n: (r, control.get(n)) for n, r in ratios.items() if r > max(1e-4, 1.5 * control.get(n, 0.0))}
    print(f"{case}/{mode}: control worst {max(control.values()):.2e}; above the rule: {bad}")
    assert not bad, bad
    assert max(ratios.values()) <= 1e-3


@pytest.mark.parametrize("mode,bs", MODES)
@pytest.mark.parametrize("case", list(fx.CASES))
def test_bf16_against_the_reference_fixture(case, mode, bs, monkeypatch):
    pytest.importorskip("transformers")
    hf = fx.hf_model(case).to(device=DEV, dtype=torch.bfloat16).train()
    family.check_bf16_against_fixture(hf, _seqs(case), fx.gold(case), mode, bs, monkeypatch, label=case)


def test_tree_equals_dense_on_the_device_llama3():
    """dense.backward (one pass per sequence, the stack form) against engine.backward (one packed pass) on the llama3 case in fp32."""
    pytest.importorskip("transformers")
    family.check_tree_equals_dense(fx.hf_model("llama3").to(DEV), fx.hf_model("llama3").to(DEV), _seqs("llama3"), forward=False)
