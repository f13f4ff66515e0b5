"""Cohere / Cohere2 through the engine on the GPU: UNMODIFIED transformers CohereForCausalLM / Cohere2ForCausalLM models
(tests/test_cohere_fixture.py: one LayerNorm per layer, the parallel attention || MLP block, interleaved RoPE over the whole head,
biases on q, k, v and o, sliding layers that rotate and full layers that do not, a scale on the final logits) in packed mode and the
block-wise stack walk - the protocol of tests/family.py with the numeric bounds of tests/test_gpu_engine_phi_glm.py.

* fp32 against HF's own eager attention in float64 on the card: logprobs within 1e-4, loss within 1e-5, every gradient within
  max(1e-4, 1.5 x control) and 1e-3, where the control is the same engine on Llama-shaped wiring of the same sizes
  (test_cohere_fixture.llama_control).
* bf16 against the fixture the reference computed (loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN, logprobs 0.08 / 0.015).
* tree equals dense on the device; per-layer recomputation with kept attention outputs gives the gradients of the plain pass bit
  for bit (a recomputed Cohere layer carries two pending updates).
* the tree forward honours the logit scale."""
import pytest
import torch

import family
import test_cohere_fixture as fx
from dynamictreeattn_amd import synth
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
    """The control's ratio for parameter `name`: its namesake's; for a bias its weight's (the Llama wiring has none)."""
    return control.get(name.replace(".bias", ".weight"), 0.0)


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
    assert abs(loss_c - loss) > 1e-5 * abs(loss)                      # this family's wiring changes the loss: not an inert case
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


def test_tree_forward_honours_the_logit_scale():
    """engine.forward on cohere_b (logit_scale 0.3, no power of two) in fp32: the fixture's logprobs; the same weights under
    logit_scale 1.0 give the fwd_dense_off_logit_scale record, MIN_GAP away."""
    pytest.importorskip("transformers")
    g = fx.gold("cohere_b")
    seqs = _seqs("cohere_b")
    for off, rec, other in ((None, "fwd_dense", "fwd_dense_off_logit_scale"), ("logit_scale", "fwd_dense_off_logit_scale", "fwd_dense")):
        hf = fx.hf_model("cohere_b", off).to(DEV)
        t = TokenTrie(seqs); t.forward_permute()
        out = [o.cpu() for o in TreeTrainingEngine(hf.config, DEV, torch.float32, max(map(len, seqs)), forward_only=True).forward(hf, t)]
        assert fx._dist(out, g[rec]) < 1e-4 and fx._dist(out, g[other]) >= fx.MIN_GAP
