"""Sliding-window layers through the engine on the GPU.  An UNMODIFIED transformers.Qwen2ForCausalLM with one full and two sliding
layers (window 24, tests/test_qwen2_swa_fixture.py) runs in packed mode, packed mode with per-layer recomputation (with and without
the kept attention outputs) and the block-wise stack walk with blocks below and above the window, against the reference's dense
per-sequence run (tests/golden/engine_qwen2_swa.pt) with the tolerances of tests/test_gpu_engine_d64.py.  A Qwen3ForCausalLM whose
config names the sliding layers in layer_types runs in fp32 against HF's own eager attention on the card, and the dta_mi355x
attention backend against HF eager on the same sliding configuration."""
import numpy as np
import pytest
import torch

import family
import test_qwen2_swa_fixture as fx
from dynamictreeattn_amd import ops, synth
from oracle import model_oracle as mo
from test_gpu_engine import REF_BF16_BOUND, REF_BF16_MEDIAN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _seqs():
    return synth.as_tensors(synth.make_case(fx.QWEN2_SWA_DATA))


@pytest.mark.parametrize("mode,bs,recompute", [("packed", 2048, None), ("packed", 2048, 0.0), ("packed", 2048, 1.0),
                                               ("stack", 16, None), ("stack", 2048, None)])
def test_unmodified_qwen2_sliding_window_through_the_engine(mode, bs, recompute, monkeypatch):
    """recompute: None = the plain packed pass; otherwise every layer is recomputed in the backward, keeping that fraction of the
    attention outputs (0: the forward attention runs again; 1: AttentionTape replays it)."""
    pytest.importorskip("transformers")
    hf = fx.hf_qwen2_swa().to(device=DEV, dtype=torch.bfloat16).train()
    assert [getattr(l.self_attn, "sliding_window", None) for l in hf.model.layers] == [None, fx.WINDOW, fx.WINDOW]
    g = fx.gold()
    gold_grads = fx.gold_grads(g)
    seqs = _seqs()
    out, loss, e = family.run_engine(hf, seqs, family.att(len(seqs)), torch.bfloat16, mode, bs, monkeypatch, recompute=recompute)
    for a, b in zip(out, g["fwd_dense"]):
        assert a.dtype == torch.float32 and a.shape == b.shape
        assert (a - b).abs().max() < 0.08 and (a - b).abs().mean() < 0.015
    assert e.last_mode.startswith(mode + ("+recompute" if recompute is not None else "")), e.last_mode
    assert abs(loss - g["bwd_dense_loss"]) < 1e-2 * abs(loss)
    named = dict(hf.named_parameters())
    ratios = {n: mo.grad_ratio(gold_grads[n], named[n].grad.float().cpu()) for n in gold_grads}
    assert max(ratios.values()) <= REF_BF16_BOUND, max(ratios.items(), key=lambda kv: kv[1])
    assert float(np.median(list(ratios.values()))) <= REF_BF16_MEDIAN


def _qwen3_ratios(cfg, mode, monkeypatch):
    """family.fp32_against_hf64 on Qwen3ForCausalLM(cfg) at its seeded initialisation: logprob error, loss, reference loss, grad ratios."""
    import transformers as tr
    torch.manual_seed(3)
    seqs = _seqs()
    return family.fp32_against_hf64(tr.Qwen3ForCausalLM(cfg).float().train(), seqs, family.att(len(seqs)), mode, monkeypatch)[:4]


@pytest.mark.parametrize("mode", ["packed", "stack"])
def test_qwen3_layer_types_fp32_against_hf_eager(mode, monkeypatch):
    """Qwen3ForCausalLM (q/k head norms) with layer_types = [full, sliding, sliding]: the engine in fp32 (fp32 attention kernels) against
    HF's eager attention in float64 on the card - logprobs, loss and every gradient.  Every gradient is within 1e-4 of the float64
    one except the final norm's (a small gradient summed over every row and the whole vocabulary: 2.5e-4 for the unwindowed engine on
    the same model, measured on the MI355X); so each parameter is bounded by max(1e-4, 1.5 x the same engine's ratio with every
    layer full) - the window adds no error of its own."""
    pytest.importorskip("transformers")
    cfg = fx.hf_config("Qwen3Config")
    assert cfg.layer_types == ["full_attention", "sliding_attention", "sliding_attention"]
    lp_err, loss, loss_r, ratios = _qwen3_ratios(cfg, mode, monkeypatch)
    assert lp_err < 1e-4
    assert abs(loss - loss_r) <= 1e-5 * abs(loss_r)
    full_cfg = fx.hf_config("Qwen3Config")
    full_cfg.layer_types = ["full_attention"] * len(cfg.layer_types)
    _, _, loss_f, control = _qwen3_ratios(full_cfg, mode, monkeypatch)
    assert abs(loss_f - loss_r) > 1e-5 * abs(loss_r)                  # the window changes the loss (the engines agree to ~1e-7)
    bad = {n: (r, control[n]) for n, r in ratios.items() if r > max(1e-4, 1.5 * control[n])}
    assert not bad, bad
    assert max(ratios.values()) <= 1e-3


def test_hf_backend_sliding_window_against_eager():
    """attn_implementation="dta_mi355x" on the sliding Qwen2 configuration against HF eager: logits and input-side gradients of one
    sequence longer than several windows (fp32)."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import hf_attention
    name = hf_attention.register()
    eager = fx.hf_qwen2_swa("eager").to(DEV)
    mine = fx.hf_qwen2_swa(name).to(DEV)
    s = max(_seqs(), key=len).to(DEV)[None]
    assert s.shape[1] > 3 * fx.WINDOW
    a, b = eager(input_ids=s, use_cache=False).logits, mine(input_ids=s, use_cache=False).logits
    assert float((a - b).abs().max()) < 1e-4
    a.float().pow(2).mean().backward(); b.float().pow(2).mean().backward()
    q_eager = eager.model.layers[2].self_attn.q_proj.weight.grad
    q_mine = mine.model.layers[2].self_attn.q_proj.weight.grad
    assert float((q_eager - q_mine).norm() / q_eager.norm()) < 1e-4
    with pytest.raises(ValueError):
        hf_attention.dta_attention_forward(None, torch.zeros(2, 1, 1, 64, device=DEV), torch.zeros(2, 1, 1, 64, device=DEV),
                                           torch.zeros(2, 1, 1, 64, device=DEV), sliding_window=8)
    assert ops.stack_meta(3, fx.WINDOW).window == fx.WINDOW
