"""Qwen3-MoE through the engine on the GPU.  An UNMODIFIED transformers.Qwen3MoeForCausalLM with the fixture's weights
(tests/test_qwen3_moe_fixture.py: one dense layer, two layers of 8 experts, top 2) runs in every mode against the reference's dense
per-sequence run (tests/golden/engine_qwen3_moe.pt): in fp32 elementwise, with every token routed as the fixture routed it; in bf16 within
the norm-relative bounds of the bf16 engine tests.  Qwen3TreeLM with the MoE configuration has HF's parameter names and gradients, two
identical calls give identical bits, and one fp32 forward at Qwen3-30B-A3B width is compared with HF's own model on the card."""
import numpy as np
import pytest
import torch

import family
import test_qwen3_moe_fixture as fx
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo
from test_gpu_engine import REF_BF16_BOUND, REF_BF16_MEDIAN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _seqs():
    return synth.as_tensors(synth.make_case(fx.QWEN3_MOE_DATA))


class _RecordRouting:
    """Records the top-k ids of every router call (ops.moe_router_fwd_raw) in call order."""

    def __init__(self, monkeypatch):
        self.calls = []
        real = ops.moe_router_fwd_raw

        def rec(logits, k, norm):
            out = real(logits, k, norm)
            self.calls.append(out[0].detach().clone())
            return out
        monkeypatch.setattr(ops, "moe_router_fwd_raw", rec)


def _check_routing(engine, trie, calls, g):
    """The packed rows of every sequence were routed as the fixture's dense per-sequence run routed that sequence's tokens."""
    packed = engine.last_packed
    assert len(calls) == len(fx.MOE_LAYERS)
    ids = [c.cpu().long() for c in calls]
    n = 0
    for i, attach_list in enumerate(trie.attach_lists):
        path = torch.as_tensor(packed._paths_host[i])
        for attachment, length in attach_list:
            sid = attachment["_sequence_batch_id"]
            for li in range(len(fx.MOE_LAYERS)):
                assert torch.equal(ids[li][path[:length]], g["topk_ids"][sid][li].long()), (sid, li)
            n += 1
    assert n == len(g["topk_ids"])


def _hf(dtype):
    pytest.importorskip("transformers")
    return fx.hf_qwen3_moe().to(device=DEV, dtype=dtype).train()


def _fp32_grads_match(named, gold_grads):
    for n, ref in gold_grads.items():
        got = named[n].grad
        assert got is not None, n
        err = float((got.float().cpu() - ref).abs().max())
        assert err <= 2e-3 * float(ref.abs().max()) + 1e-7, (n, err, float(ref.abs().max()))


@pytest.mark.parametrize("mode,bs,recompute,full", [("packed", 2048, None, 0), ("packed", 2048, 0.0, 0), ("packed", 2048, 1.0, 0),
                                                    ("packed", 2048, 1.0, 1), ("stack", 2048, None, 0), ("stack", 24, None, 0)])
def test_fp32_moe_engine_vs_reference(mode, bs, recompute, full, monkeypatch):
    """fp32: loss, forward logprobs and every parameter gradient (router and experts included) elementwise against the fixture; routing
    equal to the fixture's.  recompute: per-layer recomputation keeping that fraction of attention outputs, with `full` leading layers
    kept whole.  stack 24: blocks that split the trie at forks."""
    hf = _hf(F32)
    g = fx.gold()
    seqs = _seqs()
    maxlen = max(map(len, seqs))
    t = TokenTrie(seqs); t.forward_permute()
    rec = _RecordRouting(monkeypatch)
    e0 = TreeTrainingEngine(hf.config, DEV, F32, maxlen, forward_only=True)
    out = e0.forward(hf, t)
    for a, b in zip(out, g["fwd_dense"]):
        assert a.dtype == F32 and a.shape == b.shape
        assert float((a.cpu() - b).abs().max()) <= 2e-4 * (1 + float(b.abs().max()))
    _check_routing(e0, t, rec.calls, g)
    _, loss, e = family.run_engine(hf, seqs, family.att(len(seqs)), F32, mode, bs, monkeypatch, forward=False, recompute=recompute, full_layers=full)
    assert e.last_mode.startswith(mode + ("+recompute" if recompute is not None else "")), e.last_mode
    if mode == "stack" and bs < maxlen:
        assert int(e.last_mode.split("x")[-1]) > 1, e.last_mode
    assert abs(loss - g["bwd_dense_loss"]) <= 1e-5 * abs(loss)
    _fp32_grads_match(dict(hf.named_parameters()), fx.gold_grads(g))


@pytest.mark.parametrize("mode,bs", [("packed", 2048), ("stack", 24)])
def test_bf16_moe_engine_vs_reference(mode, bs, monkeypatch):
    """bf16: the norm-relative gradient bounds of the bf16 engine tests; forward logprobs close to the fp32 reference."""
    hf = _hf(torch.bfloat16)
    g = fx.gold()
    gold_grads = fx.gold_grads(g)
    seqs = _seqs()
    out, loss, _ = family.run_engine(hf, seqs, family.att(len(seqs)), torch.bfloat16, mode, bs, monkeypatch)
    for a, b in zip(out, g["fwd_dense"]):
        assert (a - b).abs().max() < 0.08 and (a - b).abs().mean() < 0.015
    assert abs(loss - g["bwd_dense_loss"]) < 1e-2 * abs(loss)
    named = dict(hf.named_parameters())
    ratios = {n: mo.grad_ratio(gold_grads[n], named[n].grad.float().cpu()) for n in gold_grads}
    assert max(ratios.values()) <= REF_BF16_BOUND, max(ratios.items(), key=lambda kv: kv[1])
    assert float(np.median(list(ratios.values()))) <= REF_BF16_MEDIAN


def test_qwen3_tree_lm_moe_names_and_gradients_equal_hf():
    hf = _hf(F32)
    mine = Qwen3TreeLM.from_named(fx.QWEN3_MOE, {n: p.detach().cpu() for n, p in hf.named_parameters()}, DEV, F32)
    assert sorted(n for n, _ in mine.named_parameters()) == sorted(n for n, _ in hf.named_parameters())
    seqs = _seqs()
    grads = []
    for m in (hf, mine):
        t = TokenTrie(seqs, fx.att(len(seqs))); t.backward_permute()
        TreeTrainingEngine(m.config, DEV, F32, max(map(len, seqs))).backward(m, t, mo.default_loss, 2048)
        grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
    for n in grads[0]:
        assert torch.equal(grads[0][n], grads[1][n]), n


def test_moe_gradients_bitwise_repeatable():
    hf = _hf(torch.bfloat16)
    seqs = _seqs()
    runs = []
    for _ in range(2):
        hf.zero_grad(set_to_none=True)
        t = TokenTrie(seqs, fx.att(len(seqs))); t.backward_permute()
        loss = TreeTrainingEngine(hf.config, DEV, torch.bfloat16, max(map(len, seqs))).backward(hf, t, mo.default_loss, 2048)
        runs.append((loss, {n: p.grad.detach().clone() for n, p in hf.named_parameters()}))
    assert runs[0][0] == runs[1][0]
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_fp32_qwen3_30b_a3b_width_vs_hf_on_the_card(monkeypatch):
    """Four layers at Qwen3-30B-A3B width (H 2048, I 768, E 128, k 8, 32/4 heads) over a small tau2-shaped trie: the engine's fp32
    logprobs against HF's own Qwen3MoeForCausalLM run per sequence on the card.  A flipped expert changes every later token of its path.
    So each sequence's routing (the engine's packed rows vs HF's router, every layer) must agree up to its first token that has an HF
    routing margin below 1e-4 in some layer; logprobs are compared elementwise on the positions before the first token whose routing
    differs at all (a flip is allowed only at such a near-tie); the number of positions and sequences left out is reported."""
    pytest.importorskip("transformers")
    import transformers
    cfg = dict(synth.QWEN3_30B_A3B, num_hidden_layers=4, vocab_size=4096)
    with torch.device(DEV):
        hf = transformers.Qwen3MoeForCausalLM(fx.hf_config(cfg))
    w = fx.moe_weights(hf, seed=17, router_std=0.045, device=DEV)       # router logits of std ~2
    with torch.no_grad():
        for n, p in hf.named_parameters():
            p.copy_(w[n])
    del w
    hf = hf.float().eval()
    seqs = synth.as_tensors(synth.tau2(seed=3, V=4096, G=3, sys_len=160, turns=2, lo=40, hi=120, cap=512))
    k = cfg["num_experts_per_tok"]
    hf_ids, low, lp_hf = [], [], []
    with torch.no_grad():
        for s in seqs:
            rec = []
            hooks = [l.mlp.gate.register_forward_hook(lambda m_, i_, o_: rec.append(o_[0].float())) for l in hf.model.layers]
            logits = hf(input_ids=s.to(DEV)[None], use_cache=False).logits[0, :-1].float()
            for h_ in hooks:
                h_.remove()
            probs = [torch.softmax(r, -1) for r in rec]
            srt = [p.sort(-1, descending=True).values for p in probs]
            hf_ids.append(torch.stack([p.topk(k, -1).indices.sort(-1).values for p in probs]).cpu())      # [layers, len, k] as sets
            low.append(torch.stack([(x[:, k - 1] - x[:, k]) < 1e-4 for x in srt]).any(0).cpu())
            lp_hf.append(torch.log_softmax(logits, -1).gather(-1, s.to(DEV)[1:, None])[:, 0].cpu())
    rec = _RecordRouting(monkeypatch)
    t = TokenTrie(seqs); t.forward_permute()
    e = TreeTrainingEngine(hf.config, DEV, F32, max(map(len, seqs)), forward_only=True)
    out = e.forward(hf, t)
    ids = [c.cpu().long().sort(-1).values for c in rec.calls]
    assert len(ids) == cfg["num_hidden_layers"]
    n_cmp = n_all = whole = 0
    for i, attach_list in enumerate(t.attach_lists):
        path = torch.as_tensor(e.last_packed._paths_host[i])
        for attachment, length in attach_list:
            sid = attachment["_sequence_batch_id"]
            mine = torch.stack([x[path[:length]] for x in ids])                         # [layers, len, k]
            differs = (mine != hf_ids[sid]).any(-1).any(0)
            first_diff = int(differs.nonzero()[0, 0]) if bool(differs.any()) else length
            first_low = int(low[sid].nonzero()[0, 0]) if bool(low[sid].any()) else length
            assert first_diff >= first_low, (sid, first_diff, first_low)                 # no flip before a near-tie
            f = min(first_diff, length - 1)                     # logprob i predicts token i + 1 from tokens 0..i
            if f > 0:
                assert float((out[sid][:f].cpu() - lp_hf[sid][:f]).abs().max()) <= 2e-3, sid
            n_cmp += f; n_all += length - 1; whole += first_diff >= length
    print(f"30B-A3B width: compared {n_cmp} of {n_all} logprobs; {whole} of {len(seqs)} sequences routed exactly as HF throughout, "
          f"{n_all - n_cmp} positions left out after a routing flip at a margin < 1e-4")
    assert n_cmp >= n_all // 4
