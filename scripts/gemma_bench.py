#!/usr/bin/env python3
"""Gemma-2 measurements on the tau2 trie (synth.tau2(0)), bf16.

kernels : HIP-event times per launch of the three tree-attention kernels (fwd, dQ, dK/dV incl. the slab finalize), soft-capped
          (softcap 50, Gemma-2's attn_logit_softcapping) and uncapped, on the same packed call, at 16 / 8 heads x D = 128 (the headline's
          geometry) and 32 / 16 heads x D = 128 (Gemma-2-27B's); a capped full-attention call also through the windowed instantiation
          with an all-visible window (the A/B that decides whether the dedicated CAP-without-WIN instantiation is worth its build time).
engine  : TreeTrainingEngine.backward tokens/s, engine mode and peak HBM at Gemma-2-27B geometry (46 layers, hidden 4608, 32 / 16 heads,
          head_dim 128, intermediate 36 864, vocab 256 000) over an unmodified transformers Gemma2ForCausalLM, random init, with LoRA r = 16
          on all seven projections ("lora") and, if asked, full fine-tuning ("full").
Prints one JSON line per measurement.
Usage: python scripts/gemma_bench.py [kernels,lora,full] [iters] [engine steps] [engine warmup]"""
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import lora, ops, packing, synth
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine, _PackedTrie

what = (sys.argv[1] if len(sys.argv) > 1 else "kernels,lora").split(",")
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 1
dev = torch.device("cuda:0")
BF = torch.bfloat16
CAP = 50.0
GEMMA2_27B = dict(vocab_size=256000, hidden_size=4608, intermediate_size=36864, num_hidden_layers=46, num_attention_heads=32,
                  num_key_value_heads=16, head_dim=128, query_pre_attn_scalar=144, sliding_window=4096, rms_norm_eps=1e-6,
                  attn_logit_softcapping=50.0, final_logit_softcapping=30.0, max_position_embeddings=8192)


def timed(q, k, v, do, meta, scale, cap):
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, scale, cap)
    ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale, softcap=cap)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        ops.attn_fwd_raw(q, k, v, meta, scale, cap)
    b.record(); torch.cuda.synchronize()
    res = {"fwd": a.elapsed_time(b) / iters}
    tm = ops.KernelTimer(); ops.KernelTimer.active = tm
    try:
        for _ in range(iters):
            ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale, softcap=cap)
    finally:
        ops.KernelTimer.active = None
    ms = tm.totals_ms()
    res["bwd_dq"] = ms["bwd_dq"][0] / ms["bwd_dq"][1]
    fin = ms.get("bwd_dkv_finalize", (0.0, 0))
    res["bwd_dkv"] = ms["bwd_dkv"][0] / ms["bwd_dkv"][1] + (fin[0] / fin[1] if fin[1] else 0.0)
    return {n: round(t, 4) for n, t in res.items()}


def kernels(Hq, Hkv, D):
    seqs = synth.as_tensors(synth.tau2(0))
    trie = TokenTrie(seqs); trie.backward_permute()
    pk = _PackedTrie(trie, dev, Hkv)
    T = pk.plan.T
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v, do = (torch.randn(T, H, D, generator=g, device=dev).bfloat16() for H in (Hq, Hkv, Hkv, Hq))
    scale = D ** -0.5
    # the full plan with an all-visible window: the WIN = true kernels on the same tiles (win_lo = 0 for every row)
    allvis = dataclasses.replace(pk.meta, win_lo=torch.zeros(T, dtype=torch.int32, device=dev), window=packing.max_depth(pk.plan) + 1)
    rows = {"uncapped": timed(q, k, v, do, pk.meta, scale, 0.0), "capped": timed(q, k, v, do, pk.meta, scale, CAP),
            "uncapped_again": timed(q, k, v, do, pk.meta, scale, 0.0),
            "capped_via_window_instantiation": timed(q, k, v, do, allvis, scale, CAP)}
    ratio = {n: round(rows["capped"][n] / (0.5 * (rows["uncapped"][n] + rows["uncapped_again"][n])), 4) for n in rows["capped"]}
    print(json.dumps({"metric": "softcap_attention_ms", "heads": f"{Hq}/{Hkv}", "head_dim": D, "T": T, "softcap": CAP, **rows,
                      "capped_over_uncapped": ratio}), flush=True)


def engine(full: bool):
    import transformers
    cfg = transformers.Gemma2Config(**GEMMA2_27B)
    torch.manual_seed(0)
    torch.set_default_dtype(BF)
    try:
        with torch.device(dev):
            model = transformers.Gemma2ForCausalLM(cfg)
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.zero_() if n.endswith("norm.weight") else p.normal_(0.0, 0.02)          # Gemma norms multiply by 1 + w
    if not full:
        lora.attach(model, 16, 32.0, dtype=BF, seed=0)
        model.to(dev)
    model.train()
    seqs = synth.as_tensors(synth.tau2(0, V=cfg.vocab_size))
    att = lambda: [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]
    loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()
    e = TreeTrainingEngine(model.config, dev, BF, max(map(len, seqs)))
    torch.cuda.reset_peak_memory_stats()
    times = []
    for i in range(warmup + steps):
        model.zero_grad(set_to_none=True)
        trie = TokenTrie(seqs, att()); trie.backward_permute()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss = e.backward(model, trie, loss_fn, 2048)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    print(json.dumps({"metric": "engine_backward_tokens_per_s",
                      "model": "Gemma-2-27B geometry, unmodified Gemma2ForCausalLM (random init), bf16, " + ("full fine-tuning" if full else "LoRA r=16 on all seven projections"),
                      "mode": e.last_mode, "params_B": round(sum(p.numel() for p in model.parameters()) / 1e9, 2),
                      "trainable_M": round(sum(p.numel() for p in model.parameters() if p.requires_grad) / 1e6, 1),
                      "value": round(trie.n_tokens * len(times) / sum(times), 1), "unit": "tokens/s", "n_tokens": trie.n_tokens,
                      "s_per_step": [round(t, 4) for t in times], "loss": float(loss),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}), flush=True)
    model.zero_grad(set_to_none=True)
    del model, e
    torch.cuda.empty_cache()


if __name__ == "__main__":
    if "kernels" in what:
        kernels(16, 8, 128)
        kernels(32, 16, 128)
    if "lora" in what:
        engine(False)
    if "full" in what:
        engine(True)
