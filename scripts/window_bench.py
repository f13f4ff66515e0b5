#!/usr/bin/env python3
"""Sliding-window measurements on the tau2 trie (synth.tau2(0), 16 k tokens deep): HIP-event times of the three tree-attention kernels
(fwd, dQ, dK/dV incl. the slab finalize) at 16/8 heads (D = 128) and 14/2 heads (D = 64) for W = inf (the unwindowed kernels), 4096 and
1024; and TreeTrainingEngine.backward tokens/s at Qwen3-0.6B geometry (random init, bf16) with every layer sliding at W = 4096 against
none.  Prints one JSON line per measurement.
Usage: python scripts/window_bench.py [iters] [engine steps] [engine warmup]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import ops, packing, synth
from dynamictreeattn_amd.model import Qwen3TreeLM, make_config
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine, _PackedTrie

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 1
dev = torch.device("cuda:0")
seqs = synth.as_tensors(synth.tau2(0))


def attention(Hq, Hkv, D):
    trie = TokenTrie(seqs); trie.backward_permute()
    pk = _PackedTrie(trie, dev, Hkv)
    T = pk.plan.T
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v, do = (torch.randn(T, H, D, generator=g, device=dev).bfloat16() for H in (Hq, Hkv, Hkv, Hq))
    scale = D ** -0.5
    for W in (0, 4096, 1024):
        meta = pk.for_window(W) if W else pk.meta
        keys = int(sum(int(e - b) for b, e, _, _ in meta.runs.cpu().numpy()))          # key rows the query tiles visit
        out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, scale)
        ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            ops.attn_fwd_raw(q, k, v, meta, scale)
        b.record(); torch.cuda.synchronize()
        res = {"fwd": a.elapsed_time(b) / iters}
        tm = ops.KernelTimer(); ops.KernelTimer.active = tm
        try:
            for _ in range(iters):
                ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale)
        finally:
            ops.KernelTimer.active = None
        ms = tm.totals_ms()
        res["bwd_dq"] = ms["bwd_dq"][0] / ms["bwd_dq"][1]
        fin = ms.get("bwd_dkv_finalize", (0.0, 0))
        res["bwd_dkv"] = ms["bwd_dkv"][0] / ms["bwd_dkv"][1] + (fin[0] / fin[1] if fin[1] else 0.0)
        print(json.dumps({"metric": "window_attention_ms", "heads": f"{Hq}/{Hkv}", "head_dim": D, "T": T, "window": W or "inf",
                          "max_depth": packing.max_depth(pk.plan), "qtile_keys": keys,
                          **{n: round(t, 4) for n, t in res.items()}, "total": round(sum(res.values()), 4)}), flush=True)


def engine(W):
    cfg = dict(synth.QWEN3_0P6B)
    if W:
        cfg.update(layer_types=["sliding_attention"] * cfg["num_hidden_layers"], sliding_window=W)
    m = Qwen3TreeLM(make_config(cfg)).to(device=dev, dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight") or "layernorm" in name:
                p.fill_(1.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g, device=dev) * 0.02).bfloat16())
    m.train()
    loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()
    e = TreeTrainingEngine(m.config, dev, torch.bfloat16, max(map(len, seqs)))
    times = []
    for i in range(warmup + steps):
        m.zero_grad(set_to_none=True)
        trie = TokenTrie(seqs, [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]); trie.backward_permute()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss = e.backward(m, trie, loss_fn, 2048)
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    print(json.dumps({"metric": "engine_backward_tokens_per_s", "model": "Qwen3-0.6B geometry (random init), bf16",
                      "sliding_window": W or None, "mode": e.last_mode, "value": round(trie.n_tokens * len(times) / sum(times), 1),
                      "unit": "tokens/s", "s_per_step": [round(t, 4) for t in times], "loss": float(loss)}), flush=True)
    del m, e
    torch.cuda.empty_cache()


if __name__ == "__main__":
    attention(16, 8, 128)
    attention(14, 2, 64)
    for W in (0, 4096):
        engine(W)
