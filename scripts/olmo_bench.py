#!/usr/bin/env python3
"""OLMo-2 / OLMo-3 measurements on the tau2 trie (synth.tau2(0)), bf16.

kernels : alternating A/B, in one process and at the call's own row count, of the fused projection-wide q/k norm + RoPE kernel
          (dta_wide_qk_norm_rope_fwd / _bwd, q read in place from the fused [T, 3 NH, D] projection output and its gradient written
          into the fused gradient buffer) against the composed path the existing kernels allow: a contiguous copy of q,
          dta_rmsnorm_fwd over [T, NH D], the RoPE-only dta_qk_norm_rope_fwd - and backwards the RoPE-only backward,
          dta_rmsnorm_bwd and the copy into the fused gradient buffer.  Three pairs per direction, HIP-event time per call; the
          HBM bytes of each path are computed from the shapes (one read of every input, one write of every output, per launch),
          and the fused kernel's bytes/s is given as a share of 8 TB/s.
engine  : TreeTrainingEngine.backward tokens/s, engine mode and peak HBM over unmodified transformers classes, random init, full
          fine-tuning: "olmo2_1b" (Olmo2ForCausalLM: hidden 2048, 16 / 16 heads, head_dim 128, intermediate 8192, 16 layers, vocab
          100 352) and "olmo3_7b" (Olmo3ForCausalLM: hidden 4096, 32 / 32 heads, intermediate 11 008, 32 layers, 3 sliding : 1 full at
          W = 4096, YaRN on the full layers; vocab 100 352 - the released checkpoints' 100 278 is no multiple of 8, which the
          LM-head kernels need of a logits row: such a model is run with its embedding padded).
Prints one JSON line per measurement.
Usage: python scripts/olmo_bench.py [kernels,olmo2_1b,olmo3_7b] [iters] [engine steps] [engine warmup]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd._lib import lib, ptr
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

what = (sys.argv[1] if len(sys.argv) > 1 else "kernels,olmo2_1b").split(",")
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
warmup = int(sys.argv[4]) if len(sys.argv) > 4 else 1
dev = torch.device("cuda:0")
BF = torch.bfloat16
PEAK = 8e12                                   # bytes/s
EPS = 1e-6
OLMO2_1B = dict(vocab_size=100352, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=16,
                num_key_value_heads=16, rms_norm_eps=1e-6, max_position_embeddings=4096, tie_word_embeddings=False, pad_token_id=None,
                eos_token_id=None, rope_parameters={"rope_type": "default", "rope_theta": 500000.0})
_TYPES = (["sliding_attention"] * 3 + ["full_attention"]) * 8
OLMO3_7B = dict(vocab_size=100352, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                num_key_value_heads=32, rms_norm_eps=1e-6, max_position_embeddings=65536, tie_word_embeddings=False, pad_token_id=None,
                eos_token_id=None, sliding_window=4096, layer_types=_TYPES,
                rope_parameters={"sliding_attention": {"rope_type": "default", "rope_theta": 500000.0},
                                 "full_attention": {"rope_type": "yarn", "rope_theta": 500000.0, "factor": 8.0,
                                                    "original_max_position_embeddings": 8192, "attention_factor": 1.2079441541679836,
                                                    "beta_fast": 32, "beta_slow": 1}})


def _time(fn):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernels(NH, D):
    seqs = synth.as_tensors(synth.tau2(0))
    trie = TokenTrie(seqs); trie.backward_permute()
    T, n, es, dt = trie.n_tokens, NH * D, 2, ops._DT[BF]
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(T, 3 * NH, D, generator=g, device=dev).to(BF)           # the fused projection output; q is its first NH heads
    dqkv = torch.randn(T, 3 * NH, D, generator=g, device=dev).to(BF)          # the fused gradient buffer (dq arrives in its first NH heads)
    x, dbuf = qkv[:, :NH], dqkv[:, :NH]
    dy = torch.randn(T, NH, D, generator=g, device=dev).to(BF)
    w = (1 + 0.1 * torch.randn(n, generator=g, device=dev)).to(BF)
    cs = ops.rope_cos_sin(torch.randint(0, 16384, (T,), generator=g, device=dev), D, 5e5)
    y, rstd = torch.empty(T, NH, D, dtype=BF, device=dev), torch.empty(T, dtype=torch.float32, device=dev)
    part = torch.empty(lib().dta_wide_qk_norm_rope_bwd_blocks(T), n, dtype=torch.float32, device=dev)
    xc, t, da, dxc = (torch.empty(T, n, dtype=BF, device=dev) for _ in range(4))
    part_c = torch.empty(lib().dta_rmsnorm_bwd_blocks(T), n, dtype=torch.float32, device=dev)

    def fused_fwd():
        ops._launch("dta_wide_qk_norm_rope_fwd", (x, w, cs), ptr(x), ptr(w), ptr(cs), ptr(y), ptr(rstd), T, NH, D, x.stride(0), EPS, dt)

    def composed_fwd():
        xc.view(T, NH, D).copy_(x)
        ops._launch("dta_rmsnorm_fwd", (xc, w), ptr(xc), None, ptr(w), None, ptr(t), ptr(rstd), T, n, EPS, 0.0, dt)
        ops._launch("dta_qk_norm_rope_fwd", (t, cs), ptr(t), None, ptr(cs), ptr(y), None, T, NH, D, n, EPS, dt)

    def fused_bwd():
        ops._launch("dta_wide_qk_norm_rope_bwd", (x, w, cs, dy), ptr(x), ptr(w), ptr(cs), ptr(dy), ptr(rstd), ptr(dbuf), ptr(part), T, NH, D,
                    x.stride(0), n, D, dbuf.stride(0), dt)
        ops.sum_slabs(part, BF)

    def composed_bwd():                    # xc: the contiguous copy the composed forward kept
        ops._launch("dta_qk_norm_rope_bwd", (dy, cs), None, None, ptr(cs), ptr(dy), None, ptr(da), None, T, NH, D, n, n, D, n, dt)
        ops._launch("dta_rmsnorm_bwd", (xc, w, da), ptr(xc), ptr(w), ptr(da), None, ptr(rstd), ptr(dxc), ptr(part_c), T, n, 0.0, dt)
        ops.sum_slabs(part_c, BF)
        dbuf.copy_(dxc.view(T, NH, D))

    row, table = T * n * es, T * D * 4
    nbytes = {"fused_fwd": 2 * row + table, "composed_fwd": 6 * row + table,              # copy 2, norm 2, rope 2
              "fused_bwd": 3 * row + table + part.numel() * 4, "composed_bwd": 7 * row + table + part_c.numel() * 4}   # rope 2, norm 3, copy 2
    composed_fwd(); fused_fwd()
    pairs = []
    for _ in range(3):
        pairs.append({"fused_fwd": _time(fused_fwd), "composed_fwd": _time(composed_fwd), "fused_bwd": _time(fused_bwd),
                      "composed_bwd": _time(composed_bwd)})
    best = {k: min(p[k] for p in pairs) for k in pairs[0]}
    print(json.dumps({"metric": "wide_qk_norm_rope_ms", "heads": NH, "head_dim": D, "T": T, "iters": iters,
                      "pairs_ms": [{k: round(v, 4) for k, v in p.items()} for p in pairs], "bytes": nbytes,
                      "fused_over_composed": {d: round(best["fused_" + d] / best["composed_" + d], 3) for d in ("fwd", "bwd")},
                      "fused_TB_per_s": {d: round(nbytes["fused_" + d] / best["fused_" + d] / 1e9, 2) for d in ("fwd", "bwd")},
                      "fused_share_of_8TBps": {d: round(nbytes["fused_" + d] / (best["fused_" + d] * 1e-3) / PEAK, 3) for d in ("fwd", "bwd")}}),
          flush=True)


def engine(name):
    import transformers
    cls, geo, label = {"olmo2_1b": ("Olmo2", OLMO2_1B, "OLMo-2-1B geometry, unmodified Olmo2ForCausalLM"),
                       "olmo3_7b": ("Olmo3", OLMO3_7B, "OLMo-3-7B geometry, unmodified Olmo3ForCausalLM")}[name]
    cfg = getattr(transformers, cls + "Config")(**geo)
    torch.manual_seed(0)
    torch.set_default_dtype(BF)
    try:
        with torch.device(dev):
            model = getattr(transformers, cls + "ForCausalLM")(cfg)
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.fill_(1.0) if n.endswith("norm.weight") else p.normal_(0.0, 0.02)
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
    print(json.dumps({"metric": "engine_backward_tokens_per_s", "model": label + " (random init), bf16, full fine-tuning",
                      "mode": e.last_mode, "params_B": round(sum(p.numel() for p in model.parameters()) / 1e9, 2),
                      "value": round(trie.n_tokens * len(times) / sum(times), 1), "unit": "tokens/s", "n_tokens": trie.n_tokens,
                      "s_per_step": [round(t, 4) for t in times], "loss": float(loss),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}), flush=True)
    model.zero_grad(set_to_none=True)
    del model, e
    torch.cuda.empty_cache()


if __name__ == "__main__":
    if "kernels" in what:
        kernels(16, 128)           # OLMo-2-1B: the q (and k) row of 2048
        kernels(32, 128)           # OLMo-3-7B / OLMo-2-7B: 4096
        kernels(40, 128)           # OLMo-2-13B / 32B: 5120
    for name in ("olmo2_1b", "olmo3_7b"):
        if name in what:
            engine(name)
