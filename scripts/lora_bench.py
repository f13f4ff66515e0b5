#!/usr/bin/env python3
"""TreeTrainingEngine.backward on the tau2 call of BASELINE config 2 (synth.tau2(0), block_size 2048), full fine-tuning beside LoRA, one
process, sync to sync after warm-up; random-init bf16 Qwen3TreeLM of the named geometry.  Rows:

    Qwen3-0.6B, Qwen3-8B:   full fine-tuning (no adapters: the path before adapters existed; run twice, first and last, for the run-to-run
                            spread) | LoRA r = 16 on all seven targets, fp32 adapters | the same with bf16 adapters
    Qwen3-30B-A3B:          attention-only adapters r = 16 (experts and router frozen)
    Qwen3-32B geometry:     64 layers, hidden 5120, 64 / 8 heads, intermediate 25 600 - the reach row: LoRA r = 16, fp32 adapters

Every row: tokens/s, s per step, last_mode, peak HBM, trainable parameters - or that it did not fit.  B is drawn non-zero (with the
zero init every product with B would be against zeros, which the clocks of this card reward: scripts/dvfs_zero_vs_random.py).
Usage: python scripts/lora_bench.py [out.json] [steps] [warmup] [row ...]"""
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import lora, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lora_bench.json")
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
only = sys.argv[4:]
dev = torch.device("cuda:0")
BF = torch.bfloat16
QWEN3_32B = dict(vocab_size=151936, hidden_size=5120, intermediate_size=25600, num_hidden_layers=64, num_attention_heads=64,
                 num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0)
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
ROWS = [("Qwen3-0.6B", synth.QWEN3_0P6B, [("full", None), ("lora_r16_fp32", (lora.TARGETS, torch.float32)), ("lora_r16_bf16", (lora.TARGETS, BF)), ("full_again", None)]),
        ("Qwen3-8B", synth.QWEN3_8B, [("full", None), ("lora_r16_fp32", (lora.TARGETS, torch.float32)), ("lora_r16_bf16", (lora.TARGETS, BF)), ("full_again", None)]),
        ("Qwen3-30B-A3B", synth.QWEN3_30B_A3B, [("lora_r16_attn_fp32", (ATTN, torch.float32))]),
        ("Qwen3-32B", QWEN3_32B, [("lora_r16_fp32", (lora.TARGETS, torch.float32))])]
seqs = synth.as_tensors(synth.tau2(0))
maxlen = max(map(len, seqs))
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()
att = lambda: [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]


def build(cfg):
    torch.manual_seed(0)
    torch.set_default_dtype(BF)
    try:
        with torch.device(dev):
            model = Qwen3TreeLM(cfg)
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.fill_(1.0) if n.endswith("norm.weight") else p.normal_(0.0, 0.02)
    return model


def run(model, name):
    engine = TreeTrainingEngine(model.config, dev, BF, maxlen)
    torch.cuda.reset_peak_memory_stats()
    times, n_tokens, loss = [], 0, None
    for i in range(warmup + steps):
        model.zero_grad(set_to_none=True)
        trie = TokenTrie(seqs, att()); trie.backward_permute()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss = engine.backward(model, trie, loss_fn, 2048)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt); n_tokens = trie.n_tokens
    n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
    n_grads = sum(1 for p in model.parameters() if p.grad is not None)
    model.zero_grad(set_to_none=True)
    return {"row": name, "tokens_per_s": round(n_tokens * len(times) / sum(times), 1), "s_per_step": [round(t, 4) for t in times], "last_mode": engine.last_mode,
            "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1), "trainable_params_M": round(n_train / 1e6, 2), "tensors_with_grad": n_grads,
            "n_tokens": n_tokens, "packed_rows": engine.last_packed.plan.T if engine.last_packed is not None else None, "loss": float(loss)}


results = []
for geo, cfg, variants in ROWS:
    if only and geo not in only:
        continue
    try:
        model = build(cfg)
    except torch.OutOfMemoryError as e:
        results.append({"row": f"{geo}", "did_not_fit": "building the bf16 weights: " + str(e)[:120]})
        continue
    n_params = sum(p.numel() for p in model.parameters())
    for vname, spec in variants:
        name = f"{geo} {vname}"
        try:
            if spec is None:
                lora.detach(model)
                for p in model.parameters():
                    p.requires_grad_(True)
            else:
                lora.detach(model)
                lora.attach(model, 16, 32.0, spec[0], dtype=spec[1], seed=1)
                with torch.no_grad():
                    for n, p in model.named_parameters():
                        if ".lora_B." in n:
                            p.normal_(0.0, 0.02)
            r = run(model, name)
        except torch.OutOfMemoryError as e:
            r = {"row": name, "did_not_fit": str(e)[:160]}
            model.zero_grad(set_to_none=True)
        r["params_B"] = round(n_params / 1e9, 2)
        results.append(r)
        print(json.dumps(r), flush=True)
        gc.collect(); torch.cuda.empty_cache()
    del model
    gc.collect(); torch.cuda.empty_cache()
res = {"call": "synth.tau2(0), block_size 2048 (BASELINE config 2)", "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0), "rows": results}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
