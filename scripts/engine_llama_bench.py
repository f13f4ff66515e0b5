#!/usr/bin/env python3
"""End-to-end TreeTrainingEngine.backward tokens/s at Llama-3.2-1B and Llama-3.1-8B geometry on the tau2-shaped call: unmodified
transformers.LlamaForCausalLM, random init, bf16, the released models' rope_parameters (rope_type llama3, factor 32 / 8), the
engine's auto mode.  Qwen3-8B geometry (Qwen3TreeLM) is measured in the same process beside the 8B row.
Usage: python scripts/engine_llama_bench.py [steps] [warmup] [models: 1b,8b,qwen3-8b]   -> one JSON line per model."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import transformers
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 1
which = (sys.argv[3] if len(sys.argv) > 3 else "1b,8b,qwen3-8b").split(",")
dev = torch.device("cuda:0")
BF = torch.bfloat16
ROPE = {"rope_type": "llama3", "rope_theta": 500000.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
LLAMA = {"1b": ("Llama-3.2-1B", dict(vocab_size=128256, hidden_size=2048, intermediate_size=8192, num_hidden_layers=16, num_attention_heads=32,
                                     num_key_value_heads=8, head_dim=64, rms_norm_eps=1e-5, tie_word_embeddings=True,
                                     max_position_embeddings=131072, rope_parameters=dict(ROPE, factor=32.0))),
         "8b": ("Llama-3.1-8B", dict(vocab_size=128256, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32,
                                     num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5, tie_word_embeddings=False,
                                     max_position_embeddings=131072, rope_parameters=dict(ROPE, factor=8.0)))}
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()


def build(name):
    torch.manual_seed(0)
    torch.set_default_dtype(BF)                       # build the parameters in bf16 directly on the card
    try:
        with torch.device(dev):
            if name in LLAMA:
                label, model = LLAMA[name][0] + " geometry, unmodified LlamaForCausalLM", transformers.LlamaForCausalLM(transformers.LlamaConfig(**LLAMA[name][1]))
            else:
                label, model = "Qwen3-8B geometry, Qwen3TreeLM", Qwen3TreeLM(synth.QWEN3_8B)
    finally:
        torch.set_default_dtype(torch.float32)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.fill_(1.0) if n.endswith("norm.weight") else p.normal_(0.0, 0.02)
    return label, model.train()


for name in which:
    label, model = build(name)
    V = model.config.vocab_size
    seqs = synth.as_tensors(synth.tau2(0, V=V))
    maxlen = max(map(len, seqs))
    att = lambda: [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]
    engine = TreeTrainingEngine(model.config, dev, BF, maxlen)
    torch.cuda.reset_peak_memory_stats()
    times, n_tokens = [], 0
    for i in range(warmup + steps):
        model.zero_grad(set_to_none=True)
        trie = TokenTrie(seqs, att()); trie.backward_permute()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss = engine.backward(model, trie, loss_fn, 2048)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt); n_tokens = trie.n_tokens
    st = trie.get_stats("backward", 2048)
    print(json.dumps({"metric": "engine_backward_tokens_per_s", "model": f"{label} (random init), bf16", "mode": engine.last_mode,
                      "params_B": round(sum(p.numel() for p in model.parameters()) / 1e9, 2),
                      "value": round(n_tokens * len(times) / sum(times), 1), "unit": "tokens/s", "n_tokens": n_tokens,
                      "n_tree_tokens": st["n_tree_tokens"], "s_per_step": [round(t, 4) for t in times], "loss": float(loss),
                      "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}), flush=True)
    model.zero_grad(set_to_none=True)
    del model, engine
    torch.cuda.empty_cache()
