#!/usr/bin/env python3
"""End-to-end TreeTrainingEngine.backward tokens/s at Qwen2.5-0.5B geometry (synth.QWEN25_0P5B: head_dim 64, 14 / 2 heads,
q/k/v biases, tied head) on a tau2-shaped call: an unmodified transformers.Qwen2ForCausalLM, random init, bf16, one packed pass.
Usage: python scripts/engine_qwen2_bench.py [steps] [warmup]   -> one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import transformers
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 1
dev = torch.device("cuda:0")
cfg = synth.QWEN25_0P5B
c = transformers.Qwen2Config(vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                             num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                             num_key_value_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], tie_word_embeddings=True,
                             max_position_embeddings=40960, rms_norm_eps=cfg["rms_norm_eps"],
                             rope_parameters={"rope_type": "default", "rope_theta": cfg["rope_theta"]})
torch.manual_seed(0)
model = transformers.Qwen2ForCausalLM(c).to(device=dev, dtype=torch.bfloat16).train()
seqs = synth.as_tensors(synth.tau2(0))
maxlen = max(map(len, seqs))
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()
att = lambda: [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]
engine = TreeTrainingEngine(model.config, dev, torch.bfloat16, maxlen)
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
print(json.dumps({"metric": "engine_backward_tokens_per_s", "model": "Qwen2.5-0.5B geometry (random init), bf16", "mode": engine.last_mode,
                  "value": round(n_tokens * len(times) / sum(times), 1), "unit": "tokens/s", "n_tokens": n_tokens,
                  "n_tree_tokens": st["n_tree_tokens"], "s_per_step": [round(t, 4) for t in times], "loss": float(loss),
                  "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}))
