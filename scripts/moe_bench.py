#!/usr/bin/env python3
"""Qwen3-30B-A3B geometry (synth.QWEN3_30B_A3B: H 2048, I 768, 128 experts, top 8) through TreeTrainingEngine.backward on a tau2-shaped
call: Qwen3TreeLM with random-init bf16 weights, the engine's auto mode.  Reports tokens/s, the mode chosen and peak HBM; the grouped-GEMM
time and TFLOP/s per phase (fwd / dgrad / wgrad of gate|up and down) from KernelTimer spans of one step; and one MoE layer's expert
GEMMs (gate|up -> SwiGLU -> down, forward + backward) on one routing against a per-expert ops.linear loop (HF's eager form) and a dense
hipBLASLt GEMM pair of equal M.N.K.
Usage: python scripts/moe_bench.py [steps] [warmup] [layers]   -> one JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 1
layers = int(sys.argv[3]) if len(sys.argv) > 3 else synth.QWEN3_30B_A3B["num_hidden_layers"]
dev = torch.device("cuda:0")
BF = torch.bfloat16
cfg = dict(synth.QWEN3_30B_A3B, num_hidden_layers=layers)
H, I, E, K = cfg["hidden_size"], cfg["moe_intermediate_size"], cfg["num_experts"], cfg["num_experts_per_tok"]

torch.manual_seed(0)
torch.set_default_dtype(BF)                         # build the 30 B parameters in bf16 directly
with torch.device(dev):
    model = Qwen3TreeLM(cfg)
torch.set_default_dtype(torch.float32)
with torch.no_grad():
    for n, p in model.named_parameters():
        if n.endswith("norm.weight"):
            p.fill_(1.0)
        else:
            p.normal_(0.0, 0.02)
n_params = sum(p.numel() for p in model.parameters())
seqs = synth.as_tensors(synth.tau2(0))
maxlen = max(map(len, seqs))
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()
att = lambda: [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]
engine = TreeTrainingEngine(model.config, dev, BF, maxlen)
times, n_tokens, timer = [], 0, None
for i in range(warmup + steps):
    model.zero_grad(set_to_none=True)
    trie = TokenTrie(seqs, att()); trie.backward_permute()
    if i == warmup + steps - 1:
        timer = ops.KernelTimer(); ops.KernelTimer.active = timer
    torch.cuda.synchronize(); t0 = time.perf_counter()
    loss = engine.backward(model, trie, loss_fn, 2048)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    ops.KernelTimer.active = None
    if i >= warmup:
        times.append(dt); n_tokens = trie.n_tokens
st = trie.get_stats("backward", 2048)
T = engine.last_packed.plan.T if engine.last_packed is not None else None
phases = {}
for name, (ms, n) in timer.totals_ms().items():
    if not name.startswith("moe_gemm_") or n == 0:
        continue
    _, _, ph, nk = name.split("_")
    N_, K_ = map(int, nk.split("x"))
    flops = 2.0 * T * K * N_ * K_ * n if T else 0.0
    phases[f"{ph} {N_}x{K_}"] = {"ms": round(ms, 2), "calls": n, "TFLOP/s": round(flops / ms / 1e9, 1) if ms > 0 else None}
gemm_ms = sum(v["ms"] for v in phases.values())
peak = torch.cuda.max_memory_allocated() / 1e9
mode = engine.last_mode
model.zero_grad(set_to_none=True)
del model, engine
torch.cuda.empty_cache()

# one MoE layer's expert GEMMs on one routing: grouped kernels vs a per-expert ops.linear loop vs a dense GEMM pair of equal M.N.K
Tl = T or 16384
g = torch.Generator(device=dev).manual_seed(1)
h = torch.randn(Tl, H, device=dev, dtype=BF, generator=g)
wgu = (0.02 * torch.randn(E, 2 * I, H, device=dev, generator=g)).to(BF).requires_grad_(True)
wdn = (0.02 * torch.randn(E, H, I, device=dev, generator=g)).to(BF).requires_grad_(True)
ids, _, _ = ops.moe_router_fwd_raw(torch.randn(Tl, E, device=dev, generator=g).to(BF), K, True)
route = ops.moe_permute(ids, E)
offs = route.expert_offsets.cpu().tolist()            # host copy for the loop form only
src = route.src_token.long()
dy = torch.randn(Tl * K, H, device=dev, dtype=BF, generator=g)


def grouped():
    x = h.detach().requires_grad_(True)
    y = ops._MoeLinear.apply(ops.swiglu_fused(ops._MoeLinear.apply(x, wgu, route, True)), wdn, route, False)
    y.backward(dy)


def loop():
    xs = h[src].detach().requires_grad_(True)
    outs = []
    for e in range(E):
        a, b = offs[e], offs[e + 1]
        if b > a:
            outs.append(ops.linear(ops.swiglu_fused(ops.linear(xs[a:b], wgu[e])), wdn[e]))
    torch.cat(outs).backward(dy)


wgu_d = wgu[0].detach().clone().requires_grad_(True)
wdn_d = wdn[0].detach().clone().requires_grad_(True)


def dense():
    xs = h[src].detach().requires_grad_(True)
    ops.linear(ops.swiglu_fused(ops.linear(xs, wgu_d)), wdn_d).backward(dy)


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


layer_flops = 6.0 * Tl * K * (2 * I * H + H * I)          # fwd + dgrad + wgrad of both products
layer = {}
for name, fn in (("grouped", grouped), ("per_expert_loop", loop), ("dense_equal_mnk", dense)):
    ms = timed(fn)
    layer[name] = {"ms": round(ms, 3), "TFLOP/s": round(layer_flops / ms / 1e9, 1)}
print(json.dumps({"metric": "engine_backward_tokens_per_s", "model": f"Qwen3-30B-A3B geometry, {layers} layers (random init), bf16",
                  "params_B": round(n_params / 1e9, 2), "mode": mode, "value": round(n_tokens * len(times) / sum(times), 1), "unit": "tokens/s",
                  "n_tokens": n_tokens, "n_tree_tokens": st["n_tree_tokens"], "packed_rows": T, "s_per_step": [round(t, 3) for t in times],
                  "loss": float(loss), "peak_mem_GB": round(peak, 1), "moe_gemm_ms_in_step": round(gemm_ms, 1), "moe_gemm_phases": phases,
                  "one_layer_expert_gemms_fwd_bwd": layer}))
