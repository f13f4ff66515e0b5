#!/usr/bin/env python3
"""A quantised frozen base beside the 16-bit one (quant.quantize_base): TreeTrainingEngine.backward on the tau2 call of
BASELINE config 2 (synth.tau2(0), block_size 2048) with LoRA r = 16 (fp32 adapters) on all seven projections, one process, sync to sync
after warm-up; random-init bf16 Qwen3TreeLM of the named geometry.  Rows:

    Qwen3-8B, Qwen3-32B geometry:   bf16 base | fp8 base | nf4 base     (the yardstick of a geometry is its own bf16 row of this session)
    Llama-3.3-70B geometry:          nf4 base                            (80 layers, hidden 8192, 64 / 8 heads, intermediate 28 672,
                                                                          vocab 128 256; only when named on the command line)

Every row: tokens/s, s per step, last_mode (kept / recomputed layers), peak HBM, HBM at rest, and the share of the step spent in
dta_dequant_blockwise - the kernel's summed device time from ops.KernelTimer in one extra instrumented step over the mean step time of
the timed steps - or that it did not fit.

`kernel`: dta_dequant_blockwise alone on an [8192, 28672] weight, both formats and both orientations, to bf16, with dta_transpose on the
bf16 matrix of the same shape beside it (that kernel moves more bytes); device events around `reps` launches; bytes moved / time.
Usage: python scripts/quant_bench.py [out.json] [steps] [warmup] [row ...]      rows: kernel Qwen3-8B Qwen3-32B Llama-3.3-70B"""
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import lora, ops, quant, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quant_bench.json")
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 2
only = sys.argv[4:] or ["kernel", "Qwen3-8B", "Qwen3-32B"]
dev = torch.device("cuda:0")
BF = torch.bfloat16
QWEN3_32B = dict(vocab_size=151936, hidden_size=5120, intermediate_size=25600, num_hidden_layers=64, num_attention_heads=64,
                 num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0)
LLAMA33_70B = dict(vocab_size=128256, hidden_size=8192, intermediate_size=28672, num_hidden_layers=80, num_attention_heads=64,
                   num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5, rope_theta=500000.0)
ROWS = [("Qwen3-8B", synth.QWEN3_8B, (None, "fp8", "nf4")), ("Qwen3-32B", QWEN3_32B, (None, "fp8", "nf4")), ("Llama-3.3-70B", LLAMA33_70B, ("nf4",))]

def tau2_call(vocab_size):
    """The tau2 call with token ids drawn below the geometry's vocabulary (the default draws below Qwen3's 151 936: ids a smaller
    embedding does not have)."""
    seqs = synth.as_tensors(synth.tau2(0, V=vocab_size))
    assert max(int(s.max()) for s in seqs) < vocab_size
    return seqs


loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()
att = lambda seqs: [{"w_logprobs": -1.0, "w_entropy": 0.1} for _ in seqs]


def build(cfg, fmt):
    """The bf16 model from one seed - every row of a geometry starts from the same weights - and, with `fmt`, its frozen base quantised
    in place by quant.quantize_base (the bf16 base stands in HBM as a whole until then: 141 GB at 70 B)."""
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
    if fmt is not None:
        for p in model.parameters():
            p.requires_grad_(False)
        quant.quantize_base(model, fmt)
        gc.collect(); torch.cuda.empty_cache()
    return model


def run(model, name):
    seqs = tau2_call(model.config.vocab_size)
    engine = TreeTrainingEngine(model.config, dev, BF, max(map(len, seqs)))
    torch.cuda.synchronize()
    rest = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times, n_tokens, loss = [], 0, None
    for i in range(warmup + steps):
        model.zero_grad(set_to_none=True)
        trie = TokenTrie(seqs, att(seqs)); trie.backward_permute()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss = engine.backward(model, trie, loss_fn, 2048)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt); n_tokens = trie.n_tokens
    peak = torch.cuda.max_memory_allocated()
    model.zero_grad(set_to_none=True)
    tm = ops.KernelTimer(); ops.KernelTimer.active = tm                # one more step, instrumented: not among the timed ones
    try:
        trie = TokenTrie(seqs, att(seqs)); trie.backward_permute()
        engine.backward(model, trie, loss_fn, 2048)
        ms, launches = tm.totals_ms().get("dta_dequant_blockwise", (0.0, 0))
    finally:
        ops.KernelTimer.active = None
    model.zero_grad(set_to_none=True)
    mean = sum(times) / len(times)
    return {"row": name, "tokens_per_s": round(n_tokens * len(times) / sum(times), 1), "s_per_step": [round(t, 4) for t in times],
            "last_mode": engine.last_mode, "peak_mem_GB": round(peak / 1e9, 1), "rest_mem_GB": round(rest / 1e9, 1),
            "dequant_ms_per_step": round(ms, 2), "dequant_launches": launches, "dequant_share_of_step": round(ms / 1e3 / mean, 4),
            "n_tokens": n_tokens, "loss": float(loss)}


def kernel_rates(reps=500, rounds=5):
    """The five kernels alternating, `rounds` times round the list; a sample is device events around `reps` back-to-back launches into a
    preallocated output (0.06 - 0.1 s).  Per kernel: the median sample and the spread (min, max) over the rounds."""
    R, C = 8192, 28672
    w = torch.randn(R, C, device=dev, dtype=BF)
    out_rc, out_cr = torch.empty((R, C), device=dev, dtype=BF), torch.empty((C, R), device=dev, dtype=BF)
    cases = [("dta_transpose bf16", 2 * R * C * 2,
              lambda: ops._launch("dta_transpose", (w, out_cr), ops.ptr(w), ops.ptr(out_cr), R, C, C, R, 2))]
    held = []
    for fmt in ("nf4", "fp8"):
        q, s = ops.quant_blockwise(w, fmt)
        held.append((q, s))
        for transposed in (False, True):
            cases.append((f"dta_dequant_blockwise {fmt} {'transposed' if transposed else 'row-major'} -> bf16", q.numel() + s.numel() * 4 + R * C * 2,
                          lambda q=q, s=s, fmt=fmt, t=transposed: ops.dequant_blockwise(q, s, fmt, out_cr if t else out_rc, t)))
    samples = {name: [] for name, _, _ in cases}
    for rnd in range(rounds + 1):                      # round 0 warms every kernel up and is dropped
        for name, _, fn in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); a.record()
            for _ in range(reps if rnd else 10):
                fn()
            b.record(); torch.cuda.synchronize()
            if rnd:
                samples[name].append(a.elapsed_time(b) / reps)
    out = []
    for name, nbytes, _ in cases:
        v = sorted(samples[name]); med = v[len(v) // 2]
        out.append({"kernel": name, "shape": [R, C], "reps": reps, "rounds": rounds, "ms_median": round(med, 4), "ms_min": round(v[0], 4),
                    "ms_max": round(v[-1], 4), "bytes": nbytes, "TB_per_s": round(nbytes / med / 1e9, 3)})
        print(json.dumps(out[-1]), flush=True)
    return out


res = {"call": "synth.tau2(0), block_size 2048 (BASELINE config 2), LoRA r = 16 fp32 adapters on all seven projections", "steps": steps,
       "warmup": warmup, "device": torch.cuda.get_device_name(0), "rows": [], "kernel": None}
if "kernel" in only:
    res["kernel"] = kernel_rates()
    gc.collect(); torch.cuda.empty_cache()
for geo, cfg, fmts in ROWS:
    if geo not in only:
        continue
    for fmt in fmts:
        name = f"{geo} {fmt or 'bf16'} base, lora_r16_fp32"
        model = None
        try:
            model = build(cfg, fmt)
            n_params = sum(p.numel() for p in model.parameters()) + sum(m.in_features * m.out_features for m in model.modules() if isinstance(m, quant.QuantLinear))
            lora.attach(model, 16, 32.0, lora.TARGETS, dtype=torch.float32, seed=1)
            with torch.no_grad():
                for n, p in model.named_parameters():
                    if ".lora_B." in n:
                        p.normal_(0.0, 0.02)
            r = run(model, name)
            r["params_B"] = round(n_params / 1e9, 2)
        except torch.OutOfMemoryError as e:
            r = {"row": name, "did_not_fit": str(e)[:160]}
        res["rows"].append(r)
        print(json.dumps(r), flush=True)
        del model
        gc.collect(); torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump(res, open(out_path, "w"), indent=1)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
