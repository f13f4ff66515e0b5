#!/usr/bin/env python3
"""Phi-4 / GLM-4 measurements on the tau2 trie (synth.tau2(0)), bf16, one MI355X.

kernels : at the Phi-4-mini q shape (24 heads of 128, read in place from the fused [T, 24 + 2*8, 128] projection output; the gradient
          written into the fused gradient buffer) and at the call's own row count, in one process and alternating:
            existing_a / existing_b   dta_qk_norm_rope_fwd / _bwd with w = NULL, the kernel the full-head families run - the same
                                      launch timed twice per round: the two columns' difference is the session's run-to-run spread
            full                      dta_rope_partial_fwd / _bwd at R = D = 128, half-split (the same arithmetic)
            r96                       R = 96, half-split (Phi-4-mini)
            r64_interleaved           R = 64, interleaved pairs (GLM-4's rotary dimension, at this shape)
          Three rounds per direction, HIP-event time per call over `iters` calls; HBM bytes from the shapes (one read of every input,
          one write of every output), bytes/s as a share of 8 TB/s; and whether `full` gives the existing kernel's bits.
engine  : TreeTrainingEngine.backward tokens/s, engine mode and peak HBM over unmodified transformers classes, random init, full
          fine-tuning: "phi4_mini" (Phi3ForCausalLM: hidden 3072, 24 / 8 heads of 128, R = 96, longrope, intermediate 8192, 32 layers,
          vocab 200 064, tied head; the tau2 sequences lie on both sides of original_max_position_embeddings = 4096, so the engine is
          told longrope_factors = "long", as a sampler with a 131 072 context is), "phi4_14b" (hidden 5120, 40 / 10 heads, the whole
          head rotated, intermediate 17 920, 40 layers, vocab 100 352) and "glm4_9b" (Glm4ForCausalLM: hidden 4096, 32 / 2 heads,
          R = 64 interleaved, intermediate 13 696, 40 layers, vocab 151 552).
Prints one JSON line per measurement; --save appends them to the record lists of profiles/phi_glm_bench.json.
Usage: python scripts/phi_glm_bench.py [kernels,phi4_mini,phi4_14b,glm4_9b] [iters] [engine steps] [engine warmup] [--save]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd._lib import ptr
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

argv = [a for a in sys.argv[1:] if a != "--save"]
SAVE = "--save" in sys.argv
what = (argv[0] if len(argv) > 0 else "kernels").split(",")
iters = int(argv[1]) if len(argv) > 1 else 200
steps = int(argv[2]) if len(argv) > 2 else 2
warmup = int(argv[3]) if len(argv) > 3 else 1
dev = torch.device("cuda:0")
BF = torch.bfloat16
PEAK = 8e12                                   # bytes/s
OUT = os.path.join(ROOT, "profiles", "phi_glm_bench.json")
RECORDS = []

_LONG = [1.0 + 0.6 * i for i in range(48)]
_SHORT = [1.0 + 0.01 * i for i in range(48)]
PHI4_MINI = dict(vocab_size=200064, hidden_size=3072, intermediate_size=8192, num_hidden_layers=32, num_attention_heads=24,
                 num_key_value_heads=8, rms_norm_eps=1e-5, max_position_embeddings=131072, original_max_position_embeddings=4096,
                 tie_word_embeddings=True, pad_token_id=None, eos_token_id=None, bos_token_id=None, sliding_window=None,
                 rope_parameters={"rope_type": "longrope", "rope_theta": 10000.0, "partial_rotary_factor": 0.75, "short_factor": _SHORT,
                                  "long_factor": _LONG})
PHI4_14B = dict(vocab_size=100352, hidden_size=5120, intermediate_size=17920, num_hidden_layers=40, num_attention_heads=40,
                num_key_value_heads=10, rms_norm_eps=1e-5, max_position_embeddings=16384, tie_word_embeddings=False, pad_token_id=None,
                eos_token_id=None, bos_token_id=None, sliding_window=None, rope_parameters={"rope_type": "default", "rope_theta": 250000.0})
GLM4_9B = dict(vocab_size=151552, hidden_size=4096, intermediate_size=13696, num_hidden_layers=40, num_attention_heads=32,
               num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5, max_position_embeddings=32768, tie_word_embeddings=False,
               attention_bias=True, pad_token_id=None, eos_token_id=None,
               rope_parameters={"rope_type": "default", "rope_theta": 10000.0, "partial_rotary_factor": 0.5})


def emit(rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


def _time(fn):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernels(Hq=24, Hkv=8, D=128):
    seqs = synth.as_tensors(synth.tau2(0))
    trie = TokenTrie(seqs); trie.backward_permute()
    T, H3, es, dt = trie.n_tokens, Hq + 2 * Hkv, 2, ops._DT[BF]
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(T, H3, D, generator=g, device=dev).to(BF)               # the fused projection output; q is its first Hq heads
    dqkv = torch.randn(T, H3, D, generator=g, device=dev).to(BF)              # the fused gradient buffer
    x, dbuf = qkv[:, :Hq], dqkv[:, :Hq]
    dy = torch.randn(T, Hq, D, generator=g, device=dev).to(BF)
    depth = torch.randint(0, 16384, (T,), generator=g, device=dev)
    tables = {R: ops.rope_cos_sin(depth, R, 1e4) for R in (128, 96, 64)}
    y = torch.empty(T, Hq, D, dtype=BF, device=dev)
    st = x.stride(0)

    def existing_fwd():
        cs = tables[128]
        ops._launch("dta_qk_norm_rope_fwd", (x, cs), ptr(x), None, ptr(cs), ptr(y), None, T, Hq, D, st, 1e-6, dt)

    def existing_bwd():
        cs = tables[128]
        ops._launch("dta_qk_norm_rope_bwd", (dy, cs), None, None, ptr(cs), ptr(dy), None, ptr(dbuf), None, T, Hq, D, st, Hq * D, D, dbuf.stride(0), dt)

    def partial(R, pairing):
        cs = tables[R]

        def fwd():
            ops._launch("dta_rope_partial_fwd", (x, cs), ptr(x), ptr(cs), ptr(y), T, Hq, D, R, pairing, st, dt)

        def bwd():
            ops._launch("dta_rope_partial_bwd", (cs, dy), ptr(cs), ptr(dy), ptr(dbuf), T, Hq, D, R, pairing, Hq * D, D, dbuf.stride(0), dt)
        return fwd, bwd

    forms = {"existing_a": (existing_fwd, existing_bwd), "existing_b": (existing_fwd, existing_bwd), "full": partial(128, 0),
             "r96": partial(96, 0), "r64_interleaved": partial(64, 1)}
    # the same bits at R = D?  (the arithmetic is the same; the compiler may contract the two products differently)
    existing_fwd(); ref_y = y.clone(); existing_bwd(); ref_dx = dbuf.clone()
    forms["full"][0](); same_y = bool(torch.equal(y, ref_y)); dy_max = float((y.float() - ref_y.float()).abs().max())
    forms["full"][1](); same_dx = bool(torch.equal(dbuf, ref_dx))
    row = T * Hq * D * es
    nbytes = {k: 2 * row + T * R * 4 for k, R in (("existing_a", 128), ("existing_b", 128), ("full", 128), ("r96", 96), ("r64_interleaved", 64))}
    rounds = []
    for _ in range(3):
        r = {}
        for k, (fwd, bwd) in forms.items():
            r[k + "_fwd"] = _time(fwd)
        for k, (fwd, bwd) in forms.items():
            r[k + "_bwd"] = _time(bwd)
        rounds.append(r)
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    spread = {d: round(max(abs(r["existing_a_" + d] - r["existing_b_" + d]) / r["existing_a_" + d] for r in rounds), 4) for d in ("fwd", "bwd")}
    emit({"metric": "rope_partial_ms", "q_heads": Hq, "kv_heads": Hkv, "head_dim": D, "T": T, "iters": iters,
          "rounds_ms": [{k: round(v, 4) for k, v in r.items()} for r in rounds], "best_ms": {k: round(v, 4) for k, v in best.items()},
          "bytes": nbytes, "existing_run_to_run_spread": spread,
          "over_existing": {k + "_" + d: round(best[k + "_" + d] / min(best["existing_a_" + d], best["existing_b_" + d]), 3)
                            for k in ("full", "r96", "r64_interleaved") for d in ("fwd", "bwd")},
          "TB_per_s": {k + "_" + d: round(nbytes[k] / best[k + "_" + d] / 1e9, 2) for k in forms for d in ("fwd", "bwd")},
          "share_of_8TBps": {k + "_" + d: round(nbytes[k] / (best[k + "_" + d] * 1e-3) / PEAK, 3) for k in forms for d in ("fwd", "bwd")},
          "full_equals_existing_bits": {"y": same_y, "dx": same_dx, "y_max_abs_diff": dy_max}})


def engine(name):
    import transformers
    cls, geo, label, attrs = {
        "phi4_mini": ("Phi3", PHI4_MINI, "Phi-4-mini geometry, unmodified Phi3ForCausalLM, longrope_factors = long", {"longrope_factors": "long"}),
        "phi4_14b": ("Phi3", PHI4_14B, "Phi-4 14B geometry, unmodified Phi3ForCausalLM", {}),
        "glm4_9b": ("Glm4", GLM4_9B, "GLM-4-9B-0414 geometry, unmodified Glm4ForCausalLM", {})}[name]
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
    for k, v in attrs.items():
        setattr(e, k, v)
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
    emit({"metric": "engine_backward_tokens_per_s", "model": label + " (random init), bf16, full fine-tuning",
          "mode": e.last_mode, "params_B": round(sum(p.numel() for p in model.parameters()) / 1e9, 2),
          "value": round(trie.n_tokens * len(times) / sum(times), 1), "unit": "tokens/s", "n_tokens": trie.n_tokens,
          "s_per_step": [round(t, 4) for t in times], "loss": float(loss),
          "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)})
    model.zero_grad(set_to_none=True)
    del model, e
    torch.cuda.empty_cache()


if __name__ == "__main__":
    if "kernels" in what:
        kernels()
    for name in ("phi4_mini", "glm4_9b", "phi4_14b"):
        if name in what:
            engine(name)
    if SAVE:                                   # the committed file keeps a header beside the two record lists
        doc = json.load(open(OUT)) if os.path.exists(OUT) else {"script": "scripts/phi_glm_bench.py", "kernels": [], "engine": []}
        for rec in RECORDS:
            doc["kernels" if rec["metric"] == "rope_partial_ms" else "engine"].append(rec)
        with open(OUT, "w") as f:
            json.dump(doc, f, indent=1)
