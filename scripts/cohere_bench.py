#!/usr/bin/env python3
"""Cohere / Cohere2 measurements on the tau2 trie (synth.tau2(0)), bf16, one MI355X.

kernels : the LayerNorm kernels at [T, 4096] with T the call's own row count, beside dta_rmsnorm_* at the same shape in the same
          process, alternating:
            rms_a / rms_b        dta_rmsnorm_fwd (x + delta fused) / dta_rmsnorm_bwd (dres given) - the same launch timed twice per
                                 round: the two columns' difference is the session's run-to-run spread
            ln_plain             dta_layernorm_fwd without deltas (reads x and w, writes y)
            ln_one_delta         x_out = x + delta_a (reads x, delta_a, w; writes x_out, y): RMSNorm's fused form
            ln_two_deltas        x_out = x + delta_a + delta_b, the join of the parallel block (one read more)
            ln_bwd / ln_bwd_frozen   dta_layernorm_bwd with dres, with and without the dw partials
          Three rounds, HIP-event time per call over `iters` calls; HBM bytes counted per form from the shapes (one read of every
          input, one write of every output; mean / rstd and the partials included), bytes/s as a share of 8 TB/s.
engine  : TreeTrainingEngine.backward tokens/s, engine mode and peak HBM over unmodified transformers classes, random init, full
          fine-tuning: "command_r7b" (Cohere2ForCausalLM: 32 layers, hidden 4096, 32 / 8 heads of 128, intermediate 14 336, vocab
          256 000, tied head, logit_scale 0.25, layers 3 sliding : 1 full at sliding_window 4096) and "aya_8b" (CohereForCausalLM: the
          same sizes, every layer rotating, logit_scale 0.125).  The record states the values actually used.
Prints one JSON line per measurement; --save appends them to the record lists of profiles/cohere_first_form.json.
Usage: python scripts/cohere_bench.py [kernels,command_r7b,aya_8b] [iters] [engine steps] [engine warmup] [--save]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dynamictreeattn_amd import ops, synth
from dynamictreeattn_amd._lib import lib, ptr
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
OUT = os.path.join(ROOT, "profiles", "cohere_first_form.json")
RECORDS = []

SIZES = dict(vocab_size=256000, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8,
             head_dim=128, layer_norm_eps=1e-5, max_position_embeddings=131072, tie_word_embeddings=True, attention_bias=False, pad_token_id=None,
             eos_token_id=None, bos_token_id=None)
COMMAND_R7B = dict(SIZES, logit_scale=0.25, sliding_window=4096, layer_types=(["sliding_attention"] * 3 + ["full_attention"]) * 8,
                   rope_parameters={"rope_type": "default", "rope_theta": 50000.0})
AYA_8B = dict(SIZES, logit_scale=0.125, use_qk_norm=False, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})


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


def kernels(H=4096):
    seqs = synth.as_tensors(synth.tau2(0))
    trie = TokenTrie(seqs); trie.backward_permute()
    T, es, dt, eps = trie.n_tokens, 2, ops._DT[BF], 1e-5
    g = torch.Generator(device=dev).manual_seed(0)
    x, da, db, dy, dres = (torch.randn(T, H, generator=g, device=dev).to(BF) for _ in range(5))
    w = (1 + 0.1 * torch.randn(H, generator=g, device=dev)).to(BF)
    xo, y, dx = (torch.empty(T, H, dtype=BF, device=dev) for _ in range(3))
    mean, rstd, rstd_rms = (torch.empty(T, dtype=torch.float32, device=dev) for _ in range(3))
    blocks = lib().dta_layernorm_bwd_blocks(T)
    assert blocks == lib().dta_rmsnorm_bwd_blocks(T)
    part = torch.empty(blocks, H, dtype=torch.float32, device=dev)

    def ln_fwd(a, b):
        return lambda: ops._launch("dta_layernorm_fwd", (x, w), ptr(x), ptr(a), ptr(b), ptr(w), ptr(xo) if a is not None else None, ptr(y),
                                   ptr(mean), ptr(rstd), T, H, eps, dt)

    def ln_bwd(p):
        return lambda: ops._launch("dta_layernorm_bwd", (x, w, dy), ptr(x), ptr(w), ptr(dy), ptr(dres), ptr(mean), ptr(rstd), ptr(dx), ptr(p), T, H, dt)

    rms_fwd = lambda: ops._launch("dta_rmsnorm_fwd", (x, da, w), ptr(x), ptr(da), ptr(w), ptr(xo), ptr(y), ptr(rstd_rms), T, H, eps, 0.0, dt)
    rms_bwd = lambda: ops._launch("dta_rmsnorm_bwd", (x, w, dy), ptr(x), ptr(w), ptr(dy), ptr(dres), ptr(rstd_rms), ptr(dx), ptr(part), T, H, 0.0, dt)
    row, stat, wb, pb = T * H * es, T * 4, H * es, blocks * H * 4
    forms = {"rms_a_fwd": (rms_fwd, 4 * row + stat + wb), "rms_b_fwd": (rms_fwd, 4 * row + stat + wb),
             "ln_plain_fwd": (ln_fwd(None, None), 2 * row + 2 * stat + wb), "ln_one_delta_fwd": (ln_fwd(da, None), 4 * row + 2 * stat + wb),
             "ln_two_deltas_fwd": (ln_fwd(da, db), 5 * row + 2 * stat + wb)}
    bwd_forms = {"rms_a_bwd": (rms_bwd, 4 * row + stat + wb + pb), "rms_b_bwd": (rms_bwd, 4 * row + stat + wb + pb),
                 "ln_bwd": (ln_bwd(part), 4 * row + 2 * stat + wb + pb), "ln_bwd_frozen": (ln_bwd(None), 4 * row + 2 * stat + wb)}
    rounds = []
    for _ in range(3):
        r = {k: _time(fn) for k, (fn, _) in forms.items()}
        ln_fwd(None, None)(); rms_fwd()                   # the statistics the backwards read: of x itself
        r.update({k: _time(fn) for k, (fn, _) in bwd_forms.items()})
        rounds.append(r)
    forms.update(bwd_forms)
    best = {k: min(r[k] for r in rounds) for k in rounds[0]}
    spread = {d: round(max(abs(r["rms_a_" + d] - r["rms_b_" + d]) / r["rms_a_" + d] for r in rounds), 4) for d in ("fwd", "bwd")}
    emit({"metric": "layernorm_ms", "T": T, "H": H, "dtype": "bf16", "iters": iters,
          "rounds_ms": [{k: round(v, 4) for k, v in r.items()} for r in rounds], "best_ms": {k: round(v, 4) for k, v in best.items()},
          "bytes": {k: b for k, (_, b) in forms.items()}, "rmsnorm_run_to_run_spread": spread,
          "GB_per_s": {k: round(b / best[k] / 1e6, 1) for k, (_, b) in forms.items()},
          "share_of_8TBps": {k: round(b / (best[k] * 1e-3) / PEAK, 3) for k, (_, b) in forms.items()}})


def engine(name):
    import transformers
    cls, geo, label = {"command_r7b": ("Cohere2", COMMAND_R7B, "Command-R7B geometry, unmodified Cohere2ForCausalLM"),
                       "aya_8b": ("Cohere", AYA_8B, "Aya-Expanse-8B geometry, unmodified CohereForCausalLM")}[name]
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
    used = {k: geo[k] for k in ("num_hidden_layers", "hidden_size", "num_attention_heads", "num_key_value_heads", "head_dim", "intermediate_size",
                                "vocab_size", "logit_scale", "tie_word_embeddings")}
    used.update(sliding_window=geo.get("sliding_window"), layer_pattern="3 sliding : 1 full" if "layer_types" in geo else "every layer full, rotating",
                rope_theta=geo["rope_parameters"]["rope_theta"])
    emit({"metric": "engine_backward_tokens_per_s", "model": label + " (random init), bf16, full fine-tuning", "values_used": used,
          "mode": e.last_mode, "params_B": round(sum(p.numel() for p in model.parameters()) / 1e9, 2),
          "value": round(trie.n_tokens * len(times) / sum(times), 1), "unit": "tokens/s", "n_tokens": trie.n_tokens,
          "max_len": max(map(len, seqs)), "s_per_step": [round(t, 4) for t in times], "loss": float(loss),
          "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)})
    model.zero_grad(set_to_none=True)
    del model, e
    torch.cuda.empty_cache()


if __name__ == "__main__":
    if "kernels" in what:
        kernels()
    for name in ("command_r7b", "aya_8b"):
        if name in what:
            engine(name)
    if SAVE:                                   # the committed file keeps a header beside the two record lists
        doc = json.load(open(OUT)) if os.path.exists(OUT) else {"script": "scripts/cohere_bench.py", "kernels": [], "engine": []}
        for rec in RECORDS:
            doc["kernels" if rec["metric"] == "layernorm_ms" else "engine"].append(rec)
        with open(OUT, "w") as f:
            json.dump(doc, f, indent=1)
