#!/usr/bin/env python3
"""What the built-in policy objective costs per engine call, Qwen3-0.6B geometry (random init), bf16, full fine-tuning, one GPU.

Workloads
  tau2  : synth.tau2(0) - 48 sequences of up to 16 k tokens, the flagship call of bench.py.
  short : many short rollouts behind one prompt: --seqs sequences of --len tokens sharing their first --prefix tokens (default
          512 x 1024 with 256 shared).  The record names the engine mode and the loss path each call really took.
Variants (one per process run: --variant)
  fused    : engine.backward(model, trie, PolicyLoss(...))            - the objective on the packed rows, one C-ABI call
  lambda   : the same object behind a lambda                          - the per-sequence callback path
  closure  : a hand-written closure of the same objective that uses nothing but torch - runs on any revision of the package; the
             baseline
--ratio sequence runs every variant with one importance ratio per sequence (GSPO, PolicyLoss(ratio="sequence")); the closure is then
the hand-written sequence-level objective.
--is-level token|sequence|sequence_mean [--is-mode truncate|mask] adds a rollout importance weight (an off-policy correction) and
--surrogate cispo swaps the clipped surrogate for CISPO, in every variant: the closure is then the hand-written objective with the
weight / the CISPO form (closure_offpolicy).  rollout_logprobs are synthesised as old_logprobs plus 0.05 nats of noise; --no-old drops
old_logprobs from the attachments (one gradient step per batch: the weight is formed from the trainer's own log-probs).
Old and reference log-probs come from one engine.forward per workload (outside the timed window) and stay on the device.

Per workload and variant: tokens/s over the timed calls (host clock around calls that end in a device synchronise), host milliseconds
per call (until backward() returns: the loss has landed, the backward is queued), and - from one more call under torch.profiler - the
number of device launches (kernels and copies) between the last forward kernel of the LM head and the first kernel of its backward:
the loss stage.  `null` there means the profiler gave no device events, not zero.  One JSON object per run is appended to --out.
Usage: python scripts/policy_loss_bench.py --variant fused|lambda|closure [--ratio token|sequence] [--is-level ...] [--is-mode ...]
       [--surrogate ppo|cispo] [--no-old] [--workloads tau2,short] [--steps 4] [--warmup 2] [--out profiles/policy_loss_bench.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("DTA_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import Qwen3TreeLM, make_config
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

CLIP_LOW, CLIP_HIGH, KL_COEF, ENT_COEF = 0.2, 0.28, 0.02, 0.001
IS_CAP, IS_FLOOR = 2.0, 0.5
dev = torch.device("cuda:0")
BF = torch.bfloat16


def closure_loss(logprob, entropy, att):
    """The objective of PolicyLoss(clip_low=0.2, clip_high=0.28, kl_coef=0.02, kl_estimator="k3", entropy_coef=0.001), by hand."""
    A, m = att["advantages"], att["loss_mask"].to(logprob.dtype)
    r = torch.exp(logprob - att["old_logprobs"])
    pg = torch.maximum(-r * A, -torch.clamp(r, 1.0 - CLIP_LOW, 1.0 + CLIP_HIGH) * A)
    d = att["ref_logprobs"] - logprob
    term = pg + KL_COEF * (torch.exp(d) - d - 1.0) - ENT_COEF * entropy[:-1]
    return (m * term).sum() / torch.clamp(m.sum(), min=1.0)


def closure_loss_seq(logprob, entropy, att):
    """The same with ratio="sequence": every token of the sequence is clipped on the geometric mean of the masked tokens' ratios."""
    A, m = att["advantages"], att["loss_mask"].to(logprob.dtype)
    n = torch.clamp(m.sum(), min=1.0)
    r = torch.exp((m * (logprob - att["old_logprobs"])).sum() / n)
    pg = torch.maximum(-r * A, -torch.clamp(r, 1.0 - CLIP_LOW, 1.0 + CLIP_HIGH) * A)
    d = att["ref_logprobs"] - logprob
    term = pg + KL_COEF * (torch.exp(d) - d - 1.0) - ENT_COEF * entropy[:-1]
    return (m * term).sum() / n


def closure_offpolicy(ratio, surrogate, is_level, is_mode):
    """The objective with a rollout importance weight and / or the CISPO surrogate, by hand, with nothing but torch: what a user of a
    revision without them writes.  old_logprobs absent: the detached log-probs stand for them."""
    def loss_fn(logprob, entropy, att):
        A, m = att["advantages"], att["loss_mask"].to(logprob.dtype)
        n = torch.clamp(m.sum(), min=1.0)
        old = att["old_logprobs"] if att.get("old_logprobs") is not None else logprob.detach()
        r = torch.exp((m * (logprob - old)).sum() / n) if ratio == "sequence" else torch.exp(logprob - old)
        if surrogate == "cispo":
            pg = -torch.clamp(r, 1.0 - CLIP_LOW, 1.0 + CLIP_HIGH).detach() * A * logprob
        else:
            pg = torch.maximum(-r * A, -torch.clamp(r, 1.0 - CLIP_LOW, 1.0 + CLIP_HIGH) * A)
        if is_level is not None:
            y = old - att["rollout_logprobs"]
            if is_level != "token":
                y = (m * y).sum() / (n if is_level == "sequence_mean" else 1.0)
            rho = torch.exp(y)
            if is_mode == "truncate":
                omega = torch.clamp(rho, max=IS_CAP)
            else:
                omega = torch.where((rho >= IS_FLOOR) & (rho <= IS_CAP), rho, torch.zeros_like(rho))
            pg = omega * pg
        d = att["ref_logprobs"] - logprob
        term = pg + KL_COEF * (torch.exp(d) - d - 1.0) - ENT_COEF * entropy[:-1]
        return (m * term).sum() / n
    return loss_fn


def loss_of(variant, ratio="token", surrogate="ppo", is_level=None, is_mode="truncate", no_old=False):
    extended = surrogate != "ppo" or is_level is not None
    if variant == "closure":
        if extended or no_old:                                          # the plain closures read old_logprobs
            return closure_offpolicy(ratio, surrogate, is_level, is_mode)
        return closure_loss_seq if ratio == "sequence" else closure_loss
    from dynamictreeattn_amd.losses import PolicyLoss
    kw = {"ratio": ratio} if ratio != "token" else {}
    if extended:
        kw.update(surrogate=surrogate, is_level=is_level, is_mode=is_mode, is_cap=IS_CAP, is_floor=IS_FLOOR if is_mode == "mask" else 0.0)
    loss = PolicyLoss(clip_low=CLIP_LOW, clip_high=CLIP_HIGH, kl_coef=KL_COEF, kl_estimator="k3", entropy_coef=ENT_COEF, **kw)
    return loss if variant == "fused" else (lambda a, e, att: loss(a, e, att))


def build_model():
    m = Qwen3TreeLM(synth.QWEN3_0P6B).to(device=dev, dtype=BF)
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("norm.weight"):
                p.fill_(1.0)
            else:
                p.copy_((torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32) * 0.02).to(BF))
    return m.train()


def sequences(name, a):
    if name == "tau2":
        return synth.as_tensors(synth.tau2(0))
    g = torch.Generator().manual_seed(1)
    V = synth.QWEN3_0P6B["vocab_size"]
    prefix = torch.randint(0, V, (a.prefix,), generator=g)
    return [torch.cat([prefix, torch.randint(0, V, (a.len - a.prefix,), generator=g)]) for _ in range(a.seqs)]


def loss_stage_launches(model, engine, seqs, attachments, loss_fn):
    """Device launches between the LM head's last forward kernel and the first kernel of its backward, from one profiled call."""
    from torch.profiler import ProfilerActivity, profile
    model.zero_grad(set_to_none=True)
    trie = TokenTrie(seqs, attachments()); trie.backward_permute()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        engine.backward(model, trie, loss_fn, 2048)
        torch.cuda.synchronize()
    evs = sorted((e for e in prof.events() if str(e.device_type).endswith("CUDA")), key=lambda e: e.time_range.start)
    names = [e.name for e in evs]
    fwd = [i for i, n in enumerate(names) if "logprob_entropy_fwd" in n]
    if not fwd:
        return None
    bwd = [i for i, n in enumerate(names) if "logprob_entropy_bwd" in n and i > fwd[-1]]
    return bwd[0] - fwd[-1] - 1 if bwd else None


def run(name, a, model, loss_fn):
    seqs = sequences(name, a)
    engine = TreeTrainingEngine(make_config(synth.QWEN3_0P6B), dev, BF, max_seq_len=16384)
    base = engine.forward(model, TokenTrie(seqs))                       # per original sequence id, on the device
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda n, s: (torch.rand(n, generator=g, device=dev) - 0.5) * s
    fixed = [{"advantages": rnd(lp.shape[0], 2.0), "old_logprobs": lp + rnd(lp.shape[0], 0.6), "ref_logprobs": lp + rnd(lp.shape[0], 0.6),
              "loss_mask": torch.rand(lp.shape[0], generator=g, device=dev) < 0.8} for lp in base]
    if a.is_level is not None:                                          # the sampler's log-probs: old plus small noise
        for x in fixed:
            x["rollout_logprobs"] = x["old_logprobs"] + rnd(x["old_logprobs"].shape[0], 0.1)
    if a.no_old:
        for x in fixed:
            del x["old_logprobs"]
    attachments = lambda: [dict(x) for x in fixed]
    del base
    wall, host = [], []
    for i in range(a.warmup + a.steps):
        model.zero_grad(set_to_none=True)
        trie = TokenTrie(seqs, attachments()); trie.backward_permute()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loss = engine.backward(model, trie, loss_fn, 2048)
        t1 = time.perf_counter()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if i >= a.warmup:
            wall.append(t2 - t0); host.append(t1 - t0)
    try:
        launches = loss_stage_launches(model, engine, seqs, attachments, loss_fn)
    except Exception as exc:                                            # the profiler is optional equipment: say so, do not guess
        launches = None
        print(f"profiler unavailable: {exc!r}", file=sys.stderr)
    model.zero_grad(set_to_none=True)
    return {"workload": name, "sequences": len(seqs), "n_tokens": trie.n_tokens, "tree_tokens": sum(trie.lens) - sum(trie.lcp_lens),
            "mode": engine.last_mode, "loss_path": getattr(engine, "last_loss_path", "callback"), "loss": float(loss),
            "tokens_per_s": round(trie.n_tokens * len(wall) / sum(wall), 1), "s_per_call": [round(t, 4) for t in wall],
            "host_ms_per_call": round(1e3 * sum(host) / len(host), 2), "host_ms": [round(1e3 * t, 2) for t in host],
            "loss_stage_launches": launches}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["fused", "lambda", "closure"], default="fused")
    ap.add_argument("--closure", action="store_true", help="same as --variant closure")
    ap.add_argument("--ratio", choices=["token", "sequence"], default="token")
    ap.add_argument("--surrogate", choices=["ppo", "cispo"], default="ppo")
    ap.add_argument("--is-level", choices=["token", "sequence", "sequence_mean"], default=None)
    ap.add_argument("--is-mode", choices=["truncate", "mask"], default="truncate")
    ap.add_argument("--no-old", action="store_true", help="attachments without old_logprobs (one gradient step per batch)")
    ap.add_argument("--workloads", default="tau2,short")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seqs", type=int, default=512)
    ap.add_argument("--len", type=int, default=1024)
    ap.add_argument("--prefix", type=int, default=256)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "policy_loss_bench.json"))
    a = ap.parse_args()
    variant = "closure" if a.closure else a.variant
    model = build_model()
    fn = loss_of(variant, a.ratio, a.surrogate, a.is_level, a.is_mode, a.no_old)
    rec = {"metric": "policy_loss_engine_call", "model": "Qwen3-0.6B geometry (random init), bf16", "variant": variant, "ratio": a.ratio,
           "surrogate": a.surrogate, "is_level": a.is_level, "is_mode": a.is_mode if a.is_level is not None else None, "old_logprobs": not a.no_old,
           "label": a.label,
           "steps": a.steps, "warmup": a.warmup, "runs": [run(w, a, model, fn) for w in a.workloads.split(",")]}
    print(json.dumps(rec), flush=True)
    prior = json.load(open(a.out)) if os.path.exists(a.out) else []
    with open(a.out, "w") as f:
        json.dump(prior + [rec], f, indent=1)
