#!/usr/bin/env python3
"""What a preference objective (DPO) costs per engine call, Qwen3-0.6B geometry (random init), bf16, full fine-tuning, one GPU.

Workload: synth.tau2(0), the flagship call of bench.py and of scripts/policy_loss_bench.py - 8 rollouts of 6 turns behind one
2000-token system prompt, 48 sequences of up to 16 k tokens - with the sequences paired inside the prompt group: turn t of rollout 2k
is the chosen and turn t of rollout 2k + 1 the rejected member of one pair (24 pairs).  The loss mask is zero over the system prompt.
The reference log-probs come from one engine.forward outside the timed window and stay on the device.

Variants (one per process run)
  default    : engine.backward(model, trie, PreferenceLoss(beta=0.1, scale=1/24))  - the fused path: one model forward, the objective
               on the packed rows in one C-ABI call
  --baseline : the two-pass form written HERE from engine.forward, plain torch and a closure only, so that it runs on any revision of
               the package: a no-grad forward for the sequence log-probs, the DPO coefficients in torch, engine.backward with the
               linear closure g_s (m logprob).sum().  Compare the fused run against this variant run on the PARENT revision.

Per run: tokens/s over the timed calls (host clock around calls that end in a device synchronise), host milliseconds per call, and -
from one more call under torch.profiler - the number of device launches (kernels and copies) between the last forward kernel of the LM
head and the first kernel of its backward: the loss stage (`null`: the profiler gave no device events, not zero).  One JSON object per
run is appended to --out.
Usage: python scripts/preference_bench.py [--baseline] [--steps 4] [--warmup 2] [--label TEXT] [--out profiles/preference_first_form.json]"""
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

BETA, SYS_LEN, TURNS = 0.1, 2000, 6
dev = torch.device("cuda:0")
BF = torch.bfloat16


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


def pairs_of(n_seq):
    """(chosen, rejected) original sequence ids: turn t of rollout 2k against turn t of rollout 2k + 1"""
    return [((2 * k) * TURNS + t, (2 * k + 1) * TURNS + t) for k in range(n_seq // (2 * TURNS)) for t in range(TURNS)]


def two_pass_step(engine, model, seqs, attachments, pairs):
    """The baseline: DPO through engine.forward, plain torch and a linear closure.  Returns (trie, loss)."""
    atts = attachments()
    trie = TokenTrie(seqs, atts); trie.backward_permute()
    lps = engine.forward(model, trie)                                   # per original sequence id
    u = torch.stack([(a["loss_mask"].float() * (lp - a["ref_logprobs"])).sum() for lp, a in zip(lps, atts)])
    c, r = (torch.tensor(ix, device=dev) for ix in zip(*pairs))
    z = BETA * (u[c] - u[r])
    scale = 1.0 / len(pairs)
    loss = scale * torch.nn.functional.softplus(-z).sum()
    d = scale * BETA * (torch.sigmoid(z) - 1.0)
    g = torch.zeros_like(u)
    g[c], g[r] = d, -d
    closure = lambda logprob, entropy, att: g[att["_sequence_batch_id"]] * (att["loss_mask"].to(logprob.dtype) * logprob).sum()
    engine.backward(model, trie, closure, 2048)
    return trie, float(loss)


def fused_step(engine, model, seqs, attachments, loss_obj):
    trie = TokenTrie(seqs, attachments()); trie.backward_permute()
    return trie, engine.backward(model, trie, loss_obj, 2048)


def loss_stage_launches(step):
    """Device launches between the LM head's last forward kernel and the first kernel of its backward, from one profiled call (in
    the baseline: of its backward call, whose head forward is the second of the step)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = sorted((e for e in prof.events() if str(e.device_type).endswith("CUDA")), key=lambda e: e.time_range.start)
    names = [e.name for e in evs]
    bwd = [i for i, n in enumerate(names) if "logprob_entropy_bwd" in n]
    if not bwd:
        return None
    fwd = [i for i, n in enumerate(names) if "logprob_entropy_fwd" in n and i < bwd[0]]
    return bwd[0] - fwd[-1] - 1 if fwd else None


def run(a, model):
    seqs = synth.as_tensors(synth.tau2(0))
    pairs = pairs_of(len(seqs))
    engine = TreeTrainingEngine(make_config(synth.QWEN3_0P6B), dev, BF, max_seq_len=16384)
    base = engine.forward(model, TokenTrie(seqs))
    g = torch.Generator(device=dev).manual_seed(2)
    fixed = []
    for lp in base:
        n = lp.shape[0]
        mask = torch.rand(n, generator=g, device=dev) < 0.9
        mask[:SYS_LEN - 1] = False
        fixed.append({"ref_logprobs": lp + (torch.rand(n, generator=g, device=dev) - 0.5) * 0.6, "loss_mask": mask})
    for q, (c, r) in enumerate(pairs):
        fixed[c].update(pair_id=q, chosen=True); fixed[r].update(pair_id=q, chosen=False)
    attachments = lambda: [dict(x) for x in fixed]
    del base
    if a.baseline:
        step = lambda: two_pass_step(engine, model, seqs, attachments, pairs)
    else:
        from dynamictreeattn_amd.losses import PreferenceLoss
        loss_obj = PreferenceLoss(beta=BETA, scale=1.0 / len(pairs))
        step = lambda: fused_step(engine, model, seqs, attachments, loss_obj)
    wall, host = [], []
    for i in range(a.warmup + a.steps):
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        trie, loss = step()
        t1 = time.perf_counter()
        torch.cuda.synchronize(); t2 = time.perf_counter()
        if i >= a.warmup:
            wall.append(t2 - t0); host.append(t1 - t0)
    try:
        model.zero_grad(set_to_none=True)
        launches = loss_stage_launches(step)
    except Exception as exc:                                            # the profiler is optional equipment: say so, do not guess
        launches = None
        print(f"profiler unavailable: {exc!r}", file=sys.stderr)
    model.zero_grad(set_to_none=True)
    return {"workload": "tau2", "sequences": len(seqs), "pairs": len(pairs), "n_tokens": trie.n_tokens,
            "tree_tokens": sum(trie.lens) - sum(trie.lcp_lens), "mode": engine.last_mode,
            "loss_path": "two_pass (in the script)" if a.baseline else getattr(engine, "last_loss_path", None), "loss": float(loss),
            "timed": "trie build + " + ("forward + coefficients + backward" if a.baseline else "backward"),
            "tokens_per_s": round(trie.n_tokens * len(wall) / sum(wall), 1), "s_per_call": [round(t, 4) for t in wall],
            "host_ms_per_call": round(1e3 * sum(host) / len(host), 2), "loss_stage_launches": launches}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", action="store_true", help="the two-pass form from engine.forward, torch and a closure (runs on any revision)")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "preference_first_form.json"))
    a = ap.parse_args()
    rec = {"metric": "preference_loss_engine_call", "model": "Qwen3-0.6B geometry (random init), bf16", "objective": f"DPO, beta {BETA}",
           "variant": "two_pass_baseline" if a.baseline else "fused", "label": a.label, "steps": a.steps, "warmup": a.warmup,
           "runs": [run(a, build_model())]}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    prior = json.load(open(a.out)) if os.path.exists(a.out) else []
    with open(a.out, "w") as f:
        json.dump(prior + [rec], f, indent=1)
