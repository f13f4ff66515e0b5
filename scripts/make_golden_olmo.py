#!/usr/bin/env python3
"""Generate tests/golden/engine_olmo.pt by IMPORTING THE REFERENCE (build container only): the reference's dense per-sequence path
(dense.py) over the unmodified transformers Olmo2ForCausalLM / Olmo3ForCausalLM models of tests/test_olmo_fixture.py, fp32 on the CPU
with eager attention - the protocol of scripts/make_golden_gemma.py.  Every record: fwd_dense; fwd_dense_off_wide_norm (q_norm / k_norm
per head with the first head_dim weights) and, for olmo3, fwd_dense_off_window and fwd_dense_off_yarn (the same weights with ONE feature
removed); the dense backward's loss and every gradient (fp16 of g / max|g| and the scale); gradient norms.

It also measures what the fixture tests rely on and prints it: each feature gap max |fwd_dense - fwd_dense_off_*| (must be >= 0.4) and
HF's OWN bf16 run against its fp32 run (forward logprob error, loss, per-parameter gradient ratios) next to the bf16 bounds the GPU
tests apply - a scale at which HF itself is outside them would make those tests measure the fixture, not the engine.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_olmo.py"""
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.modules["areal"] = types.ModuleType("areal")               # absent third-party dependency of vocab_parallel.py:8
_p = types.ModuleType("areal.platforms"); _p.is_npu_available = True
sys.modules["areal.platforms"] = _p

import numpy as np
import torch

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_olmo_fixture as fx
from oracle import model_oracle as mo

import dense                                                     # the reference's

GOLD = os.path.join(ROOT, "tests", "golden")
RECORDED = json.load(open(os.path.join(GOLD, "recorded_bf16_table.json")))
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()


def run(model, seqs, backward=True):
    model.zero_grad()
    fwd = [x.detach().float().clone() for x in dense.forward(model, list(seqs), use_tqdm=False)]
    if not backward:
        return fwd, None, None
    loss = dense.backward(model, list(seqs), fx.att(len(seqs)), loss_fn, act_ckpt=False, use_tqdm=False)
    return fwd, float(loss), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}


def make(case):
    seqs = [torch.tensor(s, dtype=torch.long) for s in fx.seqs_of(case)]
    fwd, loss, grads = run(fx.hf_model(case), seqs)
    rec = {"fwd_dense": fwd, "bwd_dense_loss": loss, "std": fx.CASE_STD.get(case, fx.STD)}
    gaps = {}
    for off in fx.offs_of(case):
        rec["fwd_dense_off_" + off] = run(fx.hf_model(case, off), seqs, backward=False)[0]
        gaps[off] = max(float((a - b).abs().max()) for a, b in zip(fwd, rec["fwd_dense_off_" + off]))
    # HF's own bf16 against its fp32, with the bounds the GPU tests apply to the engine
    fwd16, loss16, grads16 = run(fx.hf_model(case).to(torch.bfloat16), seqs)
    err = torch.cat([(a - b).abs() for a, b in zip(fwd16, fwd)])
    ratios = {n: mo.grad_ratio(grads[n], grads16[n]) for n in grads}
    print(f"{case}: {len(seqs)} sequences, max len {max(map(len, seqs))}, loss {loss:.6f}, gaps "
          + ", ".join(f"{k} {v:.3f}" for k, v in gaps.items()) + f" (>= {fx.MIN_GAP}); "
          f"HF bf16 vs fp32: logprob err max {float(err.max()):.4f} / mean {float(err.mean()):.4f} (bounds 0.08 / 0.015), "
          f"loss rel {abs(loss16 - loss) / abs(loss):.2e} (1e-2), grad ratio max {max(ratios.values()):.4f} ({RECORDED['max']:.4f}) "
          f"median {float(np.median(list(ratios.values()))):.4f} ({RECORDED['median']:.4f})")
    assert all(g >= fx.MIN_GAP for g in gaps.values()), (case, gaps)
    rec["bwd_dense_grads_fp16_scaled"] = {n: ((g / g.abs().max()).half(), float(g.abs().max())) for n, g in grads.items()}
    rec["grad_norms"] = {n: float(g.norm()) for n, g in grads.items()}
    return rec


if __name__ == "__main__":
    content = {fx.CASES[case][0]: make(case) for case in fx.CASES}
    torch.save(content, os.path.join(GOLD, fx.FILE))
    print(fx.FILE, os.path.getsize(os.path.join(GOLD, fx.FILE)), "bytes")
