#!/usr/bin/env python3
"""Generate tests/golden/engine_llama3.pt, engine_mistral.pt and engine_mixtral.pt by IMPORTING THE REFERENCE (build container only):
the reference's dense per-sequence path (dense.py) over the unmodified HF models of tests/test_llama_family_fixture.py, fp32 on the
CPU with eager attention.  Every record: fwd_dense, fwd_dense_off (the same weights with the feature off: default RoPE,
sliding_window None, biases zeroed), the dense backward's loss and every gradient (fp16 of g / max|g| and the scale), gradient norms.

It also measures what the fixture tests rely on and prints it: the feature gap max |fwd_dense - fwd_dense_off| (must be >= 0.4) and
HF's OWN bf16 run against its fp32 run (forward logprob error, loss, per-parameter gradient ratios) next to the bf16 bounds the GPU
tests apply - a scale at which HF itself is outside them would make those tests measure the fixture, not the engine.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_llama.py [case ...]"""
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
import test_llama_family_fixture as fx
from oracle import model_oracle as mo

import dense                                                     # the reference's

GOLD = os.path.join(ROOT, "tests", "golden")
RECORDED = json.load(open(os.path.join(GOLD, "recorded_bf16_table.json")))
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()


def run(model, seqs):
    model.zero_grad()
    fwd = [x.detach().float().clone() for x in dense.forward(model, list(seqs), use_tqdm=False)]
    loss = dense.backward(model, list(seqs), fx.att(len(seqs)), loss_fn, act_ckpt=False, use_tqdm=False)
    return fwd, float(loss), {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}


def make(case):
    seqs = [torch.tensor(s, dtype=torch.long) for s in fx.seqs_of(case)]
    fwd, loss, grads = run(fx.hf_model(case), seqs)
    fwd_off, loss_off, _ = run(fx.hf_model(case, off=True), seqs)
    gap = max(float((a - b).abs().max()) for a, b in zip(fwd, fwd_off))
    # HF's own bf16 against its fp32, with the bounds the GPU tests apply to the engine
    fwd16, loss16, grads16 = run(fx.hf_model(case).to(torch.bfloat16), seqs)
    err = torch.cat([(a - b).abs() for a, b in zip(fwd16, fwd)])
    ratios = {n: mo.grad_ratio(grads[n], grads16[n]) for n in grads}
    print(f"{case}: max len {max(map(len, seqs))}, loss {loss:.6f} (feature off {loss_off:.6f}), gap {gap:.3f} (>= {fx.MIN_GAP}); "
          f"HF bf16 vs fp32: logprob err max {float(err.max()):.4f} / mean {float(err.mean()):.4f} (bounds 0.08 / 0.015), "
          f"loss rel {abs(loss16 - loss) / abs(loss):.2e} (1e-2), grad ratio max {max(ratios.values()):.4f} ({RECORDED['max']:.4f}) "
          f"median {float(np.median(list(ratios.values()))):.4f} ({RECORDED['median']:.4f})")
    assert gap >= fx.MIN_GAP, (case, gap)
    packed = {n: ((g / g.abs().max()).half(), float(g.abs().max())) for n, g in grads.items()}
    return {"fwd_dense": fwd, "fwd_dense_off": fwd_off, "bwd_dense_loss": loss, "bwd_dense_loss_off": loss_off,
            "bwd_dense_grads_fp16_scaled": packed, "grad_norms": {n: float(g.norm()) for n, g in grads.items()}, "std": fx.CASE_STD.get(case, fx.STD)}


if __name__ == "__main__":
    what = sys.argv[1:] or list(fx.CASES)
    files = {}
    for case in what:
        file, rec = fx.CASES[case][:2]
        r = make(case)
        if rec is None:
            files[file] = r
        else:
            files.setdefault(file, {})[rec] = r
    for file, content in files.items():
        torch.save(content, os.path.join(GOLD, file))
        print(file, os.path.getsize(os.path.join(GOLD, file)), "bytes")
