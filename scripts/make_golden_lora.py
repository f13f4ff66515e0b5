#!/usr/bin/env python3
"""Generate tests/golden/engine_lora.pt by IMPORTING THE REFERENCE (build container only): the reference's dense per-sequence path
(dense.py) over the unmodified tiny HF models of tests/test_lora_fixture.py whose projections are wrapped by that file's `RefLora`
(a test-side restatement of the adapter layout), base frozen, fp32 on the CPU with eager attention.  Every record: fwd_dense,
fwd_dense_off (the same model with the adapters disabled), the dense backward's loss (and the loss with the adapters off) and every
ADAPTER gradient (fp16 of g / max|g| and the scale), gradient norms.

It asserts and prints what the tests rely on: the feature gap max |fwd_dense - fwd_dense_off| >= 0.4, and HF's OWN bf16 run of the same
wrapped model against its fp32 run inside the bf16 bounds the GPU test applies to the engine (logprobs 0.08 / 0.015, loss 1 %, gradient
ratios recorded max / median) - a scale at which HF itself is outside them would make those tests measure the fixture, not the engine.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_lora.py [case ...]"""
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
import test_lora_fixture as lx
from oracle import model_oracle as mo

import dense                                                     # the reference's

GOLD = os.path.join(ROOT, "tests", "golden")
RECORDED = json.load(open(os.path.join(GOLD, "recorded_bf16_table.json")))
loss_fn = lambda lp, ent, a: a["w_logprobs"] * lp.mean() + a["w_entropy"] * ent.mean()


def run(model, seqs):
    model.zero_grad()
    fwd = [x.detach().float().clone() for x in dense.forward(model, list(seqs), use_tqdm=False)]
    loss = dense.backward(model, list(seqs), fx.att(len(seqs)), loss_fn, act_ckpt=False, use_tqdm=False)
    return fwd, float(loss), {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


def make(case):
    seqs = [torch.tensor(s, dtype=torch.long) for s in lx.seqs_of(case)]
    model = lx.wrap_ref(case, lx.base_model(case))
    fwd, loss, grads = run(model, seqs)
    assert all(p.grad is None for p in model.parameters() if not p.requires_grad)
    off = lx.wrap_ref(case, lx.base_model(case), off=True)
    for p in off.parameters():                                   # with the adapters disabled nothing trainable is left: the loss needs a graph
        p.requires_grad_(True)
    fwd_off, loss_off, _ = run(off, seqs)
    gap = max(float((a - b).abs().max()) for a, b in zip(fwd, fwd_off))
    fwd16, loss16, grads16 = run(lx.wrap_ref(case, lx.base_model(case)).to(torch.bfloat16), seqs)
    err = torch.cat([(a - b).abs() for a, b in zip(fwd16, fwd)])
    ratios = {n: mo.grad_ratio(grads[n], grads16[n]) for n in grads}
    rmax, rmed = max(ratios.values()), float(np.median(list(ratios.values())))
    print(f"{case}: {len(grads)} adapter tensors, max len {max(map(len, seqs))}, loss {loss:.6f} (adapters off {loss_off:.6f}), gap {gap:.3f} "
          f"(>= {lx.MIN_GAP}); HF bf16 vs fp32: logprob err max {float(err.max()):.4f} / mean {float(err.mean()):.4f} (bounds 0.08 / 0.015), "
          f"loss rel {abs(loss16 - loss) / abs(loss):.2e} (1e-2), grad ratio max {rmax:.4f} ({RECORDED['max']:.4f}) median {rmed:.4f} "
          f"({RECORDED['median']:.4f})")
    assert gap >= lx.MIN_GAP, (case, gap)
    assert float(err.max()) < 0.08 and float(err.mean()) < 0.015 and abs(loss16 - loss) < 1e-2 * abs(loss), case
    assert rmax <= RECORDED["max"] and rmed <= 0.9 * RECORDED["median"], (case, rmax, rmed)     # 10 % clear of the median bound
    packed = {n: ((g / g.abs().max()).half(), float(g.abs().max())) for n, g in grads.items()}
    return {"fwd_dense": fwd, "fwd_dense_off": fwd_off, "bwd_dense_loss": loss, "bwd_dense_loss_off": loss_off,
            "bwd_dense_grads_fp16_scaled": packed, "grad_norms": {n: float(g.norm()) for n, g in grads.items()}, "ab_std": lx.AB_STD}


if __name__ == "__main__":
    path = os.path.join(GOLD, "engine_lora.pt")
    what = sys.argv[1:] or list(lx.CASES)
    content = torch.load(path, weights_only=True) if os.path.exists(path) and sys.argv[1:] else {}
    for case in what:
        content[case] = make(case)
    torch.save(content, path)
    print("engine_lora.pt", os.path.getsize(path), "bytes")
