#!/usr/bin/env python3
"""Generate tests/golden/engine_cohere.pt by IMPORTING THE REFERENCE (build container only): the reference's dense per-sequence
path (dense.py) over the unmodified transformers CohereForCausalLM / Cohere2ForCausalLM models of tests/test_cohere_fixture.py, fp32 on
the CPU with eager attention - the protocol of scripts/make_golden_phi_glm.py.  Every record: fwd_dense; fwd_dense_off_* (the sequences' logprobs
concatenated, of the same weights with ONE feature removed: the logit scale and the window by configuration; the mean subtraction of the norm, the interleaved
pairing and the table-less full layers by a patch of the running HF model - test_cohere_fixture.hf_run_with); the dense backward's loss
and every gradient (fp16 of g / max|g| and the scale); gradient norms.

It also measures what the fixture tests rely on and prints it: each feature gap max |fwd_dense - fwd_dense_off_*| (must be >= 0.4) and
HF's OWN bf16 run against its fp32 run (forward logprob error, loss, per-parameter gradient ratios) next to the bf16 bounds the GPU
tests apply (family.check_bf16_against_fixture) - a scale at which HF itself is outside them would make those tests measure the
fixture, not the engine.  The weight scale and seeds in test_cohere_fixture are draws for which HF's own bf16 run sits inside every one of
those bounds; the script asserts it, on the CPU.  `--seeds CASE FIRST LAST` prints the same figures for a range of seeds instead of
writing anything.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_cohere.py"""
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
import test_cohere_fixture as fx
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


def hf_bf16_figures(case, seqs, fwd, loss, grads):
    """HF's own bf16 run against its fp32 run: (logprob err max, mean, loss rel, gradient ratio max, median)."""
    fwd16, loss16, grads16 = run(fx.hf_model(case).to(torch.bfloat16), seqs)
    err = torch.cat([(a - b).abs() for a, b in zip(fwd16, fwd)])
    ratios = [mo.grad_ratio(grads[n], grads16[n]) for n in grads]
    return float(err.max()), float(err.mean()), abs(loss16 - loss) / abs(loss), max(ratios), float(np.median(ratios))


def inside(fig):
    return fig[0] < 0.08 and fig[1] < 0.015 and fig[2] < 1e-2 and fig[3] <= RECORDED["max"] and fig[4] <= RECORDED["median"]


def make(case):
    seqs = [torch.tensor(s, dtype=torch.long) for s in fx.seqs_of(case)]
    fwd, loss, grads = run(fx.hf_model(case), seqs)
    rec = {"fwd_dense": fwd, "bwd_dense_loss": loss, "std": fx.CASE_STD[case], "embed_offset": fx.EMBED_OFFSET}
    gaps = {}
    for off in fx.offs_of(case):
        model = fx.hf_model(case, off)
        with fx.hf_run_with(off, model):
            rec["fwd_dense_off_" + off] = torch.cat(run(model, seqs, backward=False)[0])      # one tensor per record: the file stays under 1 MiB
        gaps[off] = float((torch.cat(fwd) - rec["fwd_dense_off_" + off]).abs().max())
    fig = hf_bf16_figures(case, seqs, fwd, loss, grads)
    print(f"{case}: {len(seqs)} sequences, len {min(map(len, seqs))}..{max(map(len, seqs))}, loss {loss:.6f}, gaps "
          + ", ".join(f"{k} {v:.3f}" for k, v in gaps.items()) + f" (>= {fx.MIN_GAP}); "
          f"HF bf16 vs fp32: logprob err max {fig[0]:.4f} / mean {fig[1]:.4f} (bounds 0.08 / 0.015), "
          f"loss rel {fig[2]:.2e} (1e-2), grad ratio max {fig[3]:.4f} ({RECORDED['max']:.4f}) median {fig[4]:.4f} ({RECORDED['median']:.4f})")
    assert all(g >= fx.MIN_GAP for g in gaps.values()), (case, gaps)
    assert inside(fig), (case, "HF's own bf16 run is outside the bounds of the GPU tests: pick another weight seed", fig)
    rec["bwd_dense_grads_fp16_scaled"] = {n: ((g / g.abs().max()).half(), float(g.abs().max())) for n, g in grads.items()}
    rec["grad_norms"] = {n: float(g.norm()) for n, g in grads.items()}
    return rec


def try_seeds(case, first, last):
    seqs = [torch.tensor(s, dtype=torch.long) for s in fx.seqs_of(case)]
    entry = fx.CASES[case]
    for seed in range(first, last + 1):
        fx.CASES[case] = entry[:3] + (seed,)
        fwd, loss, grads = run(fx.hf_model(case), seqs)
        fig = hf_bf16_figures(case, seqs, fwd, loss, grads)
        gaps = {}
        for off in fx.offs_of(case):
            model = fx.hf_model(case, off)
            with fx.hf_run_with(off, model):
                gaps[off] = max(float((a - b).abs().max()) for a, b in zip(fwd, run(model, seqs, backward=False)[0]))
        print(f"{case} seed {seed}: {'inside ' if inside(fig) else 'OUTSIDE'} err {fig[0]:.4f} / {fig[1]:.4f}, loss {fig[2]:.2e}, "
              f"ratio max {fig[3]:.4f} median {fig[4]:.4f}; gaps " + ", ".join(f"{k} {v:.2f}" for k, v in gaps.items()), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--seeds":
        try_seeds(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        sys.exit(0)
    content = {case: make(case) for case in fx.CASES}
    torch.save(content, os.path.join(GOLD, fx.FILE))
    size = os.path.getsize(os.path.join(GOLD, fx.FILE))
    print(fx.FILE, size, "bytes")
    assert size < (1 << 20), "the fixture must stay under 1 MiB"
