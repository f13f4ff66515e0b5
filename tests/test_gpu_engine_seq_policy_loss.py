"""GPU, end to end: TreeTrainingEngine.backward with a losses.PolicyLoss(ratio="sequence") - GSPO - on a tiny model, in bf16 and in
fp32, on the trie of test_gpu_engine_policy_loss.py (folded sequences: a proper prefix ending exactly at a fork, a duplicate; filler
rows), per-token masks, a KL term and an entropy bonus - (a) the object itself (the fused path, dta_policy_loss), (b) the same object
behind a lambda (the callback path), (c) the CPU oracle's restatement of the reference schedule in fp32 with the same object as its
loss_fn.  Bounds: that file's own - the existing engine tests' for the dtype, and the fused path no worse than the callback path by more
than 5 % + 1e-6.  old_logprobs are rebuilt so that every sequence's masked mean log-ratio is one of -0.6, -0.05, 0, 0.05, 0.6: the
sequence ratios stay on their side of the clip edges in bf16 as well."""
import json
import os

import numpy as np
import pytest
import torch

import cases
from dynamictreeattn_amd.losses import PolicyLoss, STATS
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine, _PackedTrie
from oracle import model_oracle as mo
from oracle import trie_oracle as to

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BOUND = {torch.bfloat16: json.load(open(os.path.join(GOLD, "recorded_bf16_table.json")))["max"], torch.float32: 1e-4}
LOSS_TOL = {torch.bfloat16: lambda c: 1e-2 * abs(c), torch.float32: lambda c: 1e-5 * max(abs(c), 1.0)}
CFG = cases.TINY_CFGS["d128"]
LOSS = PolicyLoss(clip_low=0.2, clip_high=0.2, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01, ratio="sequence")
STEPS = (-0.6, -0.05, 0.0, 0.05, 0.6)


def _sequences():
    """14 rollouts in 3 groups behind a 40-token prompt, 130-170 tokens each, + a proper prefix of group 0 that ends exactly at the
    group's fork + a duplicate: more than 2048 tree tokens, not a multiple of 256."""
    rng = np.random.default_rng(4)
    prompt = rng.integers(0, 512, 40).tolist()
    groups = [prompt + rng.integers(0, 512, 30).tolist() for _ in range(3)]
    seqs = [groups[i % 3] + rng.integers(0, 512, 130 + 3 * i).tolist() for i in range(14)]
    seqs.append(list(groups[0]))
    seqs.append(list(seqs[3]))
    return seqs


@pytest.fixture(scope="module")
def setup():
    seqs = _sequences()
    w = mo.init_weights(CFG, seed=3)
    m32 = Qwen3TreeLM.from_named(CFG, w, DEV, torch.float32)
    tens = [torch.tensor(s, dtype=torch.int64) for s in seqs]
    base = [t.cpu() for t in TreeTrainingEngine(m32.config, DEV, torch.float32, 256, forward_only=True).forward(m32, TokenTrie(tens, device=DEV))]
    rng = np.random.default_rng(8)
    atts = []
    for i, lp in enumerate(base):
        n = lp.shape[0]
        mask = torch.from_numpy(rng.random(n) < 0.8)
        if i == 5:
            mask[:] = False
        x = torch.from_numpy(rng.uniform(-0.5, 0.5, n))          # per-token log-ratios spread around the sequence's step
        if mask.any():
            x[mask] += STEPS[i % len(STEPS)] - x[mask].mean()
        atts.append({"advantages": torch.from_numpy(rng.normal(0.2, 0.8, n)).float(), "old_logprobs": lp - x.float(),
                     "ref_logprobs": lp + torch.from_numpy(rng.uniform(-0.3, 0.3, n)).float(), "loss_mask": mask})
    fresh = lambda: [dict(a) for a in atts]
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    o = to.TokenTrieOracle([np.asarray(s, dtype=np.int64) for s in seqs], fresh()); o.backward_permute()
    loss_c = float(mo.StackEngineOracle(CFG, wo, 256).backward(o, LOSS, 2048))
    grads_c = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in wo.items()}
    n_masked = float(sum(int(a["loss_mask"].sum()) for a in atts))
    return seqs, tens, w, fresh, loss_c, grads_c, n_masked


def _engine_run(setup, dtype, loss_fn):
    seqs, tens, w, fresh, _, _, _ = setup
    m = Qwen3TreeLM.from_named(CFG, w, DEV, dtype)
    t = TokenTrie(tens, fresh(), device=DEV); t.backward_permute()
    e = TreeTrainingEngine(m.config, DEV, dtype, 256); e.mode = "packed"
    loss = e.backward(m, t, loss_fn, 2048)
    return e, loss, {n: p.grad.float().cpu() for n, p in m.named_parameters()}


def _ratios(setup, grads):
    return {n: mo.grad_ratio(setup[5][n], g) for n, g in grads.items()}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fused_callback_and_oracle_agree(setup, dtype):
    loss_c, n_masked = setup[4], setup[6]
    ea, loss_a, grads_a = _engine_run(setup, dtype, LOSS)
    stats = ea.loss_stats.cpu()
    eb, loss_b, grads_b = _engine_run(setup, dtype, lambda a, e, att: LOSS(a, e, att))
    assert ea.last_loss_path == "fused" and eb.last_loss_path == "callback" and eb.loss_stats is None
    T = ea.last_packed.plan.T
    assert T >= _PackedTrie.PAD_FROM and T > ea.last_packed.n_real_tokens and any(len(a) > 1 for a in TokenTrie(setup[1], device=DEV).attach_lists)
    print(f"{dtype}: loss fused {loss_a!r} callback {loss_b!r} oracle {loss_c!r}")
    assert abs(loss_a - loss_c) <= LOSS_TOL[dtype](loss_c), (loss_a, loss_c)
    assert abs(loss_b - loss_c) <= LOSS_TOL[dtype](loss_c), (loss_b, loss_c)
    ra, rb = _ratios(setup, grads_a), _ratios(setup, grads_b)
    worst_b = max(rb.items(), key=lambda kv: kv[1])
    print(f"{dtype}: worst grad_ratio callback {worst_b}, fused {max(ra.items(), key=lambda kv: kv[1])}")
    assert worst_b[1] <= BOUND[dtype], worst_b
    for n in ra:
        assert ra[n] <= 1.05 * rb[n] + 1e-6, (n, ra[n], rb[n])
    assert stats.shape == (len(STATS),) and float(stats[0]) == loss_a
    assert float(stats[5]) == n_masked
    assert 0 < float(stats[4]) < n_masked and float(stats[2]) > 0 and float(stats[3]) > 0


def test_the_objective_differs_from_the_token_level_one(setup):
    """The same attachments under ratio="token" give another loss: the engine really dispatched on the ratio."""
    token = PolicyLoss(clip_low=0.2, clip_high=0.2, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01)
    _, loss_t, _ = _engine_run(setup, torch.float32, token)
    assert abs(loss_t - setup[4]) > 1e-3 * abs(setup[4])
