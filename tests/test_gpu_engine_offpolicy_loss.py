"""GPU, end to end: TreeTrainingEngine.backward with a losses.PolicyLoss that carries an off-policy correction or the CISPO surrogate,
on the tiny model and the trie of test_gpu_engine_seq_policy_loss.py (folded sequences: a proper prefix ending exactly at a fork, a
duplicate; filler rows), per-token masks, a KL term and an entropy bonus - (a) the object itself (the fused path, dta_policy_loss),
(b) the same object behind a lambda (the callback path): the loss and every parameter gradient agree within that file's tolerances
for the dtype.  The statistics have the eight entries of losses.OFFPOLICY_STATS under a correction or CISPO and the six of losses.STATS
with the defaults.  rollout_logprobs sit a few hundredths of a nat off old_logprobs, plus a drift per sequence and a handful of outliers
that the cap truncates or the mask drops; in the cases without old_logprobs the kernel forms the weight from the rows' own log-probs."""
import json
import os

import numpy as np
import pytest
import torch

import cases
from dynamictreeattn_amd.losses import OFFPOLICY_STATS, STATS, PolicyLoss
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine, _PackedTrie
from oracle import model_oracle as mo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BOUND = {torch.bfloat16: json.load(open(os.path.join(GOLD, "recorded_bf16_table.json")))["max"], torch.float32: 1e-4}
LOSS_TOL = {torch.bfloat16: lambda c: 1e-2 * abs(c), torch.float32: lambda c: 1e-5 * max(abs(c), 1.0)}
CFG = cases.TINY_CFGS["d128"]
BASE = dict(clip_low=0.2, clip_high=0.2, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01)
LOSSES = {
    "token_truncate_no_old": (PolicyLoss(**BASE, is_level="token", is_cap=2.0), False),
    "sequence_mask": (PolicyLoss(**BASE, is_level="sequence_mean", is_mode="mask", is_cap=1.5, is_floor=0.7), True),
    "sequence_mask_no_old": (PolicyLoss(**BASE, is_level="sequence", is_mode="mask", is_cap=20.0, is_floor=0.05), False),
    "gspo_token_truncate": (PolicyLoss(**BASE, ratio="sequence", is_level="token", is_cap=2.0), True),
    "cispo": (PolicyLoss(**BASE, surrogate="cispo"), True),
}
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
        # the sampler's log-probs: 0.03 nats of noise around old, one token in 16 an outlier of +-1.2 nats, and a drift per sequence
        # of -0.5, 0, 0.1 or 0.55 nats, which puts the mean weight of half the sequences outside [0.7, 1.5] by 0.13 nats or more
        y = torch.from_numpy(rng.uniform(-0.03, 0.03, n) + np.where(rng.random(n) < 1 / 16, rng.choice([-1.2, 1.2], n), 0.0))
        y += (-0.5, 0.0, 0.1, 0.55)[i % 4]
        old = lp - x.float()
        atts.append({"advantages": torch.from_numpy(rng.normal(0.2, 0.8, n)).float(), "old_logprobs": old,
                     "ref_logprobs": lp + torch.from_numpy(rng.uniform(-0.3, 0.3, n)).float(), "loss_mask": mask,
                     "rollout_logprobs": old - y.float()})
    return seqs, tens, w, atts


def _attachments(setup, with_old):
    """fresh attachment dicts; without old_logprobs the former old log-probs stand for the sampler's: y = lp - rollout, formed from the
    rows' own log-probs, spreads 0.5 nats around the sequence's step (a sequence's product of weights is near 1 for step 0 only)"""
    out = []
    for a in setup[3]:
        a = dict(a)
        if not with_old:
            a["rollout_logprobs"] = a.pop("old_logprobs")
        out.append(a)
    return out


def _engine_run(setup, dtype, loss_fn, with_old):
    seqs, tens, w, _ = setup
    m = Qwen3TreeLM.from_named(CFG, w, DEV, dtype)
    t = TokenTrie(tens, _attachments(setup, with_old), device=DEV); t.backward_permute()
    e = TreeTrainingEngine(m.config, DEV, dtype, 256); e.mode = "packed"
    loss = e.backward(m, t, loss_fn, 2048)
    return e, loss, {n: p.grad.float().cpu() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(LOSSES))
def test_fused_and_callback_agree(setup, name, dtype):
    loss, with_old = LOSSES[name]
    ea, loss_a, grads_a = _engine_run(setup, dtype, loss, with_old)
    stats = ea.loss_stats.cpu()
    eb, loss_b, grads_b = _engine_run(setup, dtype, lambda *a: loss(*a), with_old)
    assert ea.last_loss_path == "fused" and eb.last_loss_path == "callback" and eb.loss_stats is None
    T = ea.last_packed.plan.T
    assert T >= _PackedTrie.PAD_FROM and T > ea.last_packed.n_real_tokens
    print(f"{name} {dtype}: loss fused {loss_a!r} callback {loss_b!r}")
    assert np.isfinite(loss_a) and abs(loss_a - loss_b) <= LOSS_TOL[dtype](loss_b), (loss_a, loss_b)
    ratios = {n: mo.grad_ratio(grads_b[n], grads_a[n]) for n in grads_b}
    worst = max(ratios.items(), key=lambda kv: kv[1])
    print(f"{name} {dtype}: worst grad_ratio fused against callback {worst}")
    assert worst[1] <= BOUND[dtype], worst
    assert any(float(g.abs().max()) > 0 for g in grads_a.values())
    n_masked = float(sum(int(a["loss_mask"].sum()) for a in setup[3]))
    assert stats.shape == (len(OFFPOLICY_STATS),) == (8,) and float(stats[0]) == loss_a and float(stats[5]) == n_masked
    if loss.is_level is not None:
        assert 0 < float(stats[7]) < n_masked and 0 < float(stats[6])       # some weights were truncated / dropped, not all
    else:
        assert float(stats[6]) == n_masked and float(stats[7]) == 0


def test_the_default_object_keeps_its_six_statistics_and_the_correction_changes_the_loss(setup):
    plain = PolicyLoss(**BASE)
    e, loss_p, _ = _engine_run(setup, torch.float32, plain, True)
    assert e.last_loss_path == "fused" and e.loss_stats.shape == (len(STATS),) == (6,)
    _, loss_w, _ = _engine_run(setup, torch.float32, LOSSES["sequence_mask"][0], True)
    _, loss_c, _ = _engine_run(setup, torch.float32, LOSSES["cispo"][0], True)
    assert abs(loss_w - loss_p) > 1e-3 * abs(loss_p) and abs(loss_c - loss_p) > 1e-3 * abs(loss_p)


def test_a_missing_rollout_key_is_an_error_on_the_fused_path(setup):
    seqs, tens, w, atts = setup
    m = Qwen3TreeLM.from_named(CFG, w, DEV, torch.float32)
    bare = [{k: v for k, v in a.items() if k != "rollout_logprobs"} for a in atts]
    t = TokenTrie(tens, bare, device=DEV); t.backward_permute()
    e = TreeTrainingEngine(m.config, DEV, torch.float32, 256); e.mode = "packed"
    with pytest.raises(KeyError, match="rollout_logprobs"):
        e.backward(m, t, LOSSES["token_truncate_no_old"][0], 2048)
