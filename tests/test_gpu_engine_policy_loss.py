"""GPU, end to end: TreeTrainingEngine.backward with a losses.PolicyLoss on a tiny model, in bf16 and in fp32, on a trie with folded
sequences (a proper prefix ending exactly at a fork, a duplicate) and filler rows, per-token masks, a KL term and an entropy bonus -
(a) the object itself (the fused path), (b) the same object behind a lambda (the callback path), (c) the CPU oracle's restatement of the
reference schedule in fp32 with the same object as its loss_fn.  Bounds: the ones the existing engine tests use for the dtype (bf16:
the reference's recorded bound and 1e-2 on the loss, test_gpu_engine.py; fp32: 1e-4 per parameter and 1e-5 on the loss,
test_gpu_properties.py); the fused path may be no worse than the callback path by more than 5 % + 1e-6 - the two differ in the fp32
summation order of dlp / dent in front of an identical backward."""
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
LOSS = PolicyLoss(clip_low=0.2, clip_high=0.2, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01)


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
    steps = np.array([-0.6, -0.05, 0.0, 0.05, 0.6])          # ratios well away from the clip edges: a bf16 model's log-probs keep their branch
    atts = []
    for i, lp in enumerate(base):
        n = lp.shape[0]
        mask = torch.from_numpy(rng.random(n) < 0.8)
        if i == 5:
            mask[:] = False
        atts.append({"advantages": torch.from_numpy(rng.normal(0.7, 0.5, n)).float(), "old_logprobs": lp + torch.from_numpy(rng.choice(steps, n)).float(),
                     "ref_logprobs": lp + torch.from_numpy(rng.uniform(-0.3, 0.3, n)).float(), "loss_mask": mask})
    fresh = lambda: [dict(a) for a in atts]
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    o = to.TokenTrieOracle([np.asarray(s, dtype=np.int64) for s in seqs], fresh()); o.backward_permute()
    loss_c = float(mo.StackEngineOracle(CFG, wo, 256).backward(o, LOSS, 2048))
    grads_c = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in wo.items()}
    n_masked = float(sum(int(a["loss_mask"].sum()) for a in atts))
    return seqs, tens, w, fresh, loss_c, grads_c, n_masked


def _engine_run(setup, dtype, loss_fn, mode="packed"):
    seqs, tens, w, fresh, _, _, _ = setup
    m = Qwen3TreeLM.from_named(CFG, w, DEV, dtype)
    t = TokenTrie(tens, fresh(), device=DEV); t.backward_permute()
    e = TreeTrainingEngine(m.config, DEV, dtype, 256); e.mode = mode
    if mode == "stack":
        e._stack_block_rows = lambda *a: 512
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


def test_stack_mode_takes_the_callback_path(setup):
    e, loss, grads = _engine_run(setup, torch.float32, LOSS, mode="stack")
    assert e.last_loss_path == "callback" and e.loss_stats is None and e.last_mode.startswith("stack")
    assert abs(loss - setup[4]) <= LOSS_TOL[torch.float32](setup[4]), (loss, setup[4])
    worst = max(_ratios(setup, grads).items(), key=lambda kv: kv[1])
    assert worst[1] <= BOUND[torch.float32], worst


def test_no_entropy_bonus_and_on_policy(setup):
    """entropy_coef == 0: the entropy is no root of the backward; old_logprobs absent: ratio 1.  Fused against callback, fp32."""
    seqs, tens, w, fresh, _, _, _ = setup
    loss = PolicyLoss(agg="token_sum", scale=1e-3)
    out = []
    for fn in (loss, lambda a, e, att: loss(a, e, att)):
        m = Qwen3TreeLM.from_named(CFG, w, DEV, torch.float32)
        atts = [{"advantages": float(0.3 + 0.1 * i), "loss_mask": a["loss_mask"]} for i, a in enumerate(fresh())]
        t = TokenTrie(tens, atts, device=DEV)
        e = TreeTrainingEngine(m.config, DEV, torch.float32, 256); e.mode = "packed"
        out.append((e.backward(m, t, fn, 2048), {n: p.grad.float().cpu() for n, p in m.named_parameters()}, e.last_loss_path))
    assert out[0][2] == "fused" and out[1][2] == "callback"
    assert abs(out[0][0] - out[1][0]) <= 1e-5 * max(abs(out[1][0]), 1.0)
    for n, g in out[1][1].items():
        assert mo.grad_ratio(g, out[0][1][n]) <= 1e-4, n
