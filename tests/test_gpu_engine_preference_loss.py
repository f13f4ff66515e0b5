"""GPU, end to end: TreeTrainingEngine.backward with a losses.PreferenceLoss on a tiny model, in bf16 and in fp32, on the 16-sequence
trie of test_gpu_engine_policy_loss.py (a proper prefix ending exactly at a fork, a duplicate; filler rows) paired into 8 pairs - the
duplicate string is one pair, the folded prefix a member of another - with masks that are zero over the 40-token prompt; kind
"sigmoid" (DPO with an SFT term) and kind "ipo" (length-normalised) - (a) the object itself (the fused path, dta_preference_loss), (b)
losses.two_pass_backward on the same engine (a forward, the coefficients, the callback path with the linear closure), (c) the CPU
oracle's two-pass in fp32.  Bounds: the existing engine tests' own for the dtype, and the fused path no worse than (b) by more than
5 % + 1e-6 per parameter.  One more case forces the block-wise walk, which takes the two-pass form by itself."""
import json
import os

import numpy as np
import pytest
import torch

import cases
from dynamictreeattn_amd.losses import PREFERENCE_STATS, PreferenceLoss, two_pass_backward
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
LOSSES = {"sigmoid": PreferenceLoss(beta=0.1, sft_coef=0.1, scale=1.0 / 8),
          "ipo": PreferenceLoss(beta=0.1, kind="ipo", length_normalize=True, scale=1.0 / 8)}
PROMPT = 40
# (chosen, rejected) by original sequence id: 3 / 15 are the same string, 14 is the proper prefix of group 0 that ends at its fork
PAIRS = [(3, 15), (0, 14), (4, 1), (7, 10), (5, 2), (8, 11), (9, 6), (12, 13)]


def _sequences():
    """the sequences of test_gpu_engine_policy_loss.py: 14 rollouts in 3 groups behind a 40-token prompt, 130-170 tokens each, + a
    proper prefix of group 0 that ends exactly at the group's fork + a duplicate: more than 2048 tree tokens, not a multiple of 256."""
    rng = np.random.default_rng(4)
    prompt = rng.integers(0, 512, PROMPT).tolist()
    groups = [prompt + rng.integers(0, 512, 30).tolist() for _ in range(3)]
    seqs = [groups[i % 3] + rng.integers(0, 512, 130 + 3 * i).tolist() for i in range(14)]
    seqs.append(list(groups[0]))
    seqs.append(list(seqs[3]))
    return seqs


class _OracleEngine:
    """the forward / backward surface of an engine over the CPU oracle (a fresh stack per pass), for two_pass_backward"""

    def forward(self, w, trie):
        return mo.StackEngineOracle(CFG, w, 256).forward(trie)

    def backward(self, w, trie, loss_fn, block_size):
        return mo.StackEngineOracle(CFG, w, 256).backward(trie, loss_fn, block_size)


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
        mask = torch.from_numpy(rng.random(n) < 0.9)
        mask[:PROMPT - 1] = False                                      # predictions of prompt tokens take no part
        atts.append({"ref_logprobs": lp + torch.from_numpy(rng.uniform(-0.3, 0.3, n)).float(), "loss_mask": mask})
    for q, (c, r) in enumerate(PAIRS):
        atts[c].update(pair_id=("pair", q), chosen=True); atts[r].update(pair_id=("pair", q), chosen=False)
    fresh = lambda: [dict(a) for a in atts]
    oracle = {}
    for kind, loss in LOSSES.items():
        wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
        o = to.TokenTrieOracle([np.asarray(s, dtype=np.int64) for s in seqs], fresh()); o.backward_permute()
        loss_c, _ = two_pass_backward(_OracleEngine(), wo, o, loss, 2048)
        oracle[kind] = (loss_c, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in wo.items()})
    return seqs, tens, w, fresh, oracle


def _engine_run(setup, dtype, loss, how, mode="packed"):
    seqs, tens, w, fresh, _ = setup
    m = Qwen3TreeLM.from_named(CFG, w, DEV, dtype)
    t = TokenTrie(tens, fresh(), device=DEV); t.backward_permute()
    e = TreeTrainingEngine(m.config, DEV, dtype, 256); e.mode = mode
    if mode == "stack":
        e._stack_block_rows = lambda *a: 512
    if how == "object":
        value, stats = e.backward(m, t, loss, 2048), e.loss_stats
    else:
        value, stats = two_pass_backward(e, m, t, loss, 2048)
    return e, value, stats.cpu(), {n: p.grad.float().cpu() for n, p in m.named_parameters()}


def _ratios(grads_c, grads):
    return {n: mo.grad_ratio(grads_c[n], g) for n, g in grads.items()}


@pytest.mark.parametrize("kind", list(LOSSES))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_fused_two_pass_and_oracle_agree(setup, dtype, kind):
    loss = LOSSES[kind]
    loss_c, grads_c = setup[4][kind]
    ea, loss_a, stats, grads_a = _engine_run(setup, dtype, loss, "object")
    eb, loss_b, stats_b, grads_b = _engine_run(setup, dtype, loss, "two_pass")
    assert ea.last_loss_path == "fused" and eb.last_loss_path == "callback" and eb.loss_stats is None
    T = ea.last_packed.plan.T
    assert T >= _PackedTrie.PAD_FROM and T > ea.last_packed.n_real_tokens and any(len(a) > 1 for a in TokenTrie(setup[1], device=DEV).attach_lists)
    print(f"{dtype} {kind}: loss fused {loss_a!r} two-pass {loss_b!r} oracle {loss_c!r}")
    assert abs(loss_a - loss_c) <= LOSS_TOL[dtype](loss_c), (loss_a, loss_c)
    assert abs(loss_b - loss_c) <= LOSS_TOL[dtype](loss_c), (loss_b, loss_c)
    ra, rb = _ratios(grads_c, grads_a), _ratios(grads_c, grads_b)
    worst_b = max(rb.items(), key=lambda kv: kv[1])
    print(f"{dtype} {kind}: worst grad_ratio two-pass {worst_b}, fused {max(ra.items(), key=lambda kv: kv[1])}")
    assert worst_b[1] <= BOUND[dtype], worst_b
    for n in ra:
        assert ra[n] <= 1.05 * rb[n] + 1e-6, (n, ra[n], rb[n])
    assert stats.shape == (len(PREFERENCE_STATS),) and float(stats[0]) == loss_a
    assert float(stats[7]) == 8 and 0 <= float(stats[6]) <= 8 and float(stats[6]) == int(stats[6])
    assert stats_b.shape == (len(PREFERENCE_STATS),) and float(stats_b[7]) == 8


def test_the_block_wise_walk_takes_the_two_pass_form(setup):
    loss = LOSSES["sigmoid"]
    loss_c, grads_c = setup[4]["sigmoid"]
    e, value, stats, grads = _engine_run(setup, torch.float32, loss, "object", mode="stack")
    assert e.last_loss_path == "two_pass" and e.last_mode.startswith("stack")
    assert stats.shape == (len(PREFERENCE_STATS),) and float(stats[7]) == 8 and abs(float(stats[0]) - value) <= 1e-6 * max(abs(value), 1.0)
    assert abs(value - loss_c) <= LOSS_TOL[torch.float32](loss_c), (value, loss_c)
    worst = max(_ratios(grads_c, grads).items(), key=lambda kv: kv[1])
    assert worst[1] <= BOUND[torch.float32], worst


def test_a_callback_that_calls_the_object_is_refused(setup):
    loss = LOSSES["sigmoid"]
    seqs, tens, w, fresh, _ = setup
    m = Qwen3TreeLM.from_named(CFG, w, DEV, torch.float32)
    t = TokenTrie(tens, fresh(), device=DEV)
    e = TreeTrainingEngine(m.config, DEV, torch.float32, 256); e.mode = "packed"
    with pytest.raises(TypeError, match="couples"):
        e.backward(m, t, lambda a, ent, att: loss(a, ent, att), 2048)
