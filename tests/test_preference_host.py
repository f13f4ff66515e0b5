"""Host side of the preference objectives (no GPU): packing.preference_pair_tables - order, duplicates within one leaf, every refusal
naming the pair id -, the constructor's refusals, the TypeError of calling the object per sequence, dp.rejoin_pairs, and
losses.two_pass_backward on the CPU oracle engine against autograd of PreferenceLoss.total - the definition, evaluated in float64 -
through dense_backward-style per-sequence graphs."""
import numpy as np
import pytest
import torch

import cases
from dynamictreeattn_amd import dp, losses, packing
from dynamictreeattn_amd.losses import PreferenceLoss, two_pass_backward
from oracle import model_oracle as mo
from oracle import trie_oracle as to


def _lists(leaves):
    """per-leaf [(pair_id, chosen), ...] -> attach lists"""
    return [[({"pair_id": pid, "chosen": ch}, 5) for pid, ch in leaf] for leaf in leaves]


def test_pair_tables_are_in_callback_order_sorted_by_the_chosen_member():
    c, r = packing.preference_pair_tables(_lists([[("b", False), ("a", True)], [("c", True)], [("a", False), ("c", False), ("b", True)]]))
    assert c.dtype == r.dtype == np.int32
    assert c.tolist() == [1, 2, 5] and r.tolist() == [3, 4, 0]
    # the two members of a pair may be the same string: two entries of one leaf's attach list
    c, r = packing.preference_pair_tables(_lists([[(7, False), (7, True)]]))
    assert c.tolist() == [1] and r.tolist() == [0]
    c, r = packing.preference_pair_tables([])
    assert c.shape == r.shape == (0,)


@pytest.mark.parametrize("leaves,word", [
    ([[("a", True), ("a", False)], [("orphan", True)]], "orphan"),                       # half a pair
    ([[("a", True), ("a", False)], [("lost", False)]], "lost"),
    ([[("x", True)], [("x", False), ("x", False)]], "x"),                                # seen three times
    ([[("two", True)], [("two", True)]], "two"),                                         # two chosen members
    ([[(("p", 3), False), (("p", 3), False)]], "('p', 3)"),                              # two rejected members
])
def test_pair_table_refusals_name_the_pair(leaves, word):
    with pytest.raises(ValueError) as e:
        packing.preference_pair_tables(_lists(leaves))
    assert repr(word) in str(e.value) or word in str(e.value)
    assert "pair_id" in str(e.value)


def test_a_missing_key_is_named():
    for key in ("pair_id", "chosen"):
        att = {"pair_id": 1, "chosen": True}
        del att[key]
        with pytest.raises(KeyError, match=key):
            packing.preference_pair_tables([[(att, 4)]])


@pytest.mark.parametrize("kw,name", [
    (dict(beta=0.0), "beta"), (dict(beta=-1.0), "beta"), (dict(beta=float("nan")), "beta"), (dict(beta=float("inf")), "beta"),
    (dict(label_smoothing=-0.1), "label_smoothing"), (dict(label_smoothing=0.5), "label_smoothing"),
    (dict(label_smoothing=0.1, kind="hinge"), "label_smoothing"), (dict(label_smoothing=0.1, kind="ipo"), "label_smoothing"),
    (dict(label_smoothing=float("nan")), "label_smoothing"), (dict(gamma=0.5, kind="ipo"), "gamma"), (dict(gamma=float("inf")), "gamma"),
    (dict(sft_coef=-1e-3), "sft_coef"), (dict(sft_coef=float("nan")), "sft_coef"), (dict(scale=float("nan")), "scale"),
    (dict(scale=float("-inf")), "scale"), (dict(kind="dpo"), "kind"),
])
def test_the_constructor_refuses_and_names_the_argument(kw, name):
    with pytest.raises(ValueError, match=name):
        PreferenceLoss(**kw)


def test_the_limits_are_accepted():
    loss = PreferenceLoss(beta=1e-6, kind="sigmoid", label_smoothing=0.49, gamma=-2.0, length_normalize=True, reference_free=True, sft_coef=0.0,
                          scale=-1.0)
    assert "label_smoothing=0.49" in repr(loss) and loss.kind == "sigmoid"
    PreferenceLoss(kind="hinge", gamma=3.0); PreferenceLoss(kind="ipo", sft_coef=2.0)
    assert losses.PREFERENCE_KINDS == ("sigmoid", "hinge", "ipo")
    assert losses.PREFERENCE_STATS == ("loss", "sum_pair_loss", "sum_sft", "reward_margin", "chosen_reward", "rejected_reward", "correct_pairs", "pairs")
    assert {"PreferenceLoss", "PREFERENCE_KINDS", "PREFERENCE_STATS", "two_pass_backward"} <= set(losses.__all__)


def test_calling_the_object_per_sequence_is_a_type_error():
    with pytest.raises(TypeError) as e:
        PreferenceLoss()(torch.zeros(3), torch.zeros(4), {"pair_id": 0, "chosen": True})
    assert "couples" in str(e.value) and "engine.backward" in str(e.value)


def test_the_reference_forms_are_checked():
    loss = PreferenceLoss()
    lps = [torch.zeros(3), torch.zeros(3)]
    att = lambda **kw: [dict(pair_id=0, chosen=True, **kw), dict(pair_id=0, chosen=False, **kw)]
    with pytest.raises(KeyError, match="ref_logprob"):
        loss.total(lps, att())
    with pytest.raises(ValueError, match="both"):
        loss.total(lps, att(ref_logprobs=torch.zeros(3), ref_logprob_sum=0.0))
    with pytest.raises(ValueError, match="ref_logprobs"):
        loss.total(lps, att(ref_logprobs=torch.zeros(4)))
    with pytest.raises(ValueError, match="loss_mask"):
        loss.total(lps, att(ref_logprob_sum=1.0, loss_mask=torch.ones(2)))
    mixed = att(ref_logprob_sum=1.0)
    mixed[1] = dict(pair_id=0, chosen=False, ref_logprobs=torch.zeros(3))
    with pytest.raises(ValueError, match="one form"):
        loss.total(lps, mixed)
    assert float(PreferenceLoss(reference_free=True).total(lps, att())) == pytest.approx(np.log(2.0))       # neither form is read


def test_rejoin_pairs_keeps_every_sequence_once_and_every_pair_in_one_bin():
    rng = np.random.default_rng(0)
    n = 40
    pair_ids = [i // 2 for i in range(n)]
    pair_ids[36:] = [None] * 4                                           # sequences outside any pair stay where they are
    order = rng.permutation(n).tolist()
    bins = [order[0:9], order[9:23], [], order[23:40]]
    split = sum(1 for q in range(18) if len({k for k, b in enumerate(bins) for i in b if pair_ids[i] == q}) > 1)
    assert split > 0                                                     # the balancer did split pairs
    out = dp.rejoin_pairs(bins, pair_ids)
    assert len(out) == len(bins) and sorted(i for b in out for i in b) == list(range(n))
    where = {i: k for k, b in enumerate(out) for i in b}
    assert all(where[2 * q] == where[2 * q + 1] for q in range(18))
    before = {i: k for k, b in enumerate(bins) for i in b}
    assert all(where[i] == before[i] for i in range(36, 40))
    assert all(where[2 * q] in (before[2 * q], before[2 * q + 1]) for q in range(18))
    assert bins[2] == [] and dp.rejoin_pairs(out, pair_ids) == out      # the input is not changed; whole pairs: nothing moves
    # with the chosen flags the rejected member moves to its chosen member's bin
    chosen = [i % 2 == (i // 2) % 2 for i in range(n)]
    out = dp.rejoin_pairs(bins, pair_ids, chosen)
    where = {i: k for k, b in enumerate(out) for i in b}
    assert sorted(i for b in out for i in b) == list(range(n))
    assert all(where[i] == before[i] for i in range(n) if pair_ids[i] is None or chosen[i])
    assert all(where[2 * q] == where[2 * q + 1] for q in range(18))


class _OracleEngine:
    def __init__(self, cfg):
        self.cfg = cfg

    def forward(self, w, trie):
        return mo.StackEngineOracle(self.cfg, w, 64).forward(trie)

    def backward(self, w, trie, loss_fn, block_size):
        return mo.StackEngineOracle(self.cfg, w, 64).backward(trie, loss_fn, block_size)


@pytest.mark.parametrize("loss", [PreferenceLoss(beta=0.5, label_smoothing=0.1, sft_coef=0.2),
                                  PreferenceLoss(beta=0.5, kind="hinge", length_normalize=True, scale=0.5),
                                  PreferenceLoss(beta=0.25, kind="ipo", length_normalize=True),
                                  PreferenceLoss(beta=2.0, gamma=0.3, length_normalize=True, reference_free=True)], ids=lambda l: l.kind)
def test_two_pass_backward_on_the_cpu_oracle_against_autograd_of_the_definition(loss):
    cfg = cases.TINY_CFGS["d16"]
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, 512, 6).tolist()
    seqs = [prompt + rng.integers(0, 512, 5 + i).tolist() for i in range(6)]
    seqs += [list(seqs[2]), seqs[0][:8]]                                # a duplicate string (pair 3 with its twin) and a proper prefix
    pairs = [(0, 1), (3, 7), (4, 5), (2, 6)]
    w = mo.init_weights(cfg, seed=1)
    atts = []
    for i, s in enumerate(seqs):
        n = len(s) - 1
        mask = torch.from_numpy(rng.random(n) < 0.8)
        mask[:5] = False
        mask[-1] = True
        atts.append({"loss_mask": mask, "ref_logprobs": torch.from_numpy(-rng.uniform(5.5, 7.0, n)).float()})
    for q, (c, r) in enumerate(pairs):
        atts[c].update(pair_id=q, chosen=True); atts[r].update(pair_id=q, chosen=False)
    # the definition: per-sequence graphs as dense_backward builds them, the objective over all of them at once, in float64
    wd = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    lps = []
    for s in seqs:
        s = torch.as_tensor(s)
        logits, _, _ = mo.qwen3_segment(cfg, wd, s, 0)
        lps.append(mo.logprobs_of(logits, s[1:]).double())
    total = loss.total(lps, atts)
    total.backward()
    # two passes over the oracle's stack engine
    wo = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    o = to.TokenTrieOracle([np.asarray(s, dtype=np.int64) for s in seqs], [dict(a) for a in atts]); o.backward_permute()
    value, stats = two_pass_backward(_OracleEngine(cfg), wo, o, loss, 2048)
    assert abs(value - float(total.detach())) <= 1e-5 * max(abs(float(total.detach())), 1.0)
    assert stats.shape == (8,) and float(stats[7]) == 4 and float(stats[0]) == pytest.approx(value)
    for k in wd:
        assert wd[k].grad is not None and float(wd[k].grad.abs().max()) > 0
        assert mo.grad_ratio(wd[k].grad, wo[k].grad) <= 1e-5, (k, mo.grad_ratio(wd[k].grad, wo[k].grad))
