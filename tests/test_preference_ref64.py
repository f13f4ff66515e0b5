"""The float64 closed form of preference_ref64 against float64 torch autograd of losses.PreferenceLoss.total - the definition - for
every kind, with and without length_normalize, reference_free, label_smoothing and sft_coef and in both forms of the reference, on
every trie of that module: the value, the per-sequence coefficients g_s, the statistics of PreferenceLoss.coefficients and the row
gradients summed over the trie.  And the properties the kernel tests lean on: the pairing, the distance of every pair from every
edge, the exact tie of the duplicate pair."""
import numpy as np
import pytest
import torch

import preference_ref64 as P
from dynamictreeattn_amd import losses, packing


def _torch_atts(atts):
    return [{k: (torch.from_numpy(np.asarray(v)) if isinstance(v, np.ndarray) else v) for k, v in a.items()} for a in atts]


# many_seqs is 2102 per-sequence autograd graphs: one configuration per kind there, every configuration on the other tries
@pytest.mark.parametrize("name,cfg", [(n, c) for n in P.TRIES for c in P.CONFIGS() if n != "many_seqs" or c in ("dpo", "slic_ln", "ipo_ln_sft")])
def test_closed_form_against_autograd(name, cfg):
    loss = P.CONFIGS()[cfg][0]
    plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts = P.make_inputs(name, cfg, seed=3)
    paths = P.paths_of(plan, att_lens)
    ref = P.closed_form(loss, [lp[rows[1:]] for rows in paths], atts, pair_c, pair_r, as_fp32=False)
    x = torch.from_numpy(lp.astype(np.float64)).requires_grad_(True)
    lps = [x[torch.from_numpy(rows[1:])] for rows in paths]
    tatts = _torch_atts(atts)
    total = loss.total(lps, tatts)
    total.backward()
    tol = lambda v: 1e-12 * max(1.0, float(np.abs(v).max()))
    assert abs(float(total.detach()) - ref["total"]) <= tol(ref["total"])
    dlp = np.zeros(plan.T)
    for s, (rows, a) in enumerate(zip(paths, atts)):
        np.add.at(dlp, rows[1:], ref["g"][s] * np.asarray(a["loss_mask"], np.float64))
    assert np.abs(x.grad.numpy() - dlp).max() <= tol(dlp)
    assert (dlp[n_real:] == 0).all()
    t2, g, stats = loss.coefficients([t.detach() for t in lps], tatts)
    assert abs(float(t2) - ref["total"]) <= tol(ref["total"])
    assert np.abs(g.numpy() - ref["g"]).max() <= tol(ref["g"])
    assert np.abs(stats.numpy() - ref["stats"]).max() <= tol(ref["stats"])
    assert tuple(P.STATS) == losses.PREFERENCE_STATS and stats.shape == (len(losses.PREFERENCE_STATS),)
    assert stats[7] == len(pair_c) and stats[6] == ref["stats"][6]


@pytest.mark.parametrize("name", list(P.TRIES))
def test_the_pairing(name):
    plan, att_lens, depth, n_real, pair_c, pair_r = P.build(name)
    S = sum(map(len, att_lens))
    assert S % 2 == 0 and sorted(list(pair_c) + list(pair_r)) == list(range(S)) and list(pair_c) == sorted(pair_c)
    assert att_lens[-1][-1] == att_lens[-1][-2] and {S - 2, S - 1} in [{int(c), int(r)} for c, r in zip(pair_c, pair_r)]
    atts = [{"pair_id": None} for _ in range(S)]
    for q, (c, r) in enumerate(zip(pair_c, pair_r)):
        atts[c] = {"pair_id": q, "chosen": True}; atts[r] = {"pair_id": q, "chosen": False}
    got_c, got_r = packing.preference_pair_tables(P.attach_lists_of(att_lens, atts))
    assert np.array_equal(got_c, pair_c) and np.array_equal(got_r, pair_r) and got_c.dtype == np.int32
    if S >= 12:
        assert (np.abs(pair_c - pair_r) > 1).any() and (pair_c > pair_r).any() and (pair_c < pair_r).any()


@pytest.mark.parametrize("cfg", list(P.CONFIGS()))
@pytest.mark.parametrize("name", list(P.TRIES))
@pytest.mark.parametrize("seed", [11])
def test_every_pair_is_away_from_every_edge(name, cfg, seed):
    """The seed of the kernel tests.  The one exception: the duplicate pair, an exact tie by construction, which is not correct."""
    loss, (plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts), ref = P.case(name, cfg, seed=seed)
    assert ref["margin_hinge"] >= 1e-3 and ref["margin_correct"] >= 1e-3, (ref["margin_hinge"], ref["margin_correct"])
    assert ref["ties"] == 1
    S = len(atts)
    q = [i for i, (c, r) in enumerate(zip(pair_c, pair_r)) if {int(c), int(r)} == {S - 2, S - 1}]
    assert len(q) == 1 and ref["du"][q[0]] == 0.0 and ref["u"][S - 2] == ref["u"][S - 1]
    assert ref["stats"][6] == float((ref["du"] > 0).sum()) and ref["stats"][7] == len(pair_c)
    if P.CONFIGS()[cfg][1] is not None and len(pair_c) > 1:
        want = np.asarray([P.TARGETS[i % 6] for i in range(len(pair_c))])
        keep = np.arange(len(pair_c)) != q[0]
        assert np.abs(ref["du"][keep] - want[keep]).max() < 1e-2           # the pairs sit on the target list
    if loss.kind == "hinge" and len(pair_c) >= 7:
        assert (ref["z"] < 1).any() and (ref["z"] > 1).any()                 # both branches of the hinge occur


def test_the_bound_is_small_and_positive():
    """The bound is a bound, not a tolerance in disguise: where the sums are short it is a few ulp of the result; it grows with the
    length of the sequence sums only (the (n - 1) u A of a sum in any order)."""
    for name, rel in (("folded", 2e-5), ("fan300", 2e-4), ("long_path", 0.2)):
        loss, inputs, ref = P.case(name, "cdpo_sft", seed=11)
        assert (ref["b_dlp"][ref["dlp"] != 0] > 0).all() and ref["b_dlp"].max() <= rel * np.abs(ref["dlp"]).max(), name
        assert (ref["b_stats"][:6] > 0).all() and (ref["b_stats"][6:] == 0).all()
