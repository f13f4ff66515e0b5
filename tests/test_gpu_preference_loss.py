"""GPU: the fused preference objective (ops.preference_loss -> dta_preference_loss) against the float64 closed form of
preference_ref64, element by element of dlp, g and u and entry by entry of the statistics, within the bound derived in that module's
docstring; on every hand-made trie of policy_loss_ref64 (folded prefixes, an all-masked sequence, a length-1 sequence as a pair member,
filler rows of a padded plan), on long_path (three runs; the 256-thread stride repeats inside a run) and on many_seqs (the sequence
pass's grid stride repeats; more than one workgroup in the pair pass); for all three kinds, both forms of the reference, SimPO
(reference_free + length_normalize + gamma), label smoothing and the SFT term.  The two counts are exact, the duplicate pair - an exact
tie - is not correct, filler rows are exactly 0, and two identical calls give identical bits."""
import numpy as np
import pytest
import torch

import preference_ref64 as P
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._staging import upload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}


def _torch_atts(atts, device="cpu"):
    return [{k: (torch.from_numpy(np.asarray(v)).to(device) if isinstance(v, np.ndarray) else v) for k, v in a.items()} for a in atts]


def _run(loss, plan, att_lens, depth, lp, atts, device="cpu"):
    attach_lists = P.attach_lists_of(att_lens, _torch_atts(atts, device))
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    tables = [lo, hi, seq_ptr, depth, *packing.policy_path_tables(plan, attach_lists), *packing.preference_pair_tables(attach_lists)]
    lo_d, hi_d, ptr_d, depth_d, *rest = upload(tables, DEV, np.int32)
    ref_lp, ref_sum, mask = ops.preference_token_inputs(loss, attach_lists, seq_ptr, DEV)
    dlp, stats, g, u = ops.preference_loss(loss, torch.from_numpy(lp).to(DEV), depth_d, lo_d, hi_d, ptr_d, tuple(rest[:4]), tuple(rest[4:]),
                                           ref_lp, ref_sum, mask)
    return dlp.cpu().numpy(), stats.cpu().numpy(), g.cpu().numpy(), u.cpu().numpy()


@pytest.mark.parametrize("cfg", list(P.CONFIGS()))
@pytest.mark.parametrize("name", list(P.TRIES))
def test_kernel_within_the_derived_bound(name, cfg):
    loss, (plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts), ref = P.case(name, cfg, seed=11)
    assert ref["margin_hinge"] >= 1e-3 and ref["margin_correct"] >= 1e-3 and ref["ties"] == 1      # fp32 and fp64 take the same branches
    dlp, stats, g, u = _run(loss, plan, att_lens, depth, lp, atts)
    label = (name, cfg)
    for got, want, bound, what in ((dlp, ref["dlp"], ref["b_dlp"], "dlp"), (g, ref["g"], ref["b_g"], "g"), (u, ref["u"], ref["b_u"], "u"),
                                   (stats[:6], ref["stats"][:6], ref["b_stats"][:6], "stats")):
        err = np.abs(got.astype(np.float64) - want)
        worst = int(np.argmax(err - bound))
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        WORST[cfg] = max(WORST.get(cfg, 0.0), ratio)
        print(f"{label} {what}: worst element {worst}: got {float(got[worst])!r} want {float(want[worst])!r} error {float(err[worst]):.3e} "
              f"bound {float(bound[worst]):.3e}; largest error / bound {ratio:.3f}")
        assert (err <= bound).all(), (label, what, worst, float(got[worst]), float(want[worst]), float(err[worst]), float(bound[worst]))
    print(f"{cfg}: largest error / bound over the tries so far {WORST[cfg]:.3f}")
    assert stats[6] == ref["stats"][6] and stats[7] == len(pair_c)       # the counts are exact; the tie pair is not correct
    S = len(atts)
    assert u[S - 2] == u[S - 1]                                          # the duplicate pair: the same bits
    assert (dlp[n_real:] == 0).all() and (dlp[depth == 0] == 0).all()    # filler rows and roots: exactly 0
    again = _run(loss, plan, att_lens, depth, lp, atts)
    for a, b in zip((dlp, stats, g, u), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (label, "two runs differ in their bits")


def test_the_tries_repeat_the_loops_they_are_meant_to():
    """long_path: a sequence longer than one workgroup stride (256) whose path has three runs, the last longer than a stride; many_seqs:
    more sequences than the sequence pass's grid cap (2048) and more pairs than one workgroup of the pair pass (256); fan300: rows
    with more sequences through them than one thread sums (the wave path of the row pass); filler: rows past the real ones."""
    from dynamictreeattn_amd._lib import lib
    plan, att, _, _, pair_c, _ = P.build("long_path")
    run_ptr, row0, depth0, seq_leaf = packing.policy_path_tables(plan, P.attach_lists_of(att))
    assert run_ptr[3] - run_ptr[2] == 3 and max(att[2]) - 1 > 256 and plan.T - row0[run_ptr[3] - 1] > 256
    plan, att, _, _, pair_c, _ = P.build("many_seqs")
    S = sum(map(len, att))
    assert S > 2048 and len(pair_c) > 256 and lib().dta_preference_loss_blocks(plan.T, S, len(pair_c)) == -(-len(pair_c) // 256) > 1
    plan, att, _, _, _, _ = P.build("fan300")
    lo, hi, _, _ = packing.policy_row_tables(plan, P.attach_lists_of(att))
    assert int((hi - lo).max()) > 64
    plan, _, _, n_real, _, _ = P.build("filler")
    assert plan.T > n_real
    assert any(1 in leaf for leaf in P.build("empty_segments")[1])      # a length-1 sequence is a pair member


def test_attachments_on_the_device_give_the_same_bits():
    for cfg in ("cdpo_sft", "slic"):
        loss, (plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts), _ = P.case("folded", cfg, seed=2)
        host = _run(loss, plan, att_lens, depth, lp, atts)
        dev = _run(loss, plan, att_lens, depth, lp, atts, device=DEV)
        for a, b in zip(host, dev):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_one_form_of_the_reference_per_call():
    loss, (plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts), _ = P.case("folded", "dpo", seed=2)
    mixed = [dict(a) for a in atts]
    mixed[0] = {k: v for k, v in mixed[0].items() if k != "ref_logprobs"}
    mixed[0]["ref_logprob_sum"] = -3.0
    with pytest.raises(ValueError, match="ref_logprob"):
        _run(loss, plan, att_lens, depth, lp, mixed)
    both = [dict(a) for a in atts]
    both[2]["ref_logprob_sum"] = -3.0
    with pytest.raises(ValueError, match="both"):
        _run(loss, plan, att_lens, depth, lp, both)
    none = [dict(a) for a in atts]
    del none[1]["ref_logprobs"]
    with pytest.raises(KeyError, match="ref_logprob"):
        _run(loss, plan, att_lens, depth, lp, none)
