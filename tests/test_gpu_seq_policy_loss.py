"""GPU: the fused sequence-level objective (ops.policy_loss -> dta_policy_loss, ratio_level 1) against the float64 closed form of
seq_policy_loss_ref64 summed over packed rows, element by element of dlp and dent and entry by entry of the statistics, within the bound
derived in that module's docstring; on every hand-made trie of policy_loss_ref64 and the two of seq_policy_loss_ref64 (a sequence of
more than 256 predictions over three row runs; more sequences than the sequence pass has workgroups).  Filler rows are exactly 0, the
two counts are exact, two runs give the same bits, and so do attachments on the host and on the device."""
import numpy as np
import pytest
import torch

import seq_policy_loss_ref64 as Q
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._staging import upload
from dynamictreeattn_amd.losses import STATS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _torch_atts(atts, device="cpu"):
    return [{k: (v if isinstance(v, float) else torch.from_numpy(np.asarray(v)).to(device)) for k, v in a.items()} for a in atts]


def _run(loss, plan, att_lens, depth, lp, ent, atts, device="cpu"):
    attach_lists = Q.attach_lists_of(att_lens, _torch_atts(atts, device))
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    lo_d, hi_d, ptr_d, depth_d, *path_d = upload([lo, hi, seq_ptr, depth, *packing.policy_path_tables(plan, attach_lists)], DEV, np.int32)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, DEV)
    dlp, dent, stats, w = ops.policy_loss(loss, torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d,
                                          old, ref, mask, adv, per_seq, tuple(path_d))
    return dlp.cpu().numpy(), dent.cpu().numpy(), stats.cpu().numpy(), w.cpu().numpy(), per_seq


def _check(name, cfg, label, **kw):
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), ref = Q.case(name, cfg, **kw)
    assert ref["margin"] >= 1e-3, (label, ref["margin"])               # fp32 and fp64 take the same branch in every sequence
    dlp, dent, stats, w, per_seq = _run(loss, plan, att_lens, depth, lp, ent, atts)
    assert per_seq == bool(kw.get("scalar_adv"))
    for got, want, bound, what in ((dlp, ref["dlp"], ref["b_dlp"], "dlp"), (dent, ref["dent"], ref["b_dent"], "dent"),
                                   (stats[:6], ref["stats"], ref["b_stats"], "stats")):
        err = np.abs(got.astype(np.float64) - want)
        worst = int(np.argmax(err - bound))
        print(f"{label} {what}: worst element {worst}: got {float(got[worst])!r} want {float(want[worst])!r} error {float(err[worst]):.3e} "
              f"bound {float(bound[worst]):.3e}; largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (label, what, worst, float(got[worst]), float(want[worst]), float(err[worst]), float(bound[worst]))
    assert stats[4] == ref["stats"][4] and stats[5] == ref["stats"][5] and stats.shape == (len(STATS),)  # the counts are exact
    assert (dlp[n_real:] == 0).all() and (dent[n_real:] == 0).all()                                      # filler rows: exactly 0
    if loss.entropy_coef == 0:
        assert (dent == 0).all()
    again = _run(loss, plan, att_lens, depth, lp, ent, atts)
    for a, b in zip((dlp, dent, stats, w), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (label, "two runs differ in their bits")
    return ref, dlp, stats


@pytest.mark.parametrize("cfg", list(Q.SEQ_CONFIGS()))
@pytest.mark.parametrize("name", list(Q.TRIES))
def test_kernel_within_the_derived_bound(name, cfg):
    ref, dlp, stats = _check(name, cfg, (name, cfg), seed=11)
    if name in ("fan300", "filler", "long_path", "many_seqs"):
        assert 0 < stats[4] < stats[5]                                   # clipped and unclipped tokens both occur


@pytest.mark.parametrize("name,cfg", [(name, list(Q.SEQ_CONFIGS())[i % 3]) for i, name in enumerate(Q.TRIES)])
def test_on_policy_and_scalar_advantages(name, cfg):
    ref, _, stats = _check(name, cfg, (name, cfg, "on policy"), seed=5, on_policy=True)
    assert (ref["r"] == 1.0).all() and stats[4] == 0                     # ratio 1: nothing is clipped
    _check(name, cfg, (name, cfg, "scalar"), seed=6, scalar_adv=True)


def test_the_new_tries_repeat_the_loops_they_are_meant_to():
    """long_path: a sequence longer than one workgroup stride (256) whose path has three runs, the last longer than a stride;
    many_seqs: more sequences than the sequence pass's grid cap.  And the inputs reach 3 nats from old / ref."""
    from dynamictreeattn_amd._lib import lib
    plan, att, _, _ = Q.build("long_path")
    run_ptr, row0, depth0, seq_leaf = packing.policy_path_tables(plan, Q.attach_lists_of(att))
    assert run_ptr[3] - run_ptr[2] == 3 and max(att[2]) - 1 > 256 and plan.T - row0[run_ptr[3] - 1] > 256
    plan, att, _, _ = Q.build("many_seqs")
    S = sum(map(len, att))
    assert S - (lib().dta_policy_loss_blocks(plan.T, S) - (lib().dta_policy_loss_blocks(plan.T, 1) - 1)) > 0     # sequences past the grid
    _, (plan, att_lens, _, _, lp, _, atts), _ = Q.case("long_path", "ppo", seed=11)
    assert max(float(np.abs(lp[rows[1:]] - a["old_logprobs"]).max()) for rows, a in zip(Q.paths_of(plan, att_lens), atts)) > 2.5


def test_attachments_on_the_device_give_the_same_bits():
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = Q.case("folded", "dual_k3", seed=2)
    host = _run(loss, plan, att_lens, depth, lp, ent, atts)
    dev = _run(loss, plan, att_lens, depth, lp, ent, atts, device=DEV)
    for a, b in zip(host[:4], dev[:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_a_trie_with_old_logprobs_on_some_sequences_only_is_refused():
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = Q.case("folded", "ppo", seed=2)
    atts = [dict(a) for a in atts]
    atts[0] = {k: v for k, v in atts[0].items() if k != "old_logprobs"}
    with pytest.raises(ValueError, match="old_logprobs"):
        _run(loss, plan, att_lens, depth, lp, ent, atts)


def test_the_path_tables_go_with_the_sequence_ratio_only():
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = Q.case("folded", "ppo", seed=2)
    attach_lists = Q.attach_lists_of(att_lens, _torch_atts(atts))
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    lo_d, hi_d, ptr_d, depth_d, *path_d = upload([lo, hi, seq_ptr, depth, *packing.policy_path_tables(plan, attach_lists)], DEV, np.int32)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, DEV)
    args = (torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d, old, ref, mask, adv, per_seq)
    with pytest.raises(ValueError, match="path_tables"):
        ops.policy_loss(loss, *args)
    from dynamictreeattn_amd.losses import PolicyLoss
    with pytest.raises(ValueError, match="path_tables"):
        ops.policy_loss(PolicyLoss(), *args, tuple(path_d))
