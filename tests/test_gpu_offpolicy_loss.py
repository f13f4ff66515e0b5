"""GPU: the fused objective with an off-policy correction or CISPO (ops.policy_loss -> dta_policy_loss) against the float64 closed
form of offpolicy_loss_ref64 summed over packed rows: dlp and dent element by element, the per-sequence workspaces w, c and omega and
the eight statistics entry by entry, within the bounds derived in that module's docstring; on the hand-made tries of
policy_loss_ref64, for every configuration of offpolicy_loss_ref64.CONFIGS, with and without old_logprobs, with per-token and scalar
advantages.  The three counts are exact, filler rows are exactly 0, two runs give the same bits.  (The margins of these very cases are
asserted on the CPU, tests/test_offpolicy_loss_ref64.py, and here again.)"""
import numpy as np
import pytest
import torch

import offpolicy_loss_ref64 as O
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._staging import upload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("folded", "twins", "fork_at_1", "single_len2", "empty_segments", "fan70", "fan300", "past_block", "filler")
SEED = 11


def _torch_atts(atts, device="cpu"):
    return [{k: (v if isinstance(v, float) else torch.from_numpy(np.asarray(v)).to(device)) for k, v in a.items()} for a in atts]


def _run(loss, plan, att_lens, depth, lp, ent, atts, device="cpu"):
    attach_lists = O.attach_lists_of(att_lens, _torch_atts(atts, device))
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, DEV)
    rollout = ops.policy_rollout_input(loss, attach_lists, seq_ptr, DEV)
    walks = ops.policy_walks_paths(loss, old is None)
    tables = [lo, hi, seq_ptr, depth] + (list(packing.policy_path_tables(plan, attach_lists)) if walks else [])
    lo_d, hi_d, ptr_d, depth_d, *path_d = upload(tables, DEV, np.int32)
    ws = {}
    dlp, dent, stats, w = ops.policy_loss(loss, torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d,
                                          old, ref, mask, adv, per_seq, tuple(path_d) or None, rollout, ws)
    return [t.cpu().numpy() for t in (dlp, dent, stats, w, ws["c"], ws["omega"])], per_seq, walks


def _check(name, cfg, on_policy, scalar):
    label = (name, cfg, "no old" if on_policy else "old", "scalar" if scalar else "per token")
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), ref = O.case(name, cfg, seed=SEED, on_policy=on_policy, scalar_adv=scalar)
    assert ref["margin"] >= 1e-3, (label, ref["margin"])               # fp32 and fp64 take the same branch everywhere
    (dlp, dent, stats, w, c, omega), per_seq, walks = _run(loss, plan, att_lens, depth, lp, ent, atts)
    assert per_seq == scalar
    assert walks == (loss.ratio == "sequence" or (loss.is_level in ("sequence", "sequence_mean") and on_policy))
    for got, want, bound, what in ((dlp, ref["dlp"], ref["b_dlp"], "dlp"), (dent, ref["dent"], ref["b_dent"], "dent"),
                                   (stats, ref["stats"], ref["b_stats"], "stats"), (w, ref["w"], ref["b_w"], "w"),
                                   (c, ref["c"], ref["b_c"], "c"), (omega, ref["omega"], ref["b_omega"], "omega")):
        assert np.isfinite(got).all(), (label, what)
        err = np.abs(got.astype(np.float64) - want)
        worst = int(np.argmax(err - bound))
        print(f"{label} {what}: worst element {worst}: got {float(got[worst])!r} want {float(want[worst])!r} error {float(err[worst]):.3e} "
              f"bound {float(bound[worst]):.3e}; largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (label, what, worst, float(got[worst]), float(want[worst]), float(err[worst]), float(bound[worst]))
    for k in (4, 5, 7):                                                 # clipped, masked and altered tokens: exact
        assert stats[k] == ref["stats"][k], (label, k, float(stats[k]), float(ref["stats"][k]))
    assert (dlp[n_real:] == 0).all() and (dent[n_real:] == 0).all()      # filler rows: exactly 0
    if loss.entropy_coef == 0:
        assert (dent == 0).all()
    if loss.ratio == "token":
        assert (c == 0).all()
    if loss.is_level in (None, "token"):
        assert (omega == 1).all()
    if loss.is_level is None:
        assert stats[6] == stats[5] and stats[7] == 0
    if loss.is_level == "sequence" and len(atts) > O.OVERFLOW_SEQ and np.asarray(atts[O.OVERFLOW_SEQ]["loss_mask"]).any():
        assert omega[O.OVERFLOW_SEQ] == (loss.is_cap if loss.is_mode == "truncate" else 0.0)       # expf overflowed: the cap or 0
    again, _, _ = _run(loss, plan, att_lens, depth, lp, ent, atts)
    for a, b in zip((dlp, dent, stats, w, c, omega), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (label, "two runs differ in their bits")
    return ref, stats


@pytest.mark.parametrize("on_policy", [False, True], ids=["old", "no_old"])
@pytest.mark.parametrize("cfg", list(O.CONFIGS()))
@pytest.mark.parametrize("name", NAMES)
def test_kernel_within_the_derived_bound(name, cfg, on_policy):
    loss = O.CONFIGS()[cfg]
    ref, stats = _check(name, cfg, on_policy, False)
    _check(name, cfg, on_policy, True)
    if name in ("fan300", "filler"):
        if loss.is_level is not None:
            assert 0 < stats[7] < stats[5]                               # altered and unaltered weights both occur
        if not on_policy:
            assert 0 < stats[4] < stats[5]                               # clipped and unclipped tokens both occur
        else:
            assert stats[4] == 0                                         # ratio 1: nothing is clipped


def test_attachments_on_the_device_give_the_same_bits():
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = O.case("folded", "cispo_tok_trunc_k3", seed=2)
    host, _, _ = _run(loss, plan, att_lens, depth, lp, ent, atts)
    dev, _, _ = _run(loss, plan, att_lens, depth, lp, ent, atts, device=DEV)
    for a, b in zip(host, dev):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_rollout_logprobs_on_some_sequences_only_or_on_none_are_refused():
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = O.case("folded", "tok_trunc", seed=2)
    some = [dict(a) for a in atts]
    some[0] = {k: v for k, v in some[0].items() if k != "rollout_logprobs"}
    with pytest.raises(ValueError, match="rollout_logprobs"):
        _run(loss, plan, att_lens, depth, lp, ent, some)
    with pytest.raises(KeyError, match="rollout_logprobs"):
        _run(loss, plan, att_lens, depth, lp, ent, [{k: v for k, v in a.items() if k != "rollout_logprobs"} for a in atts])
    some = [dict(a) for a in atts]
    some[0] = {k: v for k, v in some[0].items() if k != "old_logprobs"}
    with pytest.raises(ValueError, match="old_logprobs"):
        _run(loss, plan, att_lens, depth, lp, ent, some)


def test_the_path_tables_and_the_rollout_vector_go_with_what_needs_them():
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = O.case("folded", "seq_mask", seed=2)
    attach_lists = O.attach_lists_of(att_lens, _torch_atts(atts))
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    lo_d, hi_d, ptr_d, depth_d, *path_d = upload([lo, hi, seq_ptr, depth, *packing.policy_path_tables(plan, attach_lists)], DEV, np.int32)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, DEV)
    rollout = ops.policy_rollout_input(loss, attach_lists, seq_ptr, DEV)
    args = (torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d)
    with pytest.raises(ValueError, match="path_tables"):                 # old_logprobs given: y is a sweep, no path is walked
        ops.policy_loss(loss, *args, old, ref, mask, adv, per_seq, tuple(path_d), rollout)
    with pytest.raises(ValueError, match="path_tables"):                 # without old_logprobs the sequence pass walks the path
        ops.policy_loss(loss, *args, None, ref, mask, adv, per_seq, None, rollout)
    with pytest.raises(ValueError, match="rollout"):
        ops.policy_loss(loss, *args, old, ref, mask, adv, per_seq, None, None)
    from dynamictreeattn_amd.losses import PolicyLoss
    with pytest.raises(ValueError, match="rollout"):
        ops.policy_loss(PolicyLoss(surrogate="cispo"), *args, old, ref, mask, adv, per_seq, None, rollout)
    assert ops.policy_rollout_input(PolicyLoss(), attach_lists, seq_ptr, DEV) is None
    ops.policy_loss(loss, *args, old, ref, mask, adv, per_seq, None, rollout)
    ops.policy_loss(loss, *args, None, ref, mask, adv, per_seq, tuple(path_d), rollout)
