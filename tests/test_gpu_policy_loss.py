"""GPU: the fused policy objective (ops.policy_loss -> dta_policy_loss) against the float64 closed form of policy_loss_ref64 summed over
packed rows, element by element of dlp and dent and entry by entry of the statistics, within the bound derived in that module's
docstring; on the hand-made tries of that module (folded sequences, twins, a fork at depth 1, one 2-token sequence, empty segments,
more than 64 and more than 256 sequences through the root rows, T one past a workgroup, filler rows).  Filler rows are exactly 0, the
two counts are exact, and two runs give the same bits."""
import numpy as np
import pytest
import torch

import policy_loss_ref64 as R
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._staging import upload

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _torch_atts(atts, device="cpu"):
    return [{k: (v if isinstance(v, float) else torch.from_numpy(np.asarray(v)).to(device)) for k, v in a.items()} for a in atts]


def _run(loss, plan, att_lens, depth, lp, ent, atts, device="cpu"):
    attach_lists = R.attach_lists_of(att_lens, _torch_atts(atts, device))
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    lo_d, hi_d, ptr_d, depth_d = upload([lo, hi, seq_ptr, depth], DEV, np.int32)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, DEV)
    dlp, dent, stats, w = ops.policy_loss(loss, torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d,
                                          old, ref, mask, adv, per_seq)
    return dlp.cpu().numpy(), dent.cpu().numpy(), stats.cpu().numpy(), w.cpu().numpy(), per_seq


def _check(loss, name, label, **kw):
    plan, att_lens, depth, n_real, lp, ent, atts = R.make_inputs(name, **kw)
    ref = R.trie_ref(loss, plan, att_lens, lp, ent, atts)
    assert ref["margin"] >= 1e-3, (label, ref["margin"])               # fp32 and fp64 take the same branch everywhere
    dlp, dent, stats, w, per_seq = _run(loss, plan, att_lens, depth, lp, ent, atts)
    assert per_seq == bool(kw.get("scalar_adv"))
    for got, want, bound, what in ((dlp, ref["dlp"], ref["b_dlp"], "dlp"), (dent, ref["dent"], ref["b_dent"], "dent"),
                                   (stats[:6], ref["stats"], ref["b_stats"], "stats")):
        err = np.abs(got.astype(np.float64) - want)
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), (label, what, worst, float(got[worst]), float(want[worst]), float(err[worst]), float(bound[worst]))
    assert stats[4] == ref["stats"][4] and stats[5] == ref["stats"][5] and (stats[6:] == 0).all()      # the counts are exact
    assert (dlp[n_real:] == 0).all() and (dent[n_real:] == 0).all()                                      # filler rows: exactly 0
    if loss.entropy_coef == 0:
        assert (dent == 0).all()
    again = _run(loss, plan, att_lens, depth, lp, ent, atts)
    for a, b in zip((dlp, dent, stats, w), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (label, "two runs differ in their bits")
    return ref, dlp, stats


@pytest.mark.parametrize("cfg", list(R.CONFIGS()))
@pytest.mark.parametrize("name", list(R.TRIES))
def test_kernel_within_the_derived_bound(name, cfg):
    _check(R.CONFIGS()[cfg], name, (name, cfg), seed=11)


@pytest.mark.parametrize("name,cfg", [("folded", "dual_k3"), ("fan300", "ppo"), ("filler", "k1_sum")])
def test_on_policy_and_scalar_advantages(name, cfg):
    loss = R.CONFIGS()[cfg]
    _check(loss, name, (name, cfg, "on policy"), seed=5, on_policy=True)
    _check(loss, name, (name, cfg, "scalar"), seed=6, scalar_adv=True)
    _check(loss, name, (name, cfg, "both"), seed=7, scalar_adv=True, on_policy=True)


def test_the_wide_rows_are_really_wide_and_the_terms_large():
    """The fan tries put more sequences through their root rows than the single-thread limit, one wave and one workgroup hold; and the
    inputs reach 3 nats from old / ref, so the bound's amplification term is exercised."""
    for name, least in (("fan70", 65), ("fan300", 257)):
        plan, att_lens, depth, _ = R.build(name)
        lo, hi, _, _ = packing.policy_row_tables(plan, R.attach_lists_of(att_lens))
        assert int((hi - lo).max()) >= least and int((hi - lo).min()) >= 1
    _, att_lens, _, _, lp, _, atts = R.make_inputs("filler", seed=11)
    assert max(float(np.abs(a["ref_logprobs"]).max()) for a in atts) > 3.0


def test_attachments_on_the_device_give_the_same_bits():
    loss = R.CONFIGS()["dual_k3"]
    plan, att_lens, depth, n_real, lp, ent, atts = R.make_inputs("folded", seed=2)
    host = _run(loss, plan, att_lens, depth, lp, ent, atts)
    dev = _run(loss, plan, att_lens, depth, lp, ent, atts, device=DEV)
    for a, b in zip(host[:4], dev[:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_a_trie_with_old_logprobs_on_some_sequences_only_is_refused():
    loss = R.CONFIGS()["ppo"]
    plan, att_lens, depth, n_real, lp, ent, atts = R.make_inputs("folded", seed=2)
    atts[0] = {k: v for k, v in atts[0].items() if k != "old_logprobs"}
    with pytest.raises(ValueError, match="old_logprobs"):
        _run(loss, plan, att_lens, depth, lp, ent, atts)
