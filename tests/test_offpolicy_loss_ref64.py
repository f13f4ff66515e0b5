"""losses.PolicyLoss with an off-policy correction or the CISPO surrogate on the CPU: its torch definition (float64, autograd) against
the independent closed form of offpolicy_loss_ref64 (numpy, analytic gradients) for every configuration, per sequence and summed over
a trie; overflow and all-masked sequences; the weight as a constant of the gradient that never touches the KL or entropy term; the
default object bit-identical to what it gave before; every refusal of the constructor and the missing-key error; and the margin of
every (trie, configuration, variant) the GPU test uses - without a GPU."""
import numpy as np
import pytest
import torch

import offpolicy_loss_ref64 as O
import policy_loss_ref64 as R
from dynamictreeattn_amd import losses
from dynamictreeattn_amd.losses import PolicyLoss

REL = 1e-12
GPU_TRIES = ("folded", "twins", "fork_at_1", "single_len2", "empty_segments", "fan70", "fan300", "past_block", "filler")
VARIANTS = [(on_policy, scalar) for on_policy in (False, True) for scalar in (False, True)]
GPU_SEED = 11


def _t(att, dtype=torch.float64):
    out = {}
    for k, v in att.items():
        out[k] = v if v is None or isinstance(v, float) else torch.from_numpy(np.asarray(v)) if k == "loss_mask" else torch.from_numpy(np.asarray(v)).to(dtype)
    return out


def _definition(loss, lp, ent, att):
    a = torch.from_numpy(np.asarray(lp, np.float64)).requires_grad_(True)
    e = torch.from_numpy(np.asarray(ent, np.float64)).requires_grad_(True)
    out = loss(a, e, _t(att))
    assert out.dim() == 0 and out.dtype == torch.float64
    out.backward()
    return out.item(), a.grad.numpy(), np.zeros_like(np.asarray(ent, np.float64)) if e.grad is None else e.grad.numpy()


def _as_doubles(loss):
    """the same object with every hyper-parameter the fp32 number the kernel is handed: what trie_ref computes with"""
    f = lambda v: None if v is None else float(np.float32(v))
    return PolicyLoss(clip_low=f(loss.clip_low), clip_high=f(loss.clip_high), dual_clip=f(loss.dual_clip), kl_coef=f(loss.kl_coef),
                      kl_estimator=loss.kl_estimator, entropy_coef=f(loss.entropy_coef), agg=loss.agg, scale=f(loss.scale), ratio=loss.ratio,
                      surrogate=loss.surrogate, is_level=loss.is_level, is_mode=loss.is_mode, is_cap=f(loss.is_cap), is_floor=f(loss.is_floor))


@pytest.mark.parametrize("on_policy,scalar", VARIANTS)
@pytest.mark.parametrize("cfg", list(O.CONFIGS()))
def test_definition_equals_closed_form(cfg, on_policy, scalar):
    """per sequence, on the sequences of `folded` (one all-masked, one whose weight overflows) and `fork_at_1`"""
    loss = O.CONFIGS()[cfg]
    seen = set()
    for name in ("folded", "fork_at_1"):
        plan, att_lens, depth, n_real, lp, ent, atts = O.make_inputs(name, seed=3, on_policy=on_policy, scalar_adv=scalar,
                                                                     seq_ratio=loss.ratio == "sequence")
        for s, (rows, att) in enumerate(zip(O.paths_of(plan, att_lens), atts)):
            ref = O.seq_ref(loss, lp[rows[1:]], ent[rows], att, as_fp32=False)
            val, g_lp, g_ent = _definition(loss, lp[rows[1:]], ent[rows], att)
            mag = float(ref["mag_t_pg"].sum() + ref["mag_t_kl"].sum() + ref["mag_t_ent"].sum())
            assert np.isfinite(val) and np.isfinite(g_lp).all()
            assert abs(val - ref["loss"]) <= REL * max(mag, 1e-300), (cfg, name, s, val, ref["loss"])
            mag_g = float((ref["mag_g_pg"] + ref["mag_g_kl"]).max(initial=0.0))
            assert np.abs(g_lp - (ref["g_pg"] + ref["g_kl"])).max(initial=0.0) <= REL * max(mag_g, 1e-300), (cfg, name, s)
            want_ent = ref["g_ent"] if loss.entropy_coef != 0 else 0 * ref["g_ent"]
            assert np.abs(g_ent[:-1] - want_ent).max(initial=0.0) <= REL * max(float(ref["mag_g_ent"].max(initial=0.0)), 1e-300)
            assert g_ent[-1] == 0.0
            live = ref["m"] > 0
            seen |= {"altered"} if (ref["altered"] & live).any() else set()
            seen |= {"kept"} if (~ref["altered"] & live).any() else set()
            seen |= {"clipped"} if (ref["clipped"] & live).any() else set()
            if name == "folded" and s == 1:
                assert val == 0.0 and (g_lp == 0).all() and (g_ent == 0).all()          # the all-masked sequence
    assert {"kept"} <= seen and (loss.is_level is None or "altered" in seen) and (on_policy or "clipped" in seen), (cfg, seen)


@pytest.mark.parametrize("level", losses.IS_LEVELS)
@pytest.mark.parametrize("mode", losses.IS_MODES)
def test_an_overflowing_or_vanishing_weight_is_the_cap_or_zero_never_nan(level, mode):
    """a masked log-ratio sum of +120 (and +120 per token): exp overflows in fp32 - the definition evaluated in fp32 gives is_cap under
    "truncate" and 0 under "mask"; -120 gives 0 (or, under "mask" with a floor, is dropped); never NaN"""
    loss = PolicyLoss(is_level=level, is_mode=mode, is_cap=2.0, is_floor=0.5 if mode == "mask" else 0.0, kl_coef=0.1)
    n = 4
    lp = torch.tensor([-1.0, -2.0, -0.5, -3.0], dtype=torch.float32)
    ent = torch.ones(n + 1)
    A = torch.tensor([1.0, -1.0, 0.5, 2.0])
    for sign, omega in ((1.0, 2.0 if mode == "truncate" else 0.0), (-1.0, 0.0)):
        att = {"advantages": A, "old_logprobs": lp.clone(), "ref_logprobs": lp - 0.1, "rollout_logprobs": lp - sign * 120.0}
        a = lp.clone().requires_grad_(True)
        out = loss(a, ent, att)
        out.backward()
        no_weight = PolicyLoss(kl_coef=0.1)
        b = lp.clone().requires_grad_(True)
        kl_only = PolicyLoss(clip_low=0.2, clip_high=0.2, kl_coef=0.1)(b, ent, {**att, "advantages": 0.0 * A})
        kl_only.backward()
        want = omega * (no_weight(lp, ent, att) - kl_only.detach()) + kl_only.detach()
        assert torch.isfinite(out) and torch.isfinite(a.grad).all()
        assert abs(out.item() - want.item()) <= 1e-6 * max(abs(want.item()), 1.0), (sign, out.item(), want.item())
        if omega == 0.0:
            assert torch.equal(a.grad, b.grad)                                        # only the KL term is left


def test_the_weight_is_a_constant_that_multiplies_the_surrogate_alone():
    rng = np.random.default_rng(1)
    n = 9
    lp, ent = -rng.uniform(0.1, 3.0, n), rng.uniform(0, 3, n + 1)
    att = {"advantages": rng.normal(0, 1, n), "old_logprobs": lp - rng.uniform(-0.1, 0.1, n), "ref_logprobs": lp + rng.uniform(-1, 1, n),
           "loss_mask": rng.random(n) < 0.8}
    base = dict(kl_coef=0.3, kl_estimator="k2", entropy_coef=0.05)
    y = rng.uniform(-0.5, 0.5, n)
    att_w = {**att, "rollout_logprobs": att["old_logprobs"] - y}
    for level in losses.IS_LEVELS:
        plain, zero_adv = _definition(PolicyLoss(**base), lp, ent, att), _definition(PolicyLoss(**base), lp, ent, {**att, "advantages": 0.0})
        got = _definition(PolicyLoss(**base, is_level=level, is_cap=100.0), lp, ent, att_w)
        m = att["loss_mask"].astype(np.float64)
        omega = np.exp(y) if level == "token" else np.exp((m * y).sum() / (m.sum() if level == "sequence_mean" else 1.0))
        # the gradient of the surrogate part scales by omega exactly; the KL and entropy parts are untouched
        assert np.abs(got[1] - (omega * (plain[1] - zero_adv[1]) + zero_adv[1])).max() <= 1e-12
        assert np.array_equal(got[2], plain[2])
    # on-policy: y is formed from the detached lp - the same numbers as old = lp handed in, and no gradient through omega
    on = {k: v for k, v in att_w.items() if k != "old_logprobs"}
    on["rollout_logprobs"] = lp - y
    loss = PolicyLoss(is_level="token", is_cap=100.0)
    a, b = _definition(loss, lp, ent, on), _definition(loss, lp, ent, {**on, "old_logprobs": lp.copy()})
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    m = att["loss_mask"].astype(np.float64)
    assert np.abs(a[1] - m / m.sum() * np.exp(y) * -att["advantages"]).max() <= 1e-12


def test_cispo_never_zeroes_the_gradient_and_counts_both_sides():
    lp = np.array([-1.0, -2.0, -0.5, -1.5])
    A = np.array([1.0, 1.0, -1.0, -1.0])
    x = np.log(np.array([1.5, 0.5, 1.5, 0.5]))                    # r outside [0.8, 1.2] on both sides, both signs of A
    att = {"advantages": A, "old_logprobs": lp - x}
    loss = PolicyLoss(surrogate="cispo")
    val, g, _ = _definition(loss, lp, np.zeros(5), att)
    rc = np.array([1.2, 0.8, 1.2, 0.8])
    assert np.abs(g - 0.25 * -rc * A).max() <= 1e-15 and abs(val - 0.25 * (-rc * A * lp).sum()) <= 1e-15
    ref = O.seq_ref(loss, lp, np.zeros(5), att, as_fp32=False)
    assert ref["clipped"].all()                                    # PPO would count tokens 0 and 3 only
    assert R.seq_ref(PolicyLoss(), lp, np.zeros(5), att, as_fp32=False)["clipped"].tolist() == [True, False, False, True]
    on = _definition(loss, lp, np.zeros(5), {"advantages": A})     # on-policy: r = 1
    assert np.abs(on[1] - 0.25 * -A).max() <= 1e-15


@pytest.mark.parametrize("cfg", list(R.CONFIGS()))
def test_the_defaults_give_the_same_bits_as_before(cfg):
    """the new arguments at their defaults change nothing: bit-equal to the object built without them, equal to the closed form of
    policy_loss_ref64, rollout_logprobs not looked at, fields still a 4-tuple, the repr as it was"""
    base = R.CONFIGS()[cfg]
    kw = {k: getattr(base, k) for k in ("clip_low", "clip_high", "dual_clip", "kl_coef", "kl_estimator", "entropy_coef", "agg", "scale", "ratio")}
    explicit = PolicyLoss(**kw, surrogate="ppo", is_level=None, is_mode="truncate", is_cap=2.0, is_floor=0.0)
    assert repr(explicit) == repr(base) and "is_level" not in repr(base) and repr(base).endswith("ratio='token')")
    assert not base.extended
    plan, att_lens, depth, n_real, lp, ent, atts = R.make_inputs("folded", seed=3)
    for rows, att in zip(R.paths_of(plan, att_lens), atts):
        a_lp, a_ent = lp[rows[1:]], ent[rows]
        a, b = _definition(base, a_lp, a_ent, att), _definition(explicit, a_lp, a_ent, {**att, "rollout_logprobs": np.zeros(1)})      # not looked at
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        ref = R.seq_ref(base, a_lp, a_ent, att, as_fp32=False)
        mag = float(ref["mag_loss_lp"].sum() + ref["mag_loss_ent"].sum())
        assert abs(a[0] - ref["loss"]) <= REL * max(mag, 1e-300)
        assert np.abs(a[1] - ref["g_lp"]).max(initial=0.0) <= REL * max(float(ref["mag_g_lp"].max(initial=0.0)), 1e-300)
        # the closed form of this module with no correction is the old closed form
        mine = O.seq_ref(base, a_lp, a_ent, att, as_fp32=False)
        assert abs(mine["loss"] - ref["loss"]) <= REL * max(mag, 1e-300) and np.abs(mine["g_pg"] + mine["g_kl"] - ref["g_lp"]).max(initial=0.0) <= 1e-15
        assert len(base.fields(_t(att), rows.size - 1)) == 4 and base.rollout(_t(att), rows.size - 1) is None


def test_the_names_and_the_repr():
    assert losses.SURROGATES == ("ppo", "cispo") and losses.IS_LEVELS == ("token", "sequence", "sequence_mean")
    assert losses.IS_MODES == ("truncate", "mask")
    assert losses.OFFPOLICY_STATS == losses.STATS + ("sum_is_weight", "is_clipped_tokens") and len(losses.OFFPOLICY_STATS) == 8
    assert {"SURROGATES", "IS_LEVELS", "IS_MODES", "OFFPOLICY_STATS"} <= set(losses.__all__)
    d = PolicyLoss()
    assert (d.surrogate, d.is_level, d.is_mode, d.is_cap, d.is_floor) == ("ppo", None, "truncate", 2.0, 0.0)
    r = repr(PolicyLoss(is_level="sequence", is_mode="mask", is_cap=3.0, is_floor=0.25))
    assert all(s in r for s in ("surrogate='ppo'", "is_level='sequence'", "is_mode='mask'", "is_cap=3.0", "is_floor=0.25"))
    assert "surrogate='cispo'" in repr(PolicyLoss(surrogate="cispo")) and "is_cap=5.0" in repr(PolicyLoss(is_cap=5.0))
    assert PolicyLoss(surrogate="cispo").extended and PolicyLoss(is_level="token").extended


def test_the_constructor_refuses_naming_the_argument():
    nan, inf = float("nan"), float("inf")
    for bad in ("grpo", "CISPO", None, 1):
        with pytest.raises(ValueError, match="surrogate"):
            PolicyLoss(surrogate=bad)
    for bad in ("tokens", "seq", "none", 0):
        with pytest.raises(ValueError, match="is_level"):
            PolicyLoss(is_level=bad)
    for bad in ("clip", "truncated", None, 0):
        with pytest.raises(ValueError, match="is_mode"):
            PolicyLoss(is_mode=bad)
    for bad in (0.0, -1.0, nan, inf, -inf):
        with pytest.raises(ValueError, match="is_cap"):
            PolicyLoss(is_level="token", is_cap=bad)
    for bad in (-0.1, nan, inf, 2.0, 3.0):
        with pytest.raises(ValueError, match="is_floor"):
            PolicyLoss(is_level="token", is_mode="mask", is_cap=2.0, is_floor=bad)
    with pytest.raises(ValueError, match="is_floor"):
        PolicyLoss(is_level="token", is_mode="truncate", is_floor=0.5)
    with pytest.raises(ValueError, match="is_floor"):
        PolicyLoss(is_floor=0.5)                                       # also without a correction: the default mode is "truncate"
    with pytest.raises(ValueError, match="surrogate"):
        PolicyLoss(surrogate="cispo", ratio="sequence")
    with pytest.raises(ValueError, match="dual_clip"):
        PolicyLoss(surrogate="cispo", dual_clip=3.0)
    PolicyLoss(is_level="sequence_mean", is_mode="mask", is_cap=1e-3, is_floor=0.0)      # the limits themselves are fine


def test_the_rollout_key_is_required_exactly_under_a_correction_and_checked():
    n = 5
    lp, ent = torch.zeros(n, dtype=torch.float64) - 1.0, torch.ones(n + 1, dtype=torch.float64)
    att = {"advantages": 1.0}
    loss = PolicyLoss(is_level="token")
    with pytest.raises(KeyError, match="rollout_logprobs"):
        loss(lp, ent, att)
    with pytest.raises(KeyError, match="rollout_logprobs"):
        loss(lp, ent, {**att, "rollout_logprobs": None})
    with pytest.raises(ValueError, match="rollout_logprobs"):
        loss(lp, ent, {**att, "rollout_logprobs": torch.zeros(n + 1)})
    with pytest.raises(ValueError, match="rollout_logprobs"):
        loss(lp, ent, {**att, "rollout_logprobs": [0.0] * n})
    with pytest.raises(ValueError, match="rollout_logprobs"):
        loss(lp, ent, {**att, "rollout_logprobs": torch.zeros(n, 1)})
    assert torch.isfinite(loss(lp, ent, {**att, "rollout_logprobs": lp.clone()}))
    assert torch.isfinite(PolicyLoss(surrogate="cispo")(lp, ent, att))                    # CISPO alone needs no rollout key
    assert len(loss.fields({**att, "rollout_logprobs": lp}, n)) == 4


@pytest.mark.parametrize("name,cfg,on_policy", [("folded", "tok_mask", False), ("empty_segments", "seq_trunc", True), ("fan70", "mean_mask", False),
                                                ("filler", "gspo_tok_trunc", True), ("fork_at_1", "gspo_seq_mask", False),
                                                ("folded", "cispo_tok_trunc_k3", True)])
def test_row_sums_equal_the_definition_per_sequence(name, cfg, on_policy):
    """the closed form summed over packed rows (what the kernel is compared with) = the definition called once per sequence on its
    gathered path, differentiated by autograd and scattered; the statistics' loss entry is that sum"""
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), ref = O.case(name, cfg, seed=3, on_policy=on_policy)
    a = torch.from_numpy(lp.astype(np.float64)).requires_grad_(True)
    e = torch.from_numpy(ent.astype(np.float64)).requires_grad_(True)
    fp32_loss = _as_doubles(loss)
    total = 0.0
    for rows, att in zip(O.paths_of(plan, att_lens), atts):
        rows = torch.from_numpy(rows)
        total = total + fp32_loss(a[rows[1:]], e[rows], _t(att))
    total.backward()
    assert abs(total.item() - ref["stats"][0]) <= 1e-11 * max(abs(ref["stats"][0]), 1.0)
    assert np.abs(a.grad.numpy() - ref["dlp"]).max() <= 1e-11 * np.abs(ref["dlp"]).max()
    ge = np.zeros(plan.T) if e.grad is None else e.grad.numpy()
    assert np.abs(ge - ref["dent"]).max() <= 1e-11 * max(np.abs(ref["dent"]).max(), 1e-300)
    assert (ref["dlp"][n_real:] == 0).all() and (ref["dent"][n_real:] == 0).all()
    assert ref["stats"].shape == (8,) and ref["stats"][5] == sum(float(np.sum(x["loss_mask"])) for x in atts)
    assert 0 <= ref["stats"][7] <= ref["stats"][5] and (loss.is_level is None or ref["stats"][7] > 0)


@pytest.mark.parametrize("name", GPU_TRIES)
def test_the_margin_of_every_gpu_case_and_the_sequences_asked_for(name):
    """every (trie, configuration, with / without old_logprobs, scalar / per-token advantages) of tests/test_gpu_offpolicy_loss.py keeps
    each weight 1e-3 (relative) off is_cap and is_floor and each ratio off the clip edges; sequence 2 overflows; sequence 1 is all-masked"""
    for cfg in O.CONFIGS():
        for on_policy, scalar in VARIANTS:
            loss, (plan, att_lens, depth, n_real, lp, ent, atts), ref = O.case(name, cfg, seed=GPU_SEED, on_policy=on_policy, scalar_adv=scalar)
            assert ref["margin"] >= 1e-3, (name, cfg, on_policy, scalar, ref["margin"])
            assert np.isfinite(ref["dlp"]).all() and np.isfinite(ref["stats"]).all() and np.isfinite(ref["omega"]).all()
            if len(atts) > 1:
                assert not np.asarray(atts[1]["loss_mask"]).any()
            if len(atts) > O.OVERFLOW_SEQ and np.asarray(atts[O.OVERFLOW_SEQ]["loss_mask"]).any():
                s = O.OVERFLOW_SEQ
                rows = O.paths_of(plan, att_lens)[s]
                origin = lp[rows[1:]] if on_policy else atts[s]["old_logprobs"]
                y = origin.astype(np.float64) - atts[s]["rollout_logprobs"]
                assert (np.asarray(atts[s]["loss_mask"]) * y).sum() > 100.0
                if loss.is_level == "sequence":
                    assert ref["omega"][s] == (loss.is_cap if loss.is_mode == "truncate" else 0.0)
