"""losses.PolicyLoss on the CPU: its torch definition (float64, autograd) against the independent closed form of policy_loss_ref64
(numpy, analytic gradients) on inputs that hit every branch; its refusals; the host tables of the fused path
(packing.policy_row_tables) against a walk of every sequence's root path; and the closed form summed over packed rows against the
definition applied per sequence to gathered paths - the row-major argument itself, without a GPU."""
import numpy as np
import pytest
import torch

import policy_loss_ref64 as R
from dynamictreeattn_amd import packing
from dynamictreeattn_amd.losses import PolicyLoss

REL = 1e-12


def _t(att, dtype=torch.float64):
    out = {}
    for k, v in att.items():
        out[k] = v if v is None or isinstance(v, float) else torch.from_numpy(np.asarray(v)) if k == "loss_mask" else torch.from_numpy(np.asarray(v)).to(dtype)
    return out


def _close(got, want, scale):
    return np.abs(np.asarray(got) - np.asarray(want)).max(initial=0.0) <= REL * max(scale, 1e-300)


def _cases():
    """(label, lp [n], ent [n + 1], attachment) with hand-placed ratios: unclipped, both clamps with both signs of A, the dual-clip
    region, A = 0, masked tokens; then an all-masked sequence, old_logprobs absent, a scalar advantage, no mask."""
    r = np.array([1.0, 1.1, 1.5, 1.5, 0.5, 0.5, 4.0, 4.0, 0.85, 2.0, 0.3, 1.25])
    A = np.array([0.7, -0.4, 1.3, -1.3, 0.9, -0.9, -0.6, 0.6, 0.0, 0.0, 2.0, 1.0])
    n = r.size
    rng = np.random.default_rng(0)
    lp = -rng.uniform(0.1, 4.0, n)
    ent = rng.uniform(0.0, 4.0, n + 1)
    ref = lp + rng.uniform(-3, 3, n)
    mask = np.ones(n, bool); mask[[3, 10]] = False
    base = {"advantages": A, "old_logprobs": lp - np.log(r), "ref_logprobs": ref, "loss_mask": mask}
    fmask = np.where(mask, 0.5, 0.0); fmask[0] = 1.0
    return [("all branches", lp, ent, base),
            ("float mask", lp, ent, {**base, "loss_mask": fmask}),
            ("all masked", lp, ent, {**base, "loss_mask": np.zeros(n, bool)}),
            ("on policy", lp, ent, {k: v for k, v in base.items() if k != "old_logprobs"}),
            ("old None", lp, ent, {**base, "old_logprobs": None}),
            ("scalar advantage", lp, ent, {**base, "advantages": -0.75}),
            ("no mask", lp, ent, {k: v for k, v in base.items() if k != "loss_mask"}),
            ("one prediction", lp[:1], ent[:2], {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in base.items()})]


@pytest.mark.parametrize("cfg", list(R.CONFIGS()))
def test_definition_equals_closed_form(cfg):
    loss = R.CONFIGS()[cfg]
    seen = set()
    for label, lp, ent, att in _cases():
        ref = R.seq_ref(loss, lp, ent, att, as_fp32=False)
        assert ref["margin"] >= 1e-3, (cfg, label, ref["margin"])          # fp32 and fp64 take the same branch: asserted on the reference
        a = torch.from_numpy(lp).requires_grad_(True)
        e = torch.from_numpy(ent).requires_grad_(True)
        out = loss(a, e, _t(att))
        assert out.dim() == 0 and out.dtype == torch.float64
        out.backward()
        mag = float(ref["mag_loss_lp"].sum() + ref["mag_loss_ent"].sum())
        assert abs(out.item() - ref["loss"]) <= REL * max(mag, 1e-300), (cfg, label, out.item(), ref["loss"])
        assert _close(a.grad.numpy(), ref["g_lp"], float(ref["mag_g_lp"].max(initial=0.0))), (cfg, label)
        ge = np.zeros_like(ent) if e.grad is None else e.grad.numpy()
        assert _close(ge[:-1], ref["g_ent"] if loss.entropy_coef != 0 else 0 * ref["g_ent"], float(ref["mag_g_ent"].max(initial=0.0))), (cfg, label)
        assert ge[-1] == 0.0                                                # entropy[len - 1] is not used
        if "old_logprobs" in att and att["old_logprobs"] is not None and not isinstance(att["advantages"], float):
            x = lp - att["old_logprobs"]; A = att["advantages"]; rr = np.exp(x)
            lo, hi = 1 - loss.clip_low, 1 + loss.clip_high
            seen |= {"in"} if ((rr >= lo) & (rr <= hi) & (A != 0)).any() else set()
            seen |= {"hi+"} if ((rr > hi) & (A > 0) & (ref["g_lp"] == 0) & (ref["m"] > 0)).any() else set()
            seen |= {"lo-"} if ((rr < lo) & (A < 0) & (ref["g_lp"] == 0) & (ref["m"] > 0)).any() else set()
            seen |= {"zero"} if (A == 0).any() else set()
            seen |= {"masked"} if (ref["m"] == 0).any() else set()
            if loss.dual_clip is not None:
                seen |= {"dual"} if ((rr > loss.dual_clip) & (A < 0) & ref["clipped"]).any() else set()
    want = {"in", "zero", "masked"} | ({"dual"} if loss.dual_clip is not None else set())
    if loss.kl_coef == 0:
        want |= {"hi+", "lo-"}                                              # (a KL term keeps the gradient of a clipped token non-zero)
    assert want <= seen, (cfg, want - seen)


def test_clipped_tokens_have_exactly_zero_policy_gradient():
    loss = PolicyLoss(clip_low=0.2, clip_high=0.2)
    _, lp, ent, att = _cases()[0]
    a = torch.from_numpy(lp).requires_grad_(True)
    loss(a, torch.from_numpy(ent), _t(att)).backward()
    r, A = np.exp(lp - att["old_logprobs"]), att["advantages"]
    clipped = ((r > 1.2) & (A > 0)) | ((r < 0.8) & (A < 0))
    assert clipped.sum() >= 3 and (a.grad.numpy()[clipped] == 0).all() and (a.grad.numpy()[~clipped & (A != 0) & att["loss_mask"]] != 0).all()


def test_all_masked_sequence_divides_by_one():
    loss = PolicyLoss(kl_coef=0.1, entropy_coef=0.1)
    _, lp, ent, att = _cases()[2]
    a = torch.from_numpy(lp).requires_grad_(True)
    out = loss(a, torch.from_numpy(ent), _t(att))
    out.backward()
    assert out.item() == 0.0 and np.isfinite(a.grad.numpy()).all() and (a.grad.numpy() == 0).all()


def test_refusals_name_the_argument():
    for kw, name in ((dict(kl_estimator="k4"), "kl_estimator"), (dict(agg="mean"), "agg"), (dict(clip_low=-0.1), "clip_low"),
                     (dict(clip_high=-1e-9), "clip_high"), (dict(dual_clip=1.0), "dual_clip"), (dict(dual_clip=0.5), "dual_clip"),
                     (dict(kl_coef=float("nan")), "kl_coef"), (dict(entropy_coef=float("inf")), "entropy_coef"),
                     (dict(scale=float("inf")), "scale"), (dict(clip_low=float("nan")), "clip_low"), (dict(dual_clip=float("inf")), "dual_clip")):
        with pytest.raises(ValueError, match=name):
            PolicyLoss(**kw)
    lp, ent = torch.zeros(5), torch.zeros(6)
    ok = {"advantages": torch.ones(5), "old_logprobs": torch.zeros(5), "ref_logprobs": torch.zeros(5), "loss_mask": torch.ones(5, dtype=torch.bool)}
    loss = PolicyLoss(kl_coef=0.1)
    loss(lp, ent, ok)
    for key in ("advantages", "old_logprobs", "ref_logprobs", "loss_mask"):
        with pytest.raises(ValueError, match=key):
            loss(lp, ent, {**ok, key: torch.ones(4)})
    with pytest.raises(KeyError, match="advantages"):
        loss(lp, ent, {k: v for k, v in ok.items() if k != "advantages"})
    with pytest.raises(KeyError, match="ref_logprobs"):
        loss(lp, ent, {k: v for k, v in ok.items() if k != "ref_logprobs"})
    PolicyLoss()(lp, ent, {"advantages": 1.0})                              # no KL: ref_logprobs is not asked for


# ---- the host tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TRIES))
def test_row_tables_equal_the_walk_of_every_root_path(name):
    plan, att_lens, depth, n_real = R.build(name)
    lo, hi, seq_ptr, seq_lens = packing.policy_row_tables(plan, R.attach_lists_of(att_lens))
    T, S = plan.T, sum(map(len, att_lens))
    assert lo.shape == hi.shape == (T,) and lo.dtype == hi.dtype == seq_ptr.dtype == np.int32 and seq_ptr.shape == (S + 1,)
    assert seq_lens.tolist() == [n for leaf in att_lens for n in leaf] and seq_ptr.tolist() == [0] + np.cumsum(seq_lens - 1).tolist()
    through = [set() for _ in range(T)]                                     # brute force: the sequences whose root path holds row t
    for s, rows in enumerate(R.paths_of(plan, att_lens)):
        assert (depth[rows] == np.arange(rows.size)).all()
        for t in rows:
            through[t].add(s)
    for t in range(T):
        assert 0 <= lo[t] <= hi[t] <= S
        got = {s for s in range(lo[t], hi[t]) if seq_lens[s] > depth[t]}
        assert got == through[t], (name, t, int(depth[t]), int(lo[t]), int(hi[t]))
    if name == "filler":
        assert T >= 2048 and n_real % 256 and T % 256 == 0 and T > n_real
        assert (lo[n_real:] == 0).all() and (hi[n_real:] == 0).all()        # filler rows belong to no sequence
    assert all(through[t] for t in range(n_real) if name != "empty_segments")


def test_the_tries_are_the_ones_asked_for():
    plan, att, _, _ = R.build("folded")
    assert att[0] == [3, 5, 7] and plan.seg_depth0[1] == 3                  # two shorter sequences on leaf 0, one ending at leaf 1's fork
    assert R.TRIES["twins"][2] == [[4, 4]] and R.TRIES["fork_at_1"][1][0] == 1 and R.TRIES["single_len2"][0] == [2]
    assert (np.diff(R.build("empty_segments")[0].seg_off) == 0).sum() == 2
    assert len(R.TRIES["fan70"][0]) > 64 and len(R.TRIES["fan300"][0]) > 256 and R.build("past_block")[0].T == 257


# ---- rows against sequences ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [("folded", "dual_k3"), ("empty_segments", "k2"), ("fan70", "k1_sum"), ("filler", "ppo")])
def test_row_sums_equal_the_definition_per_sequence(name, cfg):
    """The closed form summed row by row (what the kernel is checked against) = the definition called once per sequence on its
    gathered path, differentiated by autograd and scattered back: loss, d/dlp, d/dent."""
    loss = R.CONFIGS()[cfg]
    plan, att_lens, depth, n_real, lp, ent, atts = R.make_inputs(name, seed=3)
    ref = R.trie_ref(loss, plan, att_lens, lp, ent, atts)
    assert ref["margin"] >= 1e-3
    a = torch.from_numpy(lp.astype(np.float64)).requires_grad_(True)
    e = torch.from_numpy(ent.astype(np.float64)).requires_grad_(True)
    fp32_loss = PolicyLoss(**{k: (None if getattr(loss, k) is None else float(np.float32(getattr(loss, k))))
                              for k in ("clip_low", "clip_high", "dual_clip", "kl_coef", "entropy_coef", "scale")},
                           kl_estimator=loss.kl_estimator, agg=loss.agg)
    total = 0.0
    for rows, att in zip(R.paths_of(plan, att_lens), atts):
        rows = torch.from_numpy(rows)
        total = total + fp32_loss(a[rows[1:]], e[rows], _t(att))
    total.backward()
    assert abs(total.item() - ref["stats"][0]) <= 1e-11 * max(abs(ref["stats"][0]), 1.0)
    assert np.abs(a.grad.numpy() - ref["dlp"]).max() <= 1e-11 * np.abs(ref["dlp"]).max()
    ge = np.zeros(plan.T) if e.grad is None else e.grad.numpy()
    assert np.abs(ge - ref["dent"]).max() <= 1e-11 * max(np.abs(ref["dent"]).max(), 1e-300)
    assert (ref["dlp"][n_real:] == 0).all() and (ref["dent"][n_real:] == 0).all()
    assert ref["stats"][5] == sum(float(np.asarray(t["loss_mask"]).sum()) for t in atts)
