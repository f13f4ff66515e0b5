"""losses.PolicyLoss(ratio="sequence") on the CPU: its torch definition (float64, autograd) against the independent closed form of
seq_policy_loss_ref64 (numpy, analytic gradients); the on-policy, all-masked and 2-token cases as the definition states them; the
token-level objects unchanged; the refusal of an unknown ratio; the host tables of the fused path (packing.policy_path_tables) against
a walk of every sequence's root path; and the closed form summed over packed rows (c_s m + the KL gradient, row by row over the row
tables) against the definition applied per sequence - without a GPU."""
import numpy as np
import pytest
import torch

import policy_loss_ref64 as R
import seq_policy_loss_ref64 as Q
from dynamictreeattn_amd import losses, packing
from dynamictreeattn_amd.losses import PolicyLoss

REL = 1e-12


def _t(att, dtype=torch.float64):
    out = {}
    for k, v in att.items():
        out[k] = v if v is None or isinstance(v, float) else torch.from_numpy(np.asarray(v)) if k == "loss_mask" else torch.from_numpy(np.asarray(v)).to(dtype)
    return out


def _cases():
    """(label, lp [n], ent [n + 1], attachment): per-token ratios spread over 0.3 .. 4 with both signs of A, zeros and masked tokens,
    the masked mean log-ratio placed on `target`; then the variants."""
    out = []
    rng = np.random.default_rng(0)
    n = 12
    lp = -rng.uniform(0.1, 4.0, n)
    ent = rng.uniform(0.0, 4.0, n + 1)
    A = np.array([0.7, -0.4, 1.3, -1.3, 0.9, -0.9, -0.6, 0.6, 0.0, 0.0, 2.0, 1.0])
    mask = np.ones(n, bool); mask[[3, 10]] = False
    ref = lp + rng.uniform(-3, 3, n)
    for target in Q.TARGETS:
        x = np.log(np.array([1.0, 1.1, 1.5, 1.5, 0.5, 0.5, 4.0, 4.0, 0.85, 2.0, 0.3, 1.25]))
        x[mask] += target - x[mask].mean()
        base = {"advantages": A, "old_logprobs": lp - x, "ref_logprobs": ref, "loss_mask": mask}
        out.append((f"target {target}", lp, ent, base))
    base = out[0][3]
    out += [("all masked", lp, ent, {**base, "loss_mask": np.zeros(n, bool)}),
            ("on policy", lp, ent, {k: v for k, v in base.items() if k != "old_logprobs"}),
            ("old None", lp, ent, {**base, "old_logprobs": None}),
            ("scalar advantage", lp, ent, {**base, "advantages": -0.75}),
            ("no mask", lp, ent, {k: v for k, v in base.items() if k != "loss_mask"}),
            ("one prediction", lp[:1], ent[:2], {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in base.items()})]
    return out


def _definition(loss, lp, ent, att):
    a = torch.from_numpy(np.asarray(lp, np.float64)).requires_grad_(True)
    e = torch.from_numpy(np.asarray(ent, np.float64)).requires_grad_(True)
    out = loss(a, e, _t(att))
    assert out.dim() == 0 and out.dtype == torch.float64
    out.backward()
    return out.item(), a.grad.numpy(), np.zeros_like(ent) if e.grad is None else e.grad.numpy()


@pytest.mark.parametrize("cfg", list(Q.SEQ_CONFIGS()))
def test_definition_equals_closed_form(cfg):
    loss = Q.SEQ_CONFIGS()[cfg]
    assert loss.ratio == "sequence"
    seen = set()
    for label, lp, ent, att in _cases():
        ref = Q.seq_ref(loss, lp, ent, att, as_fp32=False)
        assert ref["margin"] >= 1e-3, (cfg, label, ref["margin"])
        val, g_lp, g_ent = _definition(loss, lp, ent, att)
        mag = float(ref["mag_t_pg"].sum() + ref["mag_t_kl"].sum() + ref["mag_t_ent"].sum())
        assert abs(val - ref["loss"]) <= REL * max(mag, 1e-300), (cfg, label, val, ref["loss"])
        mag_g = float((ref["mag_g_pg"] + ref["mag_g_kl"]).max(initial=0.0))
        assert np.abs(g_lp - ref["g_lp"]).max() <= REL * max(mag_g, 1e-300), (cfg, label)
        assert np.abs(g_ent[:-1] - (ref["g_ent"] if loss.entropy_coef != 0 else 0 * ref["g_ent"])).max() <= REL * max(float(ref["mag_g_ent"].max()), 1e-300)
        assert g_ent[-1] == 0.0
        if label.startswith("target"):
            live = ref["m"] > 0
            seen |= {"clipped"} if (ref["clipped"] & live).any() else set()
            seen |= {"unclipped"} if (~ref["clipped"] & live & (att["advantages"] != 0)).any() else set()
            seen |= {"all clipped"} if ref["c"] == 0.0 and (ref["clipped"] & live).any() else set()
            seen |= {"dual"} if loss.dual_clip is not None and ref["r"] > loss.dual_clip else set()
            seen |= {"below"} if ref["r"] < 1 - loss.clip_low else set()
            seen |= {"inside"} if 1 - loss.clip_low < ref["r"] < 1 + loss.clip_high else set()
    want = {"clipped", "unclipped", "below", "inside"} | ({"dual"} if loss.dual_clip is not None else set())
    assert want <= seen, (cfg, want - seen)


def test_the_gradient_reaches_every_masked_token_through_the_sequence_ratio():
    """Inside the clip range no token is clipped: d/dlp_t = c_s m_t with ONE scalar, masked-out tokens get exactly 0 - and the value
    differs from the token-level objective's on the same inputs."""
    loss = PolicyLoss(ratio="sequence")
    label, lp, ent, att = _cases()[2]                               # target 0: r = 1
    ref = Q.seq_ref(loss, lp, ent, att, as_fp32=False)
    assert abs(ref["r"] - 1.0) < 1e-12 and not ref["clipped"].any()
    val, g, _ = _definition(loss, lp, ent, att)
    m = att["loss_mask"]
    assert (g[~m] == 0).all() and np.ptp(g[m]) <= 1e-15 and abs(g[m][0] - ref["c"]) <= REL * abs(ref["c"]) and ref["c"] != 0
    assert abs(val - _definition(PolicyLoss(), lp, ent, att)[0]) > 1e-3


def test_on_policy_ratio_is_one_and_the_gradient_as_if_old_were_detached():
    loss = PolicyLoss(clip_low=0.2, clip_high=0.2, ratio="sequence")
    _, lp, ent, att = [c for c in _cases() if c[0] == "on policy"][0]
    ref = Q.seq_ref(loss, lp, ent, att, as_fp32=False)
    A, m = att["advantages"], att["loss_mask"].astype(np.float64)
    assert ref["r"] == 1.0 and ref["margin"] == np.inf and not ref["clipped"].any()
    val, g, _ = _definition(loss, lp, ent, att)
    w = 1.0 / m.sum()
    assert abs(val - w * (m * -A).sum()) <= REL and np.abs(g - w / m.sum() * (m * -A).sum() * m).max() <= REL
    same = _definition(loss, lp, ent, {**att, "old_logprobs": lp.copy()})
    assert same[0] == val and np.array_equal(same[1], g)


def test_all_masked_and_two_token_sequences():
    loss = PolicyLoss(kl_coef=0.1, entropy_coef=0.1, ratio="sequence")
    _, lp, ent, att = [c for c in _cases() if c[0] == "all masked"][0]
    val, g, ge = _definition(loss, lp, ent, att)
    assert val == 0.0 and (g == 0).all() and (ge == 0).all()        # n^ = max(0, 1) = 1, r = exp(0) = 1, every term masked
    assert Q.seq_ref(loss, lp, ent, att)["r"] == 1.0
    # one prediction: the sequence ratio IS the token ratio, so both objectives agree wherever the token is not clipped
    _, lp1, ent1, att1 = [c for c in _cases() if c[0] == "one prediction"][0]
    att1 = {**att1, "old_logprobs": lp1 - 0.05}
    a, b = _definition(loss, lp1, ent1, att1), _definition(PolicyLoss(kl_coef=0.1, entropy_coef=0.1), lp1, ent1, att1)
    assert abs(a[0] - b[0]) <= REL * abs(b[0]) and np.abs(a[1] - b[1]).max() <= REL * np.abs(b[1]).max()
    ref = Q.seq_ref(loss, lp1, ent1, att1, as_fp32=False)
    assert abs(a[0] - ref["loss"]) <= REL * abs(ref["loss"]) and abs(ref["r"] - np.exp(0.05)) < 1e-12


@pytest.mark.parametrize("cfg", list(R.CONFIGS()))
def test_token_objects_give_the_same_numbers_as_before(cfg):
    """ratio="token" is the default and changes nothing: bit-equal to the object built without the keyword, and equal to the token-level
    closed form of policy_loss_ref64."""
    base = R.CONFIGS()[cfg]
    assert base.ratio == "token"
    kw = {k: getattr(base, k) for k in ("clip_low", "clip_high", "dual_clip", "kl_coef", "kl_estimator", "entropy_coef", "agg", "scale")}
    explicit = PolicyLoss(**kw, ratio="token")
    for label, lp, ent, att in _cases():
        a, b = _definition(base, lp, ent, att), _definition(explicit, lp, ent, att)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (cfg, label)
        ref = R.seq_ref(base, lp, ent, att, as_fp32=False)
        mag = float(ref["mag_loss_lp"].sum() + ref["mag_loss_ent"].sum())
        assert abs(a[0] - ref["loss"]) <= REL * max(mag, 1e-300), (cfg, label)
        assert np.abs(a[1] - ref["g_lp"]).max() <= REL * max(float(ref["mag_g_lp"].max(initial=0.0)), 1e-300), (cfg, label)


def test_ratio_is_an_enumerant_and_shows_in_repr():
    assert losses.RATIOS == ("token", "sequence") and "RATIOS" in losses.__all__
    for bad in ("seq", "tokens", None, 1):
        with pytest.raises(ValueError, match="ratio"):
            PolicyLoss(ratio=bad)
    assert "ratio='sequence'" in repr(PolicyLoss(ratio="sequence")) and "ratio='token'" in repr(PolicyLoss())
    assert PolicyLoss(0.2, 0.2, None, 0.0, "k3", 0.0, "seq_mean", 1.0, "sequence").ratio == "sequence"      # the last positional argument


# ---- the host tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Q.TRIES))
def test_path_tables_equal_the_walk_of_every_root_path(name):
    plan, att_lens, depth, n_real = Q.build(name)
    run_ptr, row0, depth0, seq_leaf = packing.policy_path_tables(plan, Q.attach_lists_of(att_lens))
    M, S = len(att_lens), sum(map(len, att_lens))
    assert run_ptr.dtype == row0.dtype == depth0.dtype == seq_leaf.dtype == np.int32
    assert run_ptr.shape == (M + 1,) and seq_leaf.shape == (S,) and row0.shape == depth0.shape == (int(run_ptr[-1]),)
    assert seq_leaf.tolist() == [i for i, leaf in enumerate(att_lens) for _ in leaf]
    paths = Q.paths_of(plan, att_lens)
    for s, rows in enumerate(paths):
        leaf = int(seq_leaf[s])
        k0, k1 = int(run_ptr[leaf]), int(run_ptr[leaf + 1])
        assert k1 > k0 and depth0[k0] == 0 and (np.diff(depth0[k0:k1]) > 0).all()
        got = []
        for k in range(k0, k1):                                    # the walk the kernel does: depths [depth0[k], next run's depth0) of run k
            end = int(depth0[k + 1]) if k + 1 < k1 else rows.size
            got += [int(row0[k]) + d - int(depth0[k]) for d in range(int(depth0[k]), min(end, rows.size))]
        assert got == rows.tolist(), (name, s)
        assert (depth[rows] == np.arange(rows.size)).all()
    if name == "filler":
        assert plan.M == M + 1 and int(row0.max()) < n_real            # the filler segment is no leaf and in no path
    with pytest.raises(ValueError, match="attach lists"):
        packing.policy_path_tables(plan, Q.attach_lists_of(att_lens)[:-1] if M > 1 else [])


def test_the_new_tries_are_the_ones_asked_for():
    plan, att, _, _ = Q.build("long_path")
    run_ptr, row0, depth0, seq_leaf = packing.policy_path_tables(plan, Q.attach_lists_of(att))
    assert run_ptr[3] - run_ptr[2] >= 3 and max(att[2]) - 1 > 256 and plan.T - row0[run_ptr[3] - 1] > 256
    plan, att, _, n_real = Q.build("many_seqs")
    assert sum(map(len, att)) > 2048 and plan.T > n_real
    lens, lcp, att = R.TRIES["folded"]
    with pytest.raises(ValueError, match="longer"):
        packing.policy_path_tables(packing.plan_segments(lens, lcp), Q.attach_lists_of([[3, 5, 8], [6], [5, 5]]))


def test_the_inputs_keep_every_sequence_ratio_off_the_edges():
    for name in ("folded", "fan70", "long_path"):
        for cfg, loss in Q.SEQ_CONFIGS().items():
            plan, att_lens, depth, n_real, lp, ent, atts = Q.make_inputs(name, seed=3)
            seen = set()
            for s, (rows, att) in enumerate(zip(Q.paths_of(plan, att_lens), atts)):
                r = Q.seq_ref(loss, lp[rows[1:]], ent[rows], att)
                assert r["margin"] >= 1e-3, (name, cfg, s)
                if att["loss_mask"].any():
                    assert abs(np.log(r["r"]) - Q.TARGETS[s % 6]) < 1e-5
                    seen.add(s % 6)
                x = lp[rows[1:]].astype(np.float64) - att["old_logprobs"]
                assert np.abs(x).max(initial=0.0) < 8.0
            assert len(seen) >= min(6, len(atts) - 1)
    assert max(float(np.abs(lp[rows[1:]] - a["old_logprobs"]).max()) for rows, a in zip(Q.paths_of(plan, att_lens), atts)) > 2.5


# ---- rows against sequences ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [("folded", "dual_k3"), ("empty_segments", "ppo"), ("fan70", "k1_sum"), ("filler", "ppo"), ("long_path", "dual_k3")])
def test_row_sums_equal_the_definition_per_sequence(name, cfg):
    """dlp[t] = sum over the sequences through row t (the row tables' range, n_s >= depth) of c_s m + w_s m kl_coef dkl - the kernel's
    row pass, in float64 - = the definition called once per sequence on its gathered path, differentiated by autograd and scattered."""
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), ref = Q.case(name, cfg, seed=3)
    assert ref["margin"] >= 1e-3
    a = torch.from_numpy(lp.astype(np.float64)).requires_grad_(True)
    e = torch.from_numpy(ent.astype(np.float64)).requires_grad_(True)
    fp32_loss = PolicyLoss(**{k: (None if getattr(loss, k) is None else float(np.float32(getattr(loss, k))))
                              for k in ("clip_low", "clip_high", "dual_clip", "kl_coef", "entropy_coef", "scale")},
                           kl_estimator=loss.kl_estimator, agg=loss.agg, ratio="sequence")
    total = 0.0
    for rows, att in zip(Q.paths_of(plan, att_lens), atts):
        rows = torch.from_numpy(rows)
        total = total + fp32_loss(a[rows[1:]], e[rows], _t(att))
    total.backward()
    assert abs(total.item() - ref["stats"][0]) <= 1e-11 * max(abs(ref["stats"][0]), 1.0)
    assert np.abs(a.grad.numpy() - ref["dlp"]).max() <= 1e-11 * np.abs(ref["dlp"]).max()
    ge = np.zeros(plan.T) if e.grad is None else e.grad.numpy()
    assert np.abs(ge - ref["dent"]).max() <= 1e-11 * max(np.abs(ref["dent"]).max(), 1e-300)
    assert (ref["dlp"][n_real:] == 0).all() and (ref["dent"][n_real:] == 0).all()
    # the same sum, driven by the row tables instead of the paths
    lo, hi, seq_ptr, seq_lens = packing.policy_row_tables(plan, Q.attach_lists_of(att_lens))
    kc = float(np.float32(loss.kl_coef))
    rows_dlp = np.zeros(plan.T)
    for t in range(plan.T):
        d = int(depth[t])
        for s in range(lo[t], hi[t]):
            if d >= 1 and seq_lens[s] - 1 >= d:
                m = float(atts[s]["loss_mask"][d - 1])
                dd = float(atts[s]["ref_logprobs"][d - 1]) - float(lp[t])
                dkl = 0.0 if kc == 0 else 1.0 if loss.kl_estimator == "k1" else 1.0 - np.exp(dd)
                rows_dlp[t] += ref["c"][s] * m + ref["w"][s] * m * kc * dkl
    assert np.abs(rows_dlp - ref["dlp"]).max() <= 1e-11 * np.abs(ref["dlp"]).max()
