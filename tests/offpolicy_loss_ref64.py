"""Float64 closed form of losses.PolicyLoss with an off-policy correction (a rollout importance weight, truncated or masked, per token
or per sequence) and / or the CISPO surrogate - value, analytic gradients, the eight statistics of losses.OFFPOLICY_STATS - in plain
numpy (no autograd), per sequence and summed over the packed rows of a trie; inputs whose weights and ratios sit away from every branch
edge by construction; and the error bound of the fp32 kernels (dta_policy_loss_ex) against it.  `TRIES`, `build`, `paths_of` and
`attach_lists_of` of policy_loss_ref64 are reused, and the inputs are those of policy_loss_ref64.make_inputs (token ratio) or
seq_policy_loss_ref64.make_inputs (sequence ratio) with `rollout_logprobs` added.

Closed form for one sequence (lp, A, m, old, ref as in losses.py; x_j = lp_j - old_j, n^ = max(sum m, 1), [lo, hi] = [1 - clip_low,
1 + clip_high]; r_j = e^(x_j) or the one r = exp(sum m x / n^) of a sequence-level ratio; old absent: x = 0):
    y_j = old_j - rollout_j   (old absent: lp_j - rollout_j; a constant of the gradient either way)
    rho = e^(y_j) ("token") | exp(sum_j m_j y_j) ("sequence") | exp(sum_j m_j y_j / n^) ("sequence_mean")
    omega = rho, but  "truncate": is_cap where rho > is_cap;   "mask": 0 where rho < is_floor or rho > is_cap;   no correction: 1
    "ppo":    pg, dpg as in policy_loss_ref64 (token ratio) / seq_policy_loss_ref64 (sequence ratio)
    "cispo":  pg = -clamp(r, lo, hi) A lp,  dpg = -clamp(r, lo, hi) A,  "clipped" = r outside [lo, hi]
    token ratio:     dloss/dlp_j = w m_j (omega dpg_j + kl_coef dkl_j)
    sequence ratio:  dloss/dlp_t = c_s m_t + w m_t kl_coef dkl_t,   c_s = w r / n^ * sum_j m_j omega_j (-A_j) [j not clipped]
    loss = sum_j w m_j (omega pg_j + kl_coef kl_j - entropy_coef ent_j)        (KL and entropy never carry omega)
    stats = {loss, sum m omega pg, sum m kl, sum m ent, sum m [clipped], sum m, sum m omega, sum m [omega != rho]}
`margin` is the smallest RELATIVE distance of a rho from is_cap (and from is_floor under "mask") over the masked tokens - for a
sequence-level weight over the sequences with a masked token -, of r from lo and hi for CISPO's count (old given), and the distance of
r from the clip edges as policy_loss_ref64 / seq_policy_loss_ref64 measure it for "ppo".  make_inputs keeps every one of them at
1e-3 or more - the test asserts it -, so fp32 and fp64 take the same branch.

Error bound of the kernels (u = 2^-24, every input an fp32 number, 0/1 masks).  Everything the two existing modules derive holds
unchanged: a term of magnitude |t|^ is off by (C_OPS + amp) u |t|^, C_OPS = 14 roundings, amp = |x| + |d| for a token ratio and
(n + 1) X + (n - 1) for a sequence ratio (X = sum |m x| / n^), and a sum of N terms in any order adds (N - 1) u sum |t|^.  The weight
adds, to every term that holds it:
    per token:     y (1 rounding, u |y|, which the exponential turns into a relative u |y| of rho), the accurate expf (2 u), the product
                   of omega with pg or dpg (1):  amp_w = |y| + 3
    per sequence:  each y_j one rounding, u |y_j|; their masked sum over the n predictions in any order, (n - 1) u sum |m y|; the
                   division by n^ ("sequence_mean") one more, at most u sum |m y| (/ n^) - together an ABSOLUTE (n + 1) u Y of the
                   exponent, Y = sum |m y| ("sequence") or sum |m y| / n^ ("sequence_mean"), which the exponential turns into a relative
                   error of rho; expf 2 u; the product 1:  amp_w = (n + 1) Y + 3
(a truncated weight is is_cap itself and a masked one 0 - both exact; the bound is kept all the same).  CISPO's value holds one more
product, with lp: + 1.  Under a sequence ratio the summands of c_s hold their own omega_j: the largest amp_w of the sequence is taken
for all.  sum m omega is bounded as a sum of terms m omega with (C_OPS + amp_w) u each; the three counts (clipped, masked, altered
weights) are sums of 0/1 values below 2^24 and must be exact.  The per-sequence workspaces: w holds one rounding (2 u |w| is allowed),
omega[s] amp_w u omega, c[s] its term's bound.  A rho below 2^-126 (a denormal, or 0 where float64 still holds 1e-70) is off by less
than the n 2^-126 every bound carries.  Nothing here was measured or tuned."""
import functools

import numpy as np

import policy_loss_ref64 as R
import seq_policy_loss_ref64 as Q

U32, FLOOR, C_OPS = R.U32, R.FLOOR, R.C_OPS
TRIES, build, paths_of, attach_lists_of = R.TRIES, R.build, R.paths_of, R.attach_lists_of
IS_CAP, IS_FLOOR = 2.0, 0.5                       # the edges of every configuration below
Y_TARGETS = (-1.0, -0.2, 0.0, 0.3, 1.0, 0.0)      # masked mean of y of sequence s: Y_TARGETS[s % 6]; e^y = 0.37 .. 2.72, 9 % or more off an edge
OVERFLOW_SEQ, OVERFLOW_SUM = 2, 110.0             # sequence 2 of a trie (if it has one): masked sum of y = 110 > 88.7, expf overflows
NUDGE = 4e-3                                      # a token's rho closer than this (relative) to an edge is moved to 2 NUDGE off it


def CONFIGS():
    """name -> PolicyLoss: the three weight levels x the two modes on a token ratio; two on a sequence ratio; CISPO alone and with a
    token-level truncated weight and a k3 KL term.  The clip edges are among policy_loss_ref64.EDGES."""
    from dynamictreeattn_amd.losses import PolicyLoss
    cap, fl = IS_CAP, IS_FLOOR
    return {
        "tok_trunc": PolicyLoss(is_level="token", is_cap=cap),
        "tok_mask": PolicyLoss(is_level="token", is_mode="mask", is_cap=cap, is_floor=fl, kl_coef=0.1, kl_estimator="k1", agg="token_sum", scale=1.0 / 37,
                               clip_low=0.1, clip_high=0.2),
        "seq_trunc": PolicyLoss(is_level="sequence", is_cap=cap, dual_clip=3.0, entropy_coef=0.01),
        "seq_mask": PolicyLoss(is_level="sequence", is_mode="mask", is_cap=cap, is_floor=fl),
        "mean_trunc": PolicyLoss(is_level="sequence_mean", is_cap=cap, kl_coef=0.2, kl_estimator="k2", entropy_coef=-0.02, scale=2.0),
        "mean_mask": PolicyLoss(is_level="sequence_mean", is_mode="mask", is_cap=cap, is_floor=fl, clip_low=0.2, clip_high=0.28),
        "gspo_tok_trunc": PolicyLoss(ratio="sequence", is_level="token", is_cap=cap, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01),
        "gspo_seq_mask": PolicyLoss(ratio="sequence", is_level="sequence", is_mode="mask", is_cap=cap, is_floor=fl, clip_low=0.2, clip_high=0.28,
                                    dual_clip=3.0),
        "cispo": PolicyLoss(surrogate="cispo"),
        "cispo_tok_trunc_k3": PolicyLoss(surrogate="cispo", is_level="token", is_cap=cap, kl_coef=0.05, kl_estimator="k3"),
    }


def _rel(rho, edge):
    return np.abs(np.asarray(rho, np.float64) / edge - 1.0)


def seq_ref(loss, logprob, entropy, att, as_fp32=True):
    """The closed form for ONE sequence; arguments as policy_loss_ref64.seq_ref, att with `rollout_logprobs` when loss.is_level is set.
    Returns float64 arrays [n] unless noted: value terms `t_pg` (w m omega pg), `t_kl`, `t_ent` (their sum is the loss), gradient parts
    `g_pg`, `g_kl` (their sum is dloss/dlp) and `g_ent`, per-token `pg` (omega pg), `kl`, `m`, `ent`, `omega_j`, `clipped`, `altered`,
    magnitudes `mag_*`, bound factors `k_pg` (value terms), `k_g` (surrogate gradient), `k_kl`, `k_om`, and the scalars `w`, `c`, `omega`
    (the sequence's weight; 1 for none / "token"), `b_c`, `b_omega`, `loss`, `margin`."""
    _f32 = (lambda v: float(np.float32(v))) if as_fp32 else float
    lp = np.asarray(logprob, np.float64)
    n = lp.shape[0]
    ent = np.asarray(entropy, np.float64)[:n]
    A = att["advantages"]
    A = np.full(n, float(A)) if np.ndim(A) == 0 else np.asarray(A, np.float64)
    old = att.get("old_logprobs")
    on_policy = old is None
    old = lp if on_policy else np.asarray(old, np.float64)
    x = lp - old
    m = att.get("loss_mask")
    m = np.ones(n) if m is None else np.asarray(m).astype(np.float64)
    lo, hi = 1.0 - _f32(loss.clip_low), 1.0 + _f32(loss.clip_high)
    c = None if loss.dual_clip is None else _f32(loss.dual_clip)
    kc, ec, scale = _f32(loss.kl_coef), _f32(loss.entropy_coef), _f32(loss.scale)
    cap, floor = _f32(loss.is_cap), _f32(loss.is_floor)
    nm = float(m.sum())
    nh = max(nm, 1.0)
    seq_ratio, cispo = loss.ratio == "sequence", loss.surrogate == "cispo"
    margin = np.inf
    # ---- the ratio and the surrogate
    if seq_ratio:
        r = np.full(n, float(np.exp((m * x).sum() / nh)))
        amp_r = np.full(n, (n + 1) * float(np.abs(m * x).sum() / nh) + (n - 1))
        live = np.full(n, (not on_policy) and bool(((A != 0) & (m != 0)).any()))
    else:
        r, amp_r, live = np.exp(x), np.abs(x), (A != 0) & (not on_policy)
    if cispo:
        rc = np.clip(r, lo, hi)
        pg, dpg, clipped = -rc * A * lp, -rc * A, (r < lo) | (r > hi)
        mag_pg, mag_dpg = np.abs(pg), np.abs(dpg)
        if not on_policy and n:
            margin = min(margin, float(_rel(r, lo).min()), float(_rel(r, hi).min()))
    else:
        clipped = ((r > hi) & (A > 0)) | ((r < lo) & (A < 0))
        pg = np.where(clipped, -np.where(r > hi, hi, lo) * A, -r * A)
        if c is not None:
            dual = (A < 0) & (r > c)
            pg, clipped = np.where(dual, -c * A, pg), clipped | dual
        dpg = np.where(clipped, 0.0, -r * A)
        mag_pg, mag_dpg = np.abs(pg), np.abs(r * A)
        if live.any():
            margin = min([margin] + [float(np.abs(r[live] - e).min()) for e in [lo, hi] + ([c] if c is not None else [])])
    # ---- the rollout importance weight
    omega_s, amp_ws = 1.0, 0.0
    if loss.is_level is None:
        omega, amp_w, altered = np.ones(n), np.zeros(n), np.zeros(n, bool)
    else:
        y = old - np.asarray(att["rollout_logprobs"], np.float64)
        if loss.is_level == "token":
            rho, amp_w, counted = np.exp(y), np.abs(y) + 3.0, m != 0
        else:
            div = nh if loss.is_level == "sequence_mean" else 1.0
            rho = np.full(n, float(np.exp((m * y).sum() / div)))
            amp_w = np.full(n, (n + 1) * float(np.abs(m * y).sum() / div) + 3.0)
            counted = np.full(n, nm > 0)
        if loss.is_mode == "truncate":
            altered = rho > cap
            omega = np.where(altered, cap, rho)
            edges = [cap]
        else:
            altered = (rho < floor) | (rho > cap)
            omega = np.where(altered, 0.0, rho)
            edges = [cap] + ([floor] if floor > 0 else [])
        if counted.any():
            margin = min([margin] + [float(_rel(rho[counted], e).min()) for e in edges])
        if loss.is_level != "token" and n:
            omega_s, amp_ws = float(omega[0]), float(amp_w[0])
    # ---- KL
    kl, dkl, K, D, d = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    if kc != 0:
        d = np.asarray(att["ref_logprobs"], np.float64) - lp
        if loss.kl_estimator == "k1":
            kl, dkl, K, D = -d, np.ones(n), np.abs(d), np.ones(n)
        elif loss.kl_estimator == "k2":
            kl, dkl, K, D = 0.5 * d * d, -d, 0.5 * d * d, np.abs(d)
        else:
            e = np.exp(d)
            kl, dkl, K, D = e - d - 1.0, 1.0 - e, e + np.abs(d) + 1.0, e + 1.0
    w = scale / nh if loss.agg == "seq_mean" else scale
    k_pg = C_OPS + amp_r + amp_w + (1.0 if cispo else 0.0)
    if seq_ratio:
        cs = w * r[0] / nh * float((m * omega * -A)[~clipped].sum()) if n else 0.0
        mag_c = abs(w) * r[0] / nh * float((np.abs(m) * omega * np.abs(A))[~clipped].sum()) if n else 0.0
        g_pg, mag_g_pg = cs * m, mag_c * np.abs(m)
        k_g = np.full(n, C_OPS + (amp_r[0] + float(amp_w.max()) if n else 0.0))
        b_c = U32 * float(k_g[0] if n else C_OPS) * mag_c + FLOOR
    else:
        cs, b_c = 0.0, 0.0
        g_pg, mag_g_pg, k_g = w * m * omega * dpg, abs(w) * np.abs(m) * omega * mag_dpg, k_pg
    out = {"t_pg": w * m * omega * pg, "t_kl": w * m * kc * kl, "t_ent": -w * m * ec * ent,
           "g_pg": g_pg, "g_kl": w * m * kc * dkl, "g_ent": -w * m * ec * np.ones(n),
           "pg": omega * pg, "kl": kl, "m": m, "ent": ent, "omega_j": omega, "clipped": clipped, "altered": altered,
           "mag_t_pg": abs(w) * np.abs(m) * omega * mag_pg, "mag_t_kl": abs(w) * np.abs(m) * abs(kc) * K,
           "mag_t_ent": abs(w) * np.abs(m) * abs(ec) * np.abs(ent),
           "mag_g_pg": mag_g_pg, "mag_g_kl": abs(w) * np.abs(m) * abs(kc) * D, "mag_g_ent": abs(w) * np.abs(m) * abs(ec) * np.ones(n),
           "mag_pg": np.abs(m) * omega * mag_pg, "mag_kl": np.abs(m) * K, "k_pg": k_pg, "k_g": k_g, "k_kl": C_OPS + np.abs(d), "k_om": C_OPS + amp_w,
           "w": w, "c": cs, "omega": omega_s, "b_c": b_c, "b_omega": U32 * amp_ws * omega_s + FLOOR, "margin": margin}
    out["loss"] = float(out["t_pg"].sum() + out["t_kl"].sum() + out["t_ent"].sum())
    return out


def make_inputs(name, seed=0, on_policy=False, scalar_adv=False, seq_ratio=False):
    """The seeded fp32 inputs of policy_loss_ref64.make_inputs (seq_ratio: of seq_policy_loss_ref64.make_inputs, whose sequence ratios
    sit away from the clip edges) with `rollout_logprobs` added to every attachment: y = old - rollout (on_policy: lp - rollout) spreads
    0.8 nats around the masked mean Y_TARGETS[s % 6]; a token whose e^y comes within NUDGE of is_cap or is_floor is moved 2 NUDGE off
    it.  The masked sum of sequence OVERFLOW_SEQ is OVERFLOW_SUM: expf overflows.  Sequence 1 is all-masked (as in the base inputs)."""
    base = (Q if seq_ratio else R).make_inputs(name, seed=seed, on_policy=on_policy, scalar_adv=scalar_adv)
    plan, att_lens, depth, n_real, lp, ent, atts = base
    rng = np.random.default_rng(seed + 1000)
    for s, (rows, a) in enumerate(zip(paths_of(plan, att_lens), atts)):
        n = rows.size - 1
        m = np.asarray(a["loss_mask"], bool)
        y = rng.uniform(-0.8, 0.8, n)
        if m.any():
            y[m] += (OVERFLOW_SUM / m.sum() if s == OVERFLOW_SEQ else Y_TARGETS[s % len(Y_TARGETS)]) - y[m].mean()
        for e in (IS_CAP, IS_FLOOR):
            y = np.where(_rel(np.exp(y), e) < NUDGE, np.log(e * (1.0 + 2 * NUDGE)), y)
        origin = lp[rows[1:]] if on_policy else a["old_logprobs"]
        a["rollout_logprobs"] = (origin.astype(np.float64) - y).astype(np.float32)
    return plan, att_lens, depth, n_real, lp, ent, atts


def trie_ref(loss, plan, att_lens, lp, ent, atts):
    """The closed form summed over packed rows: `dlp`, `dent` (float64 [T]) with bounds `b_dlp`, `b_dent`, `stats` (float64 [8],
    losses.OFFPOLICY_STATS order) with `b_stats` (0 for the three counts), `margin` (the smallest of the sequences'), and the
    per-sequence `w`, `c`, `omega` with `b_w`, `b_c`, `b_omega`."""
    T = plan.T
    lp, ent = np.asarray(lp, np.float64), np.asarray(ent, np.float64)
    dlp, dent = np.zeros(T), np.zeros(T)
    e_lp, e_ent, mag_lp, mag_ent, n_lp, n_ent = (np.zeros(T) for _ in range(6))
    stats, e_st, mag_st, n_st = np.zeros(8), np.zeros(8), np.zeros(8), np.zeros(8)
    margin, per_seq = np.inf, {k: [] for k in ("w", "c", "omega", "b_c", "b_omega")}
    has_kl = float(np.float32(loss.kl_coef)) != 0
    for rows, att in zip(paths_of(plan, att_lens), atts):
        n = rows.size - 1
        r = seq_ref(loss, lp[rows[1:]], ent[rows], att)
        for k in per_seq:
            per_seq[k].append(r[k])
        if n == 0:
            continue
        margin = min(margin, r["margin"])
        a, b = rows[1:], rows[:-1]                    # rows of the log-prob terms (depth j + 1) and of the entropy terms (depth j)
        np.add.at(dlp, a, r["g_pg"] + r["g_kl"]); np.add.at(e_lp, a, r["k_g"] * r["mag_g_pg"] + r["k_kl"] * r["mag_g_kl"])
        np.add.at(mag_lp, a, r["mag_g_pg"] + r["mag_g_kl"]); np.add.at(n_lp, a, 2 if has_kl else 1)
        np.add.at(dent, b, r["g_ent"]); np.add.at(e_ent, b, C_OPS * r["mag_g_ent"]); np.add.at(mag_ent, b, r["mag_g_ent"]); np.add.at(n_ent, b, 1)
        m = r["m"]
        mag_ent_stat, mag_om = np.abs(m) * np.abs(r["ent"]), np.abs(m) * r["omega_j"]
        for k, (val, mag, cc, cnt) in enumerate((
                (r["loss"], r["mag_t_pg"].sum() + r["mag_t_kl"].sum() + r["mag_t_ent"].sum(),
                 (r["k_pg"] * r["mag_t_pg"]).sum() + (r["k_kl"] * r["mag_t_kl"]).sum() + C_OPS * r["mag_t_ent"].sum(), 3 * n),
                ((m * r["pg"]).sum(), r["mag_pg"].sum(), (r["k_pg"] * r["mag_pg"]).sum(), n),
                ((m * r["kl"]).sum(), r["mag_kl"].sum(), (r["k_kl"] * r["mag_kl"]).sum(), n),
                ((m * r["ent"]).sum(), mag_ent_stat.sum(), C_OPS * mag_ent_stat.sum(), n),
                ((m * r["clipped"]).sum(), 0.0, 0.0, 0), (m.sum(), 0.0, 0.0, 0),
                ((m * r["omega_j"]).sum(), mag_om.sum(), (r["k_om"] * mag_om).sum(), n),
                ((m * r["altered"]).sum(), 0.0, 0.0, 0))):
            stats[k] += val; mag_st[k] += mag; e_st[k] += cc; n_st[k] += cnt
    bound = lambda e, mag, n: U32 * (e + np.maximum(n - 1, 0) * mag) + n * FLOOR
    out = {"dlp": dlp, "dent": dent, "b_dlp": bound(e_lp, mag_lp, n_lp), "b_dent": bound(e_ent, mag_ent, n_ent), "stats": stats,
           "b_stats": bound(e_st, mag_st, n_st), "margin": margin}
    out.update({k: np.asarray(v) for k, v in per_seq.items()})
    out["b_w"] = 2 * U32 * np.abs(out["w"])
    return out


@functools.lru_cache(maxsize=None)
def case(name, cfg, seed=0, on_policy=False, scalar_adv=False):
    """(loss, inputs of make_inputs, trie_ref of them), made once per process and shared: treat as read-only"""
    loss = CONFIGS()[cfg]
    inputs = make_inputs(name, seed=seed, on_policy=on_policy, scalar_adv=scalar_adv, seq_ratio=loss.ratio == "sequence")
    plan, att_lens, depth, n_real, lp, ent, atts = inputs
    return loss, inputs, trie_ref(loss, plan, att_lens, lp, ent, atts)
