"""Float64 closed form of losses.PolicyLoss(ratio="sequence") - the GSPO objective: value, analytic gradients, statistics - in plain
numpy (no autograd), per sequence and summed over the packed rows of a trie; inputs whose sequence ratios sit away from every branch
edge by construction; two more hand-made tries; and the error bound of the fp32 kernels (dta_policy_loss_seq) against it.  The tries,
`build`, `paths_of` and `attach_lists_of` of policy_loss_ref64 are reused.

Closed form for one sequence (lp, A, m, old, ref as in losses.py; x_j = lp_j - old_j, n^ = max(sum m, 1), [lo, hi] = [1 - clip_low,
1 + clip_high], dual clip c):
    r = exp(sum_j m_j x_j / n^)                      one ratio for the whole sequence; old absent: r = 1
    token j is clipped  iff  (r > hi and A_j > 0) or (r < lo and A_j < 0) or (c given, A_j < 0 and r > c)
    pg_j = -r A_j where not clipped, else -hi A_j | -lo A_j | -c A_j
    dr/dlp_t = r m_t / n^, so   d/dlp_t sum_j w m_j pg_j = c_s m_t,   c_s = w r / n^ * sum_j m_j (-A_j) [j not clipped]
    dloss/dlp_t = c_s m_t + w m_t kl_coef dkl_t;   dloss/dentropy_t = -w m_t entropy_coef      (KL and entropy as in policy_loss_ref64)
`margin` is the distance of r from the nearest of lo, hi and c (old given and some masked token with A != 0; else inf).  The tests
assert it >= 1e-3 for every sequence: make_inputs places each sequence's masked mean log-ratio on one of TARGETS, whose ratios are at
least 0.05 from every edge of SEQ_CONFIGS.

Error bound of the kernels (u = 2^-24, every input an fp32 number, 0/1 masks so that mask sums and products are exact).
The exponent e = sum_j m_j x_j / n^: each x_j = lp - old carries one rounding, u |x_j|, m_j x_j none; their sum over the n predictions
of the sequence, in any order, adds at most (n - 1) u sum |m x| (each partial sum is rounded once and never exceeds sum |m x|); the
division by n^ one more, u |e| <= u sum |m x| / n^.  With X = sum_j |m_j x_j| / n^ the exponent is off by at most (n + 1) u X
ABSOLUTELY, which the exponential turns into a RELATIVE error of r, on top of the 2 u of the accurate expf.  That error enters every
term of the sequence that holds r - the new ingredient against the token-level bound, where a token's ratio saw its own x alone.
Then c_s = w r / n^ * G: w = scale / n^ (1 rounding), two products and a division (3), G = sum_j m_j (-A_j) over the unclipped tokens
(no rounding per term, at most (n - 1) u sum m |A| for the summation), and c_s m_t is exact: 6 roundings, well inside the C_OPS = 14 of
policy_loss_ref64, which is kept for every term so that one constant serves.  Hence a surrogate term t - c_s m_t in dlp, w m_j pg_j in
the loss, m_j pg_j in sum_pg - of magnitude |t|^ (|w| r / n^ sum_j m_j |A_j| [unclipped] * m_t, resp. |w| m_j |pg_j|, m_j |pg_j|) is
off by at most
    (C_OPS + (n + 1) X + (n - 1)) u |t|^ = (C_OPS + amp_s) u |t|^
(for the value terms the (n - 1) is the in-sequence summation of m pg; a clipped pg_j holds no r and is bounded all the same).  The KL
and entropy terms are the token-level ones: (C_OPS + |d|) u |t|^ and C_OPS u |t|^.  A row of dlp sums one surrogate and one KL term per
sequence through it; a sum of N terms in ANY order adds at most (N - 1) u sum |t|^.  So, as in policy_loss_ref64,
    |got - ref| <= u sum_i (k_i + N - 1) |t_i|^ + N 2^-126
per element of dlp / dent (N = the terms of that row) and per statistic (N = all its terms); the counts (clipped tokens, masked
tokens) are sums of 0/1 values below 2^24 and must be exact.  Second-order terms are dropped.  Nothing here was fitted to the kernels'
observed error."""
import functools

import numpy as np

import policy_loss_ref64 as R
from dynamictreeattn_amd import packing

U32, FLOOR, C_OPS = R.U32, R.FLOOR, R.C_OPS
paths_of, attach_lists_of = R.paths_of, R.attach_lists_of
TARGETS = (-0.6, -0.05, 0.0, 0.05, 0.6, 1.3)      # masked mean log-ratio of sequence s: TARGETS[s % 6]; ratios 0.549 .. 3.67

TRIES = dict(R.TRIES)
# one sequence of 519 predictions over 3 separate row runs (100 + 100 + 320 rows): the workgroup's stride loop repeats inside the last
# run and the run walk takes three steps; a twin of it and shorter sequences that end inside the first and the second run
TRIES["long_path"] = ([150, 250, 520], [100, 200], [[150, 60], [250, 120], [520, 520]])
# more sequences than the sequence pass has workgroups (2048): its grid stride repeats; all of them pass through the root row
TRIES["many_seqs"] = ([3] * 2100, [1] * 2099, [[3]] * 2100)
NEW_TRIES = ("long_path", "many_seqs")


def build(name):
    """policy_loss_ref64.build, for the two tries of this module as well"""
    if name in R.TRIES:
        return R.build(name)
    lens, lcp, att = TRIES[name]
    plan = packing.plan_segments(lens, lcp)
    n_real = plan.T
    if plan.T >= 2048 and plan.T % 256:
        plan = packing.pad_plan(plan, 256)
    seg = np.repeat(np.arange(plan.M), np.diff(plan.seg_off))
    depth = (plan.seg_depth0[seg] + np.arange(plan.T) - plan.seg_off[seg]).astype(np.int32)
    return plan, att, depth, n_real


def SEQ_CONFIGS():
    """plain; dual clip + k3 + entropy; token_sum + k1 - the hyper-parameters of policy_loss_ref64.CONFIGS, sequence-level"""
    from dynamictreeattn_amd.losses import PolicyLoss
    return {
        "ppo": PolicyLoss(ratio="sequence"),
        "dual_k3": PolicyLoss(clip_low=0.2, clip_high=0.28, dual_clip=3.0, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01, ratio="sequence"),
        "k1_sum": PolicyLoss(clip_low=0.1, clip_high=0.2, kl_coef=0.1, kl_estimator="k1", agg="token_sum", scale=1.0 / 37, ratio="sequence"),
    }


def seq_ref(loss, logprob, entropy, att, as_fp32=True):
    """The closed form for ONE sequence; arguments as policy_loss_ref64.seq_ref.  Returns float64 arrays [n] unless noted: value terms
    `t_pg` (w m pg), `t_kl`, `t_ent` (their sum is the loss), gradients `g_lp`, `g_ent`, per-token `pg`, `kl`, `m`, `clipped`, `ent`,
    magnitudes `mag_*`, `amp_kl` = |d|, and the scalars `r`, `c`, `w`, `loss`, `margin`, `amp` (the amp_s of the module docstring)."""
    _f32 = (lambda v: float(np.float32(v))) if as_fp32 else float
    lp = np.asarray(logprob, np.float64)
    n = lp.shape[0]
    ent = np.asarray(entropy, np.float64)[:n]
    A = att["advantages"]
    A = np.full(n, float(A)) if np.ndim(A) == 0 else np.asarray(A, np.float64)
    old = att.get("old_logprobs")
    on_policy = old is None
    x = np.zeros(n) if on_policy else lp - np.asarray(old, np.float64)
    m = att.get("loss_mask")
    m = np.ones(n) if m is None else np.asarray(m).astype(np.float64)
    lo, hi = 1.0 - _f32(loss.clip_low), 1.0 + _f32(loss.clip_high)
    c = None if loss.dual_clip is None else _f32(loss.dual_clip)
    kc, ec, scale = _f32(loss.kl_coef), _f32(loss.entropy_coef), _f32(loss.scale)
    nh = max(float(m.sum()), 1.0)
    r = float(np.exp((m * x).sum() / nh))
    X = float(np.abs(m * x).sum() / nh)
    bound_of = np.where(A > 0, hi, lo)
    clipped = ((r > hi) & (A > 0)) | ((r < lo) & (A < 0))
    pg = np.where(clipped, -bound_of * A, -r * A)
    if c is not None:
        dual = (A < 0) & (r > c)
        pg = np.where(dual, -c * A, pg)
        clipped = clipped | dual
    edges = [lo, hi] + ([c] if c is not None else [])
    live = (not on_policy) and bool(((A != 0) & (m != 0)).any())
    margin = min(abs(r - e) for e in edges) if live else np.inf
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
    cs = w * r / nh * float((m * -A)[~clipped].sum())
    mag_c = abs(w) * r / nh * float((np.abs(m) * np.abs(A))[~clipped].sum())
    out = {"t_pg": w * m * pg, "t_kl": w * m * kc * kl, "t_ent": -w * m * ec * ent,
           "g_lp": cs * m + w * m * kc * dkl, "g_ent": -w * m * ec * np.ones(n), "pg": pg, "kl": kl, "m": m, "clipped": clipped, "ent": ent,
           "mag_t_pg": abs(w) * np.abs(m) * np.abs(pg), "mag_t_kl": abs(w) * np.abs(m) * abs(kc) * K, "mag_t_ent": abs(w) * np.abs(m) * abs(ec) * np.abs(ent),
           "mag_g_pg": mag_c * np.abs(m), "mag_g_kl": abs(w) * np.abs(m) * abs(kc) * D, "mag_g_ent": abs(w) * np.abs(m) * abs(ec) * np.ones(n),
           "mag_pg": np.abs(m) * np.abs(pg), "mag_kl": np.abs(m) * K, "amp_kl": np.abs(d),
           "r": r, "c": cs, "w": w, "margin": margin, "amp": (n + 1) * X + (n - 1)}
    out["loss"] = float(out["t_pg"].sum() + out["t_kl"].sum() + out["t_ent"].sum())
    return out


def make_inputs(name, seed=0, spread=3.0, on_policy=False, scalar_adv=False):
    """Seeded fp32 inputs of a trie, as policy_loss_ref64.make_inputs makes them (per-token log-ratios spread up to `spread` nats, a
    mask with zeros, the second sequence all-masked, advantages of both signs and exact zeros) - but the masked tokens' old log-probs
    of sequence s are shifted so that their mean log-ratio is TARGETS[s % 6]: the sequence ratio is away from every edge by
    construction."""
    plan, att_lens, depth, n_real = build(name)
    rng = np.random.default_rng(seed)
    T = plan.T
    lp = (-rng.uniform(0.05, 6.0, T)).astype(np.float32)
    ent = rng.uniform(0.0, 5.0, T).astype(np.float32)
    atts = []
    for s, rows in enumerate(paths_of(plan, att_lens)):
        n = rows.size - 1
        mine = lp[rows[1:]].astype(np.float64)
        x = rng.uniform(-spread, spread, n) * (rng.random(n) < 0.5) + rng.uniform(-0.15, 0.15, n)
        adv = rng.normal(0, 1.5, n)
        adv[rng.random(n) < 0.1] = 0.0
        m = (rng.random(n) < 0.8)
        if s == 1:
            m[:] = False
        if m.any():
            x[m] += TARGETS[s % len(TARGETS)] - x[m].mean()
        a = {"advantages": float(rng.normal()) if scalar_adv else adv.astype(np.float32),
             "ref_logprobs": (mine + rng.uniform(-spread, spread, n)).astype(np.float32), "loss_mask": m}
        if not on_policy:
            a["old_logprobs"] = (mine - x).astype(np.float32)
        atts.append(a)
    return plan, att_lens, depth, n_real, lp, ent, atts


def trie_ref(loss, plan, att_lens, lp, ent, atts):
    """The closed form summed over packed rows: `dlp`, `dent` (float64 [T]) with bounds `b_dlp`, `b_dent`, `stats` (float64 [6],
    losses.STATS order) with `b_stats`, `margin` (the smallest of the sequences') and the per-sequence `r`, `c`, `w`."""
    T = plan.T
    lp, ent = np.asarray(lp, np.float64), np.asarray(ent, np.float64)
    dlp, dent = np.zeros(T), np.zeros(T)
    e_lp, e_ent, mag_lp, mag_ent, n_lp, n_ent = (np.zeros(T) for _ in range(6))
    stats, e_st, mag_st, n_st = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6)
    margin, rs, cs, ws = np.inf, [], [], []
    has_kl = float(np.float32(loss.kl_coef)) != 0
    for rows, att in zip(paths_of(plan, att_lens), atts):
        n = rows.size - 1
        r = seq_ref(loss, lp[rows[1:]], ent[rows], att)
        rs.append(r["r"]); cs.append(r["c"]); ws.append(r["w"])
        if n == 0:
            continue
        margin = min(margin, r["margin"])
        k_pg, k_kl = C_OPS + r["amp"], C_OPS + r["amp_kl"]
        a, b = rows[1:], rows[:-1]                    # rows of the log-prob terms (depth j + 1) and of the entropy terms (depth j)
        np.add.at(dlp, a, r["g_lp"]); np.add.at(e_lp, a, k_pg * r["mag_g_pg"] + k_kl * r["mag_g_kl"])
        np.add.at(mag_lp, a, r["mag_g_pg"] + r["mag_g_kl"]); np.add.at(n_lp, a, 2 if has_kl else 1)
        np.add.at(dent, b, r["g_ent"]); np.add.at(e_ent, b, C_OPS * r["mag_g_ent"]); np.add.at(mag_ent, b, r["mag_g_ent"]); np.add.at(n_ent, b, 1)
        m = r["m"]
        mag_ent_stat = np.abs(m) * np.abs(r["ent"])
        for k, (val, mag, cc, cnt) in enumerate((
                (r["loss"], r["mag_t_pg"].sum() + r["mag_t_kl"].sum() + r["mag_t_ent"].sum(),
                 k_pg * r["mag_t_pg"].sum() + (k_kl * r["mag_t_kl"]).sum() + C_OPS * r["mag_t_ent"].sum(), 3 * n),
                ((m * r["pg"]).sum(), r["mag_pg"].sum(), k_pg * r["mag_pg"].sum(), n),
                ((m * r["kl"]).sum(), r["mag_kl"].sum(), (k_kl * r["mag_kl"]).sum(), n),
                ((m * r["ent"]).sum(), mag_ent_stat.sum(), C_OPS * mag_ent_stat.sum(), n),
                ((m * r["clipped"]).sum(), 0.0, 0.0, 0), (m.sum(), 0.0, 0.0, 0))):
            stats[k] += val; mag_st[k] += mag; e_st[k] += cc; n_st[k] += cnt
    bound = lambda e, mag, n: U32 * (e + np.maximum(n - 1, 0) * mag) + n * FLOOR
    return {"dlp": dlp, "dent": dent, "b_dlp": bound(e_lp, mag_lp, n_lp), "b_dent": bound(e_ent, mag_ent, n_ent), "stats": stats,
            "b_stats": bound(e_st, mag_st, n_st), "margin": margin, "r": np.asarray(rs), "c": np.asarray(cs), "w": np.asarray(ws)}


@functools.lru_cache(maxsize=None)
def case(name, cfg, seed=0, on_policy=False, scalar_adv=False):
    """(loss, inputs of make_inputs, trie_ref of them), made once per process and shared: treat as read-only"""
    loss = SEQ_CONFIGS()[cfg]
    inputs = make_inputs(name, seed=seed, on_policy=on_policy, scalar_adv=scalar_adv)
    plan, att_lens, depth, n_real, lp, ent, atts = inputs
    return loss, inputs, trie_ref(loss, plan, att_lens, lp, ent, atts)
