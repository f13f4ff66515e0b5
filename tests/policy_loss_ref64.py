"""Float64 closed form of losses.PolicyLoss - value, analytic gradients, statistics - in plain numpy (no autograd), per sequence and
summed over the packed rows of a trie; the hand-made tries and inputs the policy-loss tests share; and the error bound of the fp32
kernel (dta_policy_loss) against it.

Closed form, per prediction j of a sequence (lp = logprob[j], A, m, old, ref as in losses.py; x = lp - old, r = e^x, d = ref - lp):
    inside the clip range [lo, hi] = [1 - clip_low, 1 + clip_high]:  pg = -r A,  dpg/dlp = -r A
    r > hi:  A > 0: pg = -hi A, dpg = 0 (clipped);   A <= 0: pg = -r A, dpg = -r A
    r < lo:  A < 0: pg = -lo A, dpg = 0 (clipped);   A >= 0: pg = -r A, dpg = -r A
    dual clip c, A < 0, r > c:  pg = -c A, dpg = 0 (clipped)
    kl, dkl/dlp:  k1: -d, 1;   k2: d^2 / 2, -d;   k3: e^d - d - 1, 1 - e^d
    dloss/dlp[j] = w m (dpg + kl_coef dkl);   dloss/dentropy[j] = -w m entropy_coef (j < len - 1), 0 for entropy[len - 1]
`margin` is the distance of r from the nearest of lo, hi and c over the predictions whose branch depends on it (A != 0, old given): the
tests assert it >= 1e-3, so that fp32 and fp64 take the same branch.  The hyper-parameters are taken as the fp32 numbers the kernel is
handed (np.float32(clip_low), ...): their conversion is no error of the kernel.

Error bound of the kernel (u = 2^-24, every input an fp32 number).  Per log-prob term the kernel performs, in fp32: x = lp - old (1
rounding; its error u |x| is amplified by the exponential into a relative u |x| of r), r = expf(x) (accurate expf: <= 1 ulp = 2 u),
-r A (1), and under a KL term d = ref - lp (1, amplified likewise into u |d| of e^d), expf(d) (2), 1 - e^d or the like (1), kl_coef dkl
(1), the sum with dpg (1); the clip bounds 1 -+ clip (1); then w = scale / max(sum m, 1) (1: the mask sum of a 0/1 mask is exact), w m
(1), the product with the term (1) - at most 14 roundings, so a term t of magnitude |t|^ (the same expression with every summand
replaced by its absolute value: |w m| (|r A| + |kl_coef| D), D = 1 | |d| | e^d + 1) is off by at most (14 + |x| + |d|) u |t|^.  The
value terms are bounded the same way with K = |d| | d^2 / 2 | e^d + |d| + 1 for the KL summand (k3 cancels: its error scales with the
operands, not with the result).  A sum of n such terms in ANY order adds at most (n - 1) u sum |t|^ (each partial sum is rounded once
and never exceeds sum |t|^) - the summation depth, taken at its worst so that no mapping of rows to lanes has to be assumed.  So
    |got - ref| <= u sum_i (14 + |x_i| + |d_i| + n - 1) |t_i|^ + n 2^-126
for every element of dlp and dent (n = the terms of that row) and for every statistic (n = all its terms); the two counts (clipped
tokens, masked tokens) are sums of 0/1 values below 2^24 and must be exact.  Second-order terms (u^2) are dropped; they are nine
orders below."""
import numpy as np

from dynamictreeattn_amd import packing

U32 = 2.0 ** -24
FLOOR = 2.0 ** -126
C_OPS = 14.0


def seq_ref(loss, logprob, entropy, att, as_fp32=True):
    """The closed form for ONE sequence.  logprob [n], entropy [n + 1] (or [n]: the last element is not used), att: advantages (float or
    [n]), old_logprobs, ref_logprobs, loss_mask ([n] or absent / None).  `loss`: anything with PolicyLoss's attributes.  Returns a dict of
    float64 arrays [n] unless noted: value terms `t_loss_lp`, `t_loss_ent` (their sum over j is the loss), gradients `g_lp`, `g_ent`,
    per-token `pg`, `kl`, `m`, `clipped` (bool), magnitudes `mag_*` and amplification `amp` = |x| + |d|, scalars `w`, `loss`, `margin`.
    as_fp32: take the hyper-parameters as the fp32 numbers the kernel is handed (False: as the doubles PolicyLoss.__call__ computes with)."""
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
    r = np.exp(x)
    pg, dpg = -r * A, -r * A
    clipped = ((r > hi) & (A > 0)) | ((r < lo) & (A < 0))
    pg = np.where(clipped, -np.where(r > hi, hi, lo) * A, pg)
    if c is not None:
        dual = (A < 0) & (r > c)
        pg = np.where(dual, -c * A, pg)
        clipped = clipped | dual
    dpg = np.where(clipped, 0.0, dpg)
    edges = [lo, hi] + ([c] if c is not None else [])
    live = (A != 0) & (not on_policy)
    margin = min([float(np.abs(r[live] - e).min()) for e in edges]) if live.any() else np.inf
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
    w = scale / max(float(m.sum()), 1.0) if loss.agg == "seq_mean" else scale
    out = {"t_loss_lp": w * m * (pg + kc * kl), "t_loss_ent": -w * m * ec * ent, "g_lp": w * m * (dpg + kc * dkl),
           "g_ent": -w * m * ec * np.ones(n), "pg": pg, "kl": kl, "m": m, "clipped": clipped, "ent": ent,
           "mag_loss_lp": abs(w) * np.abs(m) * (np.abs(pg) + abs(kc) * K), "mag_loss_ent": abs(w) * np.abs(m) * abs(ec) * np.abs(ent),
           "mag_g_lp": abs(w) * np.abs(m) * (np.abs(r * A) + abs(kc) * D), "mag_g_ent": abs(w) * np.abs(m) * abs(ec) * np.ones(n),
           "mag_pg": np.abs(m) * np.abs(pg), "mag_kl": np.abs(m) * K, "amp": np.abs(x) + np.abs(d), "w": w, "margin": margin}
    out["loss"] = float(out["t_loss_lp"].sum() + out["t_loss_ent"].sum())
    return out


# ---- hand-made tries ----------------------------------------------------------------------------------------------------------
# name -> (lens, lcp_lens, per-leaf lists of sequence lengths in attach-list order): what packing.plan_segments and TokenTrie.attach_lists
# hold, written by hand.  No token ids are needed: the objective sees rows, depths and lengths only.
def _fan(n_seq, prefix=3, tail=2, dup_every=0):
    """n_seq short sequences that share a `prefix`-token start: more sequences through the root rows than one wave (64) / workgroup (256)"""
    lens = [prefix + tail + (i % 3) for i in range(n_seq)]
    folded = [[lens[i]] * (2 if dup_every and i % dup_every == 0 else 1) for i in range(n_seq)]
    return lens, [prefix] * (n_seq - 1), folded


def _big(n_leaf=75, prefix=30, tail=52):
    """T >= 2048 and T % 256 != 0: filler rows exist.  Leaf i forks off leaf i - 1 at depth prefix + (7 i) % tail."""
    lens = [prefix + tail + (i % 5) for i in range(n_leaf)]
    lcp = [prefix + (7 * i) % tail for i in range(1, n_leaf)]
    return lens, lcp, [[lens[i] - 4, lens[i]] if i % 4 == 0 else [lens[i]] for i in range(n_leaf)]


TRIES = {
    # leaf 0 carries two shorter sequences, the first ending exactly at the fork (depth 3) of leaf 1; leaf 2 twice the same sequence
    "folded": ([7, 6, 5], [3, 1], [[3, 5, 7], [6], [5, 5]]),
    "twins": ([4], [], [[4, 4]]),
    "fork_at_1": ([3, 4, 2], [1, 1], [[3], [2, 4], [2]]),
    "single_len2": ([2], [], [[2]]),
    "empty_segments": ([6, 3, 2, 5], [3, 2, 1], [[6], [3], [2, 2], [1, 5]]),     # leaves 1 and 2 are prefixes of leaf 0: their segments are empty
    "fan70": _fan(70, dup_every=5),
    "fan300": _fan(300),
    "past_block": ([200, 60], [3], [[200], [60]]),                               # T = 257: one row past a 256-row workgroup
    "filler": _big(),
}


def build(name):
    """(plan - padded as _PackedTrie pads it -, attach_lens, depth int32 [T], n_real_rows)"""
    lens, lcp, att = TRIES[name]
    plan = packing.plan_segments(lens, lcp)
    n_real = plan.T
    if plan.T >= 2048 and plan.T % 256:
        plan = packing.pad_plan(plan, 256)
    seg = np.repeat(np.arange(plan.M), np.diff(plan.seg_off))
    depth = (plan.seg_depth0[seg] + np.arange(plan.T) - plan.seg_off[seg]).astype(np.int32)
    return plan, att, depth, n_real


def attach_lists_of(att_lens, attachments=None):
    """per-leaf [(attachment, length), ...] as TokenTrie.attach_lists, the attachments taken in callback order"""
    out, s = [], 0
    for leaf in att_lens:
        out.append([((attachments[s + k] if attachments is not None else {}), n) for k, n in enumerate(leaf)])
        s += len(leaf)
    return out


def paths_of(plan, att_lens):
    """Brute force: for every sequence (callback order) the packed rows of its tokens, depth 0 .. len - 1, by walking its leaf's root path."""
    out = []
    for i, leaf in enumerate(att_lens):
        pieces = [np.arange(b, e) for b, e in plan.path_runs[i]] + [np.arange(plan.seg_off[i], plan.seg_off[i + 1])]
        path = np.concatenate(pieces).astype(np.int64)
        for n in leaf:
            assert n <= path.size
            out.append(path[:n])
    return out


def make_inputs(name, seed=0, spread=3.0, on_policy=False, scalar_adv=False):
    """Seeded fp32 inputs of a trie: lp [T], ent [T] and one attachment per sequence with old / ref up to `spread` nats from lp, a
    mask with zeros (the second sequence of a trie all-masked), advantages of both signs and exact zeros.  Ratios that come closer than
    2e-3 to a branch edge of `EDGES` are moved off it, so every margin the tests assert holds by construction, not by luck."""
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
        r = np.exp(x)
        for e in EDGES:
            near = np.abs(r - e) < 2e-3
            x = np.where(near, np.log(e + 4e-3), x)
            r = np.exp(x)
        adv = rng.normal(0, 1.5, n)
        adv[rng.random(n) < 0.1] = 0.0
        m = (rng.random(n) < 0.8)
        if s == 1:
            m[:] = False
        a = {"advantages": float(rng.normal()) if scalar_adv else adv.astype(np.float32),
             "ref_logprobs": (mine + rng.uniform(-spread, spread, n)).astype(np.float32), "loss_mask": m}
        if not on_policy:
            a["old_logprobs"] = (mine - x).astype(np.float32)
        atts.append(a)
    return plan, att_lens, depth, n_real, lp, ent, atts


EDGES = (0.8, 1.2, 1.28, 0.9, 3.0)      # 1 - clip_low, 1 + clip_high and dual_clip of the configurations in CONFIGS


def CONFIGS():
    from dynamictreeattn_amd.losses import PolicyLoss
    return {
        "ppo": PolicyLoss(),
        "dual_k3": PolicyLoss(clip_low=0.2, clip_high=0.28, dual_clip=3.0, kl_coef=0.05, kl_estimator="k3", entropy_coef=0.01),
        "k1_sum": PolicyLoss(clip_low=0.1, clip_high=0.2, kl_coef=0.1, kl_estimator="k1", agg="token_sum", scale=1.0 / 37),
        "k2": PolicyLoss(kl_coef=0.2, kl_estimator="k2", entropy_coef=-0.02, dual_clip=3.0, scale=2.0),
    }


def trie_ref(loss, plan, att_lens, lp, ent, atts):
    """The closed form summed over packed rows: dict of `dlp`, `dent` (float64 [T]) with bounds `b_dlp`, `b_dent`, `stats` (float64 [6],
    losses.STATS order) with `b_stats`, and `margin`.  Every (sequence, j) term goes to the row its sequence's root path names."""
    T = plan.T
    lp, ent = np.asarray(lp, np.float64), np.asarray(ent, np.float64)
    dlp, dent = np.zeros(T), np.zeros(T)
    e_lp, e_ent, mag_lp, mag_ent, n_lp, n_ent = (np.zeros(T) for _ in range(6))
    stats, e_st, mag_st, n_st = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6)
    margin = np.inf
    for rows, att in zip(paths_of(plan, att_lens), atts):
        n = rows.size - 1
        if n == 0:
            continue
        r = seq_ref(loss, lp[rows[1:]], ent[rows], att)
        margin = min(margin, r["margin"])
        c = C_OPS + r["amp"]
        a, b = rows[1:], rows[:-1]                    # rows of the log-prob terms (depth j + 1) and of the entropy terms (depth j)
        np.add.at(dlp, a, r["g_lp"]); np.add.at(e_lp, a, c * r["mag_g_lp"]); np.add.at(mag_lp, a, r["mag_g_lp"]); np.add.at(n_lp, a, 1)
        np.add.at(dent, b, r["g_ent"]); np.add.at(e_ent, b, C_OPS * r["mag_g_ent"]); np.add.at(mag_ent, b, r["mag_g_ent"]); np.add.at(n_ent, b, 1)
        m = r["m"]
        for k, (val, mag, cc, cnt) in enumerate((
                (r["t_loss_lp"].sum() + r["t_loss_ent"].sum(), r["mag_loss_lp"].sum() + r["mag_loss_ent"].sum(),
                 (c * r["mag_loss_lp"]).sum() + C_OPS * r["mag_loss_ent"].sum(), 2 * n),
                ((m * r["pg"]).sum(), r["mag_pg"].sum(), (c * r["mag_pg"]).sum(), n),
                ((m * r["kl"]).sum(), r["mag_kl"].sum(), (c * r["mag_kl"]).sum(), n),
                ((m * r["ent"]).sum(), (np.abs(m) * np.abs(r["ent"])).sum(), C_OPS * (np.abs(m) * np.abs(r["ent"])).sum(), n),
                ((m * r["clipped"]).sum(), 0.0, 0.0, 0), (m.sum(), 0.0, 0.0, 0))):
            stats[k] += val; mag_st[k] += mag; e_st[k] += cc; n_st[k] += cnt
    bound = lambda e, mag, n: U32 * (e + np.maximum(n - 1, 0) * mag) + n * FLOOR
    return {"dlp": dlp, "dent": dent, "b_dlp": bound(e_lp, mag_lp, n_lp), "b_dent": bound(e_ent, mag_ent, n_ent), "stats": stats,
            "b_stats": bound(e_st, mag_st, n_st), "margin": margin}
