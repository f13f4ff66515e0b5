"""Float64 closed form of losses.PreferenceLoss - DPO / cDPO / SimPO ("sigmoid"), SLiC ("hinge"), IPO ("ipo") - value, per-sequence
coefficients g_s, statistics and row gradients summed over a trie, in plain numpy (no autograd); the tries of policy_loss_ref64 and
seq_policy_loss_ref64 with their sequences paired deterministically; inputs whose pairs sit away from every branch edge by
construction; and the error bound of the fp32 kernels (dta_preference_loss) against it.

Closed form (lp, m, ref as in losses.py).  Per sequence s with n predictions:
    n^ = max(sum m, 1),  P = sum_j m_j lp_j,  F = sum_j m_j ref_j | ref_logprob_sum | 0,  N = n^ under length_normalize else 1,  u = (P - F) / N
per pair (c, r), du = u_c - u_r, z = beta du - gamma, e = label_smoothing:
    sigmoid  L = (1 - e) softplus(-z) + e softplus(z)    D = dL/du_c = beta (sigma(z) - (1 - e))
    hinge    L = max(0, 1 - z)                           D = -beta [z < 1]
    ipo      L = h^2, h = du - 1 / (2 beta)              D = 2 h
    g_c = scale D / N_c - scale sft_coef / n^_c,   g_r = -scale D / N_r,   d total / d lp[row(s, j)] = g_s m_j
    total = scale sum L - scale sft_coef sum P_c / n^_c
The hyper-parameters are taken as the fp32 numbers the kernel is handed (as_fp32; False: the doubles PreferenceLoss computes with).

Pairing (`build`): the sequences of a trie in callback order are paired two by two, (0, 1), (2, 3), ...; pairs k and k + 1 with
k % 3 == 1 then swap their second members, so that not every pair is two neighbours; the first member is the chosen one in even pairs,
the second in odd pairs.  Before that the last sequence of the last leaf is attached once more (an odd count) or twice more (an even
count): the count becomes even and the LAST pair is a duplicate - the same token string twice, sharing a leaf - with identical masks
and references.  Its u_c and u_r are the same number in float64 and bit for bit in the kernel (the same operations on the same data in
the same fixed order): an exact tie by construction, which must count as not correct.

Edges: z = 1 (hinge: the gradient changes) and u_c = u_r (correct_pairs).  `make_inputs` places du of pair q (the tie pair apart) on
TARGETS[q % 6] by shifting the reference of one member - its per-token reference log-probs over its masked tokens, or its reference
sum -, as seq_policy_loss_ref64 shifts `old`.  The targets are at least 0.2 from 0 and at least 0.5 from the hinge edge
du = (1 + gamma) / beta of every configuration in CONFIGS (2.5 and 2.0).  Under reference_free there is no reference to shift: a pair whose seeded du
comes closer than 1e-2 to 0 has predictions of one member's mask flipped until it does not.  `margin_hinge` and `margin_correct` are the smallest distances |z - 1| and |du| over the pairs (the tie pair
left out of margin_correct only); the tests assert both >= 1e-3 for every case, so fp32 and fp64 take the same branch.

Error bound of the kernels (u = 2^-24, every input an fp32 number, 0/1 masks so that n^ and every product m x are exact; a fused
multiply-add rounds once where the bound counts two roundings, so contraction only helps).
Sequence pass.  P^ is a sum of n terms m lp in some order: each partial sum is rounded once and never exceeds A_P = sum |m lp|, so
|P^ - P| <= (n - 1) u A_P; F^ likewise with A_F = sum |m ref| (per-token form; a given sum or no reference carries no error).  The
subtraction adds u |P - F|, the division by N another u |u_s|:
    |u^_s - u_s| <= d_s = u ((n - 1) (A_P + A_F) / N + 2 |u_s|)
and P^ / n^ (the SFT term) is off by at most e_sft = u ((n - 1) A_P / n^ + |P| / n^).
Pair pass.  du^ = u^_c - u^_r: d_du = d_c + d_r + u |du|.  z^ = beta du^ - gamma (a product and a subtraction):
d_z = beta d_du + u (beta |du| + |z|).  Turning the absolute error of z into one of dL/dz:
    sigmoid  sigma is formed from E = expf(-|z|) <= 1 as 1 / (1 + E) or E / (1 + E): |sigma'| <= 1/4 turns d_z into d_z / 4; the accurate
             expf (1 ulp = 2 u, damped by the factor E / (1 + E) or 1 / (1 + E) <= 1), the sum and the division add 4 u sigma; 1 - e is one
             rounding, the subtraction one more: with M = sigma + (1 - e),  |dz^ - dz| <= d_z / 4 + 5 u M
    hinge    piecewise constant: exact while the branch is the same (margin_hinge)
    ipo      linear: h^ = du^ - c0 with c0 = fl(1 / (2 beta)) (u c0) and one subtraction:  d_h = d_du + u (c0 + |h|),  D = 2 h exact
so  E_D = beta (d_z / 4 + 5 u M) + u beta |dz|  (sigmoid; the last term is the product by beta),  0 (hinge),  2 d_h (ipo).
a = scale D (1 rounding), a / N (1), b = scale sft_coef / n^ (2), their difference (1):
    |g^_c - g_c| <= E_g = |scale| E_D / N_c + 3 u (|a| / N_c + |b|),      |g^_r - g_r| <= |scale| E_D / N_r + 2 u |a| / N_r.
Row pass.  dlp[t] sums g_s m over the N sequences through the row, each product exact; a sum of N terms in ANY order adds at most
(N - 1) u sum |g_s m|.  With k_i u |t_i|^ = E_g of term i this is the bound of the other two modules,
    |got - ref| <= u sum_i (k_i + N - 1) |t_i|^ + N 2^-126
per element of dlp (N = the terms of that row) and per statistic (N = P, the pairs).  The statistics' terms:
    L        sigmoid: the two softplus see the same z^ (|softplus'| <= 1: d_z), expf 2 u E, log1pf (2 ulp = 4 u log1p(E) <= 4 u E), their
             sums, 1 - e and the products: E_L = d_z + 6 u E + 4 u L;   hinge: [z < 1] (d_z + u L);   ipo: 2 |h| d_h + u L
    loss     scale L - (scale sft_coef) (P_c / n^_c): |scale| E_L + |scale sft_coef| e_sft + 3 u (|scale| L + |scale sft_coef P_c / n^_c|)
    sum_sft  e_sft;   reward_margin: beta d_du + u beta |du|;   chosen / rejected reward: beta d_s + u beta |u_s|
The two counts (correct_pairs, pairs) are sums of 0/1 values below 2^24 and must be exact.  Second-order terms are dropped.  Nothing
here was fitted to the kernels' observed error."""
import functools

import numpy as np

import policy_loss_ref64 as R
import seq_policy_loss_ref64 as Q

U32, FLOOR = R.U32, R.FLOOR
paths_of, attach_lists_of = R.paths_of, R.attach_lists_of
TRIES = dict(Q.TRIES)                              # the hand-made tries of policy_loss_ref64 + long_path + many_seqs
TARGETS = (-2.0, -0.3, 0.2, 1.0, 3.0, 7.0)         # u_c - u_r of pair q: TARGETS[q % 6]
STATS = ("loss", "sum_pair_loss", "sum_sft", "reward_margin", "chosen_reward", "rejected_reward", "correct_pairs", "pairs")


def CONFIGS():
    """name -> (PreferenceLoss, form of the reference: "tokens" | "sum" | None).  Every kind; with and without length_normalize,
    reference_free, label_smoothing, sft_coef; both reference forms."""
    from dynamictreeattn_amd.losses import PreferenceLoss
    return {
        "dpo": (PreferenceLoss(beta=0.5), "tokens"),
        "dpo_sum": (PreferenceLoss(beta=0.1, scale=1.0 / 7), "sum"),
        "cdpo_sft": (PreferenceLoss(beta=0.5, label_smoothing=0.1, sft_coef=0.3), "tokens"),
        "simpo": (PreferenceLoss(beta=2.0, gamma=0.5, length_normalize=True, reference_free=True), None),
        "slic": (PreferenceLoss(beta=0.5, kind="hinge", gamma=0.25), "sum"),
        "slic_ln": (PreferenceLoss(beta=0.5, kind="hinge", length_normalize=True, sft_coef=0.05), "tokens"),
        "ipo": (PreferenceLoss(beta=0.25, kind="ipo", scale=0.5), "tokens"),
        "ipo_ln_sft": (PreferenceLoss(beta=0.25, kind="ipo", length_normalize=True, sft_coef=0.1), "sum"),
    }


@functools.lru_cache(maxsize=None)
def build(name):
    """(plan, attach_lens, depth int32 [T], n_real_rows, pair_c, pair_r): seq_policy_loss_ref64.build with the last sequence attached
    once or twice more and the pairs of the module docstring (callback-order indices; sorted by the chosen member)."""
    plan, att, depth, n_real = Q.build(name)
    att = [list(leaf) for leaf in att]
    S = sum(map(len, att))
    att[-1] += [att[-1][-1]] * (1 if S % 2 else 2)
    S = sum(map(len, att))
    first, second = list(range(0, S, 2)), list(range(1, S, 2))
    npairs = S // 2
    for k in range(1, npairs - 2, 3):
        second[k], second[k + 1] = second[k + 1], second[k]
    pairs = sorted((a, b) if k % 2 == 0 else (b, a) for k, (a, b) in enumerate(zip(first, second)))
    tie = (S - 2, S - 1) if (npairs - 1) % 2 == 0 else (S - 1, S - 2)
    assert tie in pairs
    return plan, att, depth, n_real, np.asarray([c for c, _ in pairs], np.int32), np.asarray([r for _, r in pairs], np.int32)


def _seq_sums(loss, lps, atts):
    """float64 per-sequence arrays: nh, P, F, A_P, A_F, n"""
    S = len(lps)
    nh, P, F, AP, AF, n = (np.zeros(S) for _ in range(6))
    for s, (lp, a) in enumerate(zip(lps, atts)):
        lp = np.asarray(lp, np.float64)
        m = a.get("loss_mask")
        m = np.ones(lp.shape[0]) if m is None else np.asarray(m).astype(np.float64)
        nh[s], P[s], AP[s], n[s] = max(m.sum(), 1.0), (m * lp).sum(), np.abs(m * lp).sum(), lp.shape[0]
        if not loss.reference_free:
            if a.get("ref_logprobs") is not None:
                ref = np.asarray(a["ref_logprobs"], np.float64)
                F[s], AF[s] = (m * ref).sum(), np.abs(m * ref).sum()
            else:
                F[s] = float(a["ref_logprob_sum"])
    return nh, P, F, AP, AF, n


def closed_form(loss, lps, atts, pair_c, pair_r, as_fp32=True):
    """The closed form over a list of per-sequence log-probs (callback order) and the pair tables.  Returns a dict: per sequence `nh`,
    `u`, `g` with bounds `b_u`, `b_g`; `stats` [8] (STATS order) with `b_stats`; `total`; `margin_hinge`, `margin_correct`; per pair `du`, `z`."""
    f = (lambda v: float(np.float32(v))) if as_fp32 else float
    beta, eps, gamma, sc, scale = f(loss.beta), f(loss.label_smoothing), f(loss.gamma), f(loss.sft_coef), f(loss.scale)
    nh, P, F, AP, AF, n = _seq_sums(loss, lps, atts)
    c, r = np.asarray(pair_c, np.int64), np.asarray(pair_r, np.int64)
    N = nh if loss.length_normalize else np.ones_like(nh)
    u = (P - F) / N
    d_s = U32 * (np.maximum(n - 1, 0) * (AP + AF) / N + 2 * np.abs(u))
    sft, e_sft = P / nh, U32 * (np.maximum(n - 1, 0) * AP / nh + np.abs(P) / nh)
    du = u[c] - u[r]
    d_du = d_s[c] + d_s[r] + U32 * np.abs(du)
    z = beta * du - gamma
    d_z = beta * d_du + U32 * (beta * np.abs(du) + np.abs(z))
    if loss.kind == "ipo":
        c0 = 1.0 / (2.0 * beta)
        h = du - c0
        d_h = d_du + U32 * (c0 + np.abs(h))
        L, D, E_D, E_L = h * h, 2 * h, 2 * d_h, 2 * np.abs(h) * d_h + U32 * h * h
    elif loss.kind == "sigmoid":
        E = np.exp(-np.abs(z))
        sig = np.where(z >= 0, 1 / (1 + E), E / (1 + E))
        sp = lambda x: np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))
        L = (1 - eps) * sp(-z) + eps * sp(z)
        dz = sig - (1 - eps)
        D = beta * dz
        E_D = beta * (d_z / 4 + 5 * U32 * (sig + (1 - eps))) + U32 * beta * np.abs(dz)
        E_L = d_z + 6 * U32 * E + 4 * U32 * L
    else:
        L = np.maximum(0.0, 1 - z)
        D = -beta * (z < 1)
        E_D = np.zeros_like(z)
        E_L = (z < 1) * (d_z + U32 * L)
    a = scale * D
    b = scale * sc / nh
    g, b_g = np.zeros_like(u), np.zeros_like(u)
    g[c] = a / N[c] - b[c]
    g[r] = -a / N[r]
    b_g[c] = abs(scale) * E_D / N[c] + 3 * U32 * (np.abs(a) / N[c] + np.abs(b[c]))
    b_g[r] = abs(scale) * E_D / N[r] + 2 * U32 * np.abs(a) / N[r]
    npairs = c.shape[0]
    terms = [scale * L - scale * sc * sft[c], L, sft[c], beta * du, beta * u[c], beta * u[r], (u[c] > u[r]).astype(np.float64), np.ones(npairs)]
    mags = [abs(scale) * np.abs(L) + abs(scale * sc) * np.abs(sft[c]), np.abs(L), np.abs(sft[c]), beta * np.abs(du), beta * np.abs(u[c]),
            beta * np.abs(u[r]), np.zeros(npairs), np.zeros(npairs)]
    errs = [abs(scale) * E_L + abs(scale * sc) * e_sft[c] + 3 * U32 * mags[0], E_L, e_sft[c], beta * d_du + U32 * mags[3],
            beta * d_s[c] + U32 * mags[4], beta * d_s[r] + U32 * mags[5], np.zeros(npairs), np.zeros(npairs)]
    stats = np.asarray([t.sum() for t in terms])
    b_stats = np.asarray([e.sum() + U32 * max(npairs - 1, 0) * m.sum() + npairs * FLOOR for e, m in zip(errs, mags)])
    b_stats[6:] = 0.0
    tie = du == 0
    return {"nh": nh, "u": u, "b_u": d_s + FLOOR, "g": g, "b_g": b_g + FLOOR, "stats": stats, "b_stats": b_stats, "total": float(stats[0]),
            "margin_hinge": float(np.abs(z - 1).min()) if loss.kind == "hinge" else np.inf, "margin_correct": float(np.abs(du[~tie]).min()) if (~tie).any() else np.inf,
            "ties": int(tie.sum()), "du": du, "z": z}


def make_inputs(name, cfg, seed=0):
    """Seeded fp32 inputs of a trie for configuration `cfg`: lp [T] and one attachment per sequence - pair_id, chosen, a mask with
    zeros (the second sequence all-masked; the two masks of a duplicate string differ in their first element) and the reference in the configuration's form, shifted so that du of pair q is
    TARGETS[q % 6] (module docstring); the members of the last pair get identical masks and references.  Returns
    (plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts)."""
    loss, form = CONFIGS()[cfg]
    plan, att_lens, depth, n_real, pair_c, pair_r = build(name)
    rng = np.random.default_rng(seed)
    lp = (-rng.uniform(0.05, 6.0, plan.T)).astype(np.float32)
    paths = paths_of(plan, att_lens)
    S = len(paths)
    atts = []
    for s, rows in enumerate(paths):
        n = rows.size - 1
        m = rng.random(n) < 0.8
        if n and not m.any():
            m[rng.integers(n)] = True                                   # every sequence but the second keeps a prediction
        if s == 1:
            m[:] = False
        ref = (lp[rows[1:]].astype(np.float64) + rng.uniform(-3.0, 3.0, n)).astype(np.float32)
        if s == S - 1:                                                  # the duplicate of sequence S - 2: the tie pair
            m, ref = atts[-1]["loss_mask"].copy(), atts[-1]["_ref"].copy()
        atts.append({"loss_mask": m, "_ref": ref})
    for q, (c, r) in enumerate(zip(pair_c, pair_r)):
        atts[c].update(pair_id=f"pair{q}", chosen=True); atts[r].update(pair_id=f"pair{q}", chosen=False)
        if {int(c), int(r)} != {S - 2, S - 1} and np.array_equal(paths[c], paths[r]) and paths[c].size > 1:
            # another duplicate string: its masks differ in the first prediction, so that only the LAST pair can tie (reference_free)
            s_, o_ = (max(c, r), min(c, r)) if max(c, r) != 1 else (min(c, r), max(c, r))
            atts[s_]["loss_mask"][0] = not atts[o_]["loss_mask"][0]
    lps = [lp[rows[1:]] for rows in paths]
    masked = lambda s: atts[s]["loss_mask"].astype(np.float64)
    F = np.asarray([(masked(s) * atts[s]["_ref"].astype(np.float64)).sum() for s in range(S)])
    if form == "sum":
        F = F.astype(np.float32).astype(np.float64)
    if form is not None:
        nh = np.asarray([max(masked(s).sum(), 1.0) for s in range(S)])
        P = np.asarray([(masked(s) * lps[s].astype(np.float64)).sum() for s in range(S)])
        N = nh if loss.length_normalize else np.ones(S)
        for q, (c, r) in enumerate(zip(pair_c, pair_r)):
            if {int(c), int(r)} == {S - 2, S - 1}:
                continue
            want = TARGETS[q % len(TARGETS)]
            # move the chosen member's reference sum (the rejected one's when the chosen has no masked token to carry a per-token shift)
            s, o, sign = (c, r, 1.0) if form == "sum" or atts[c]["loss_mask"].any() else (r, c, -1.0)
            if form == "tokens" and not atts[s]["loss_mask"].any():
                continue                                                # neither member has a masked token: both u are 0 (not in these tries)
            u_o = (P[o] - F[o]) / N[o]
            new_F = P[s] - N[s] * (u_o + sign * want)
            if form == "tokens":
                k = atts[s]["loss_mask"]
                atts[s]["_ref"] = atts[s]["_ref"].copy()
                atts[s]["_ref"][k] += np.float32((new_F - F[s]) / k.sum())
                F[s] = (masked(s) * atts[s]["_ref"].astype(np.float64)).sum()
            else:
                F[s] = float(np.float32(new_F))
    else:
        # reference_free: nothing to shift.  A pair whose seeded du comes closer than 1e-2 to the tie is moved off it by flipping
        # predictions of one member's mask, first to last, until it is not
        u_of = lambda s: (masked(s) * lps[s].astype(np.float64)).sum() / (max(masked(s).sum(), 1.0) if loss.length_normalize else 1.0)
        for c, r in zip(pair_c, pair_r):
            if {int(c), int(r)} == {S - 2, S - 1}:
                continue
            s = int(c) if c != 1 and atts[c]["loss_mask"].size else int(r)
            for j in range(atts[s]["loss_mask"].size):
                if abs(u_of(c) - u_of(r)) >= 1e-2:
                    break
                atts[s]["loss_mask"][j] = not atts[s]["loss_mask"][j]
    for s, a in enumerate(atts):
        ref = a.pop("_ref")
        if form == "tokens":
            a["ref_logprobs"] = ref
        elif form == "sum":
            a["ref_logprob_sum"] = float(F[s])
    return plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts


def trie_ref(loss, plan, att_lens, pair_c, pair_r, lp, atts):
    """closed_form over the trie's sequences, plus the row gradients: `dlp` float64 [T] with bound `b_dlp`"""
    paths = paths_of(plan, att_lens)
    out = closed_form(loss, [np.asarray(lp)[rows[1:]] for rows in paths], atts, pair_c, pair_r)
    T = plan.T
    dlp, err, mag, cnt = (np.zeros(T) for _ in range(4))
    for s, (rows, a) in enumerate(zip(paths, atts)):
        m = np.asarray(a["loss_mask"]).astype(np.float64)
        np.add.at(dlp, rows[1:], out["g"][s] * m); np.add.at(err, rows[1:], out["b_g"][s] * m)
        np.add.at(mag, rows[1:], abs(out["g"][s]) * m); np.add.at(cnt, rows[1:], 1)
    out["dlp"], out["b_dlp"] = dlp, err + U32 * np.maximum(cnt - 1, 0) * mag + cnt * FLOOR
    return out


@functools.lru_cache(maxsize=None)
def case(name, cfg, seed=0):
    """(loss, inputs of make_inputs, trie_ref of them), made once per process and shared: treat as read-only"""
    loss = CONFIGS()[cfg][0]
    inputs = make_inputs(name, cfg, seed=seed)
    plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts = inputs
    return loss, inputs, trie_ref(loss, plan, att_lens, pair_c, pair_r, lp, atts)
