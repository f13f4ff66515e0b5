"""Built-in policy objective of RL post-training: the clipped PPO / GRPO surrogate with an optional dual clip, a KL penalty to a
reference policy, an entropy bonus and a loss mask.

``PolicyLoss.__call__`` is the DEFINITION, in plain differentiable torch: a valid ``loss_fn(logprob, entropy, attachment)`` wherever
a callback is accepted (the packed engine, the block-wise walk, ``dense.backward``, the CPU oracle engines), on any device.  Handed to
``TreeTrainingEngine.backward`` as the object itself, the packed pass evaluates the same numbers in one HIP kernel over the packed
rows (``ops.policy_loss``, ``dta_policy_loss``) instead of once per sequence.

Attachment keys, per sequence of ``len`` tokens, each of length ``len - 1``; index ``j`` is the prediction of token ``j + 1`` and lines
up with the ``logprob`` argument:

    advantages     Python float or tensor [len-1]                    required
    old_logprobs   tensor [len-1]; absent / None = on-policy         ratio == 1, gradient as if old = logprob.detach()
    ref_logprobs   tensor [len-1]                                    required iff kl_coef != 0
    loss_mask      bool or float tensor [len-1]; absent = all ones

Per token, with lp = logprob[j], A = advantages[j], m = loss_mask[j]:

    r    = exp(lp - old[j])
    pg   = max(-r A, -clamp(r, 1 - clip_low, 1 + clip_high) A);   with dual_clip = c > 1 and A < 0:  pg = min(pg, -c A)
    d    = ref[j] - lp;   kl = -d (k1) | d^2 / 2 (k2) | exp(d) - d - 1 (k3)
    term = m (pg + kl_coef kl - entropy_coef entropy[j])          entropy[j]: the distribution that predicts token j + 1

and the sequence loss is w_s * sum_j term, w_s = scale / max(sum_j m, 1) ("seq_mean") or scale ("token_sum": put 1 / (global
masked-token count) into ``scale``, which stays correct under data parallelism).  ``entropy[len - 1]`` is not used.

``ratio="sequence"`` is GSPO (the objective Qwen3 and Qwen3-MoE were trained with; ``importance_sampling_level="sequence"`` in TRL and
verl): every token of a sequence is clipped on ONE ratio, the geometric mean of the masked tokens' ratios,

    r_s  = exp( sum_j m_j (lp_j - old_j) / max(sum_j m_j, 1) )    length-normalised under "token_sum" too; on-policy: r_s == 1
    pg_j = max(-r_s A_j, -clamp(r_s, 1 - clip_low, 1 + clip_high) A_j);   the dual clip with r_s in place of r

with KL, entropy, mask and w_s as above.  The gradient flows through r_s to every masked token of the sequence (GSPO itself, not the
stop-gradient "GSPO-token" variant):  d loss_s / d lp_t = c_s m_t + the token-level KL gradient, with the per-sequence scalar
c_s = w_s r_s / max(sum m, 1) * sum_j m_j (-A_j) [pg_j not clipped].  The fused path walks each sequence's root path for it.

Off-policy corrections.  The sampler that produced a rollout (other kernels, another precision, another parallel layout) assigns a
token another log-prob than this engine does under the same weights.  With ``is_level`` set, the attachment carries

    rollout_logprobs   tensor [len-1]; the sampler's log-prob of each token     required iff is_level is not None (not looked at otherwise)

and a detached importance weight multiplies the surrogate - never the KL or the entropy term:

    y_j = old_j - rollout_j                               old absent: y_j = lp_j.detach() - rollout_j, no extra model forward
    "token":          rho_j = exp(y_j)
    "sequence":       rho_s = exp(sum_j m_j y_j)                            the product of the masked tokens' ratios
    "sequence_mean":  rho_s = exp(sum_j m_j y_j / max(sum_j m_j, 1))        their geometric mean
    is_mode "truncate" (TIS):          omega = min(rho, is_cap)
    is_mode "mask" (IcePop / MIS):     omega = rho if is_floor <= rho <= is_cap else 0
    term_j = m_j (omega pg_j + kl_coef kl_j - entropy_coef entropy_j)

omega is formed by comparisons on rho, so an overflowing exponential gives is_cap ("truncate") or 0 ("mask"), never NaN.  With
``ratio="sequence"`` the weight enters the sequence scalar: c_s = w_s r_s / n^ * sum_j m_j omega_j (-A_j) [pg_j not clipped].

``surrogate="cispo"`` (MiniMax-M1) clips a detached weight instead of dropping the token's gradient, with lo = 1 - clip_low,
hi = 1 + clip_high and r the token ratio (on-policy: r = 1):

    pg = -clamp(r, lo, hi).detach() A lp,     d pg / d lp = -clamp(r, lo, hi) A   (never zeroed)

"clipped" counts the tokens with r outside [lo, hi], whatever the sign of A.  It composes with omega, the KL term, the entropy term
and the mask; it does not go with ``ratio="sequence"`` or a dual clip.  With either of the two the fused path
reports two more statistics (``OFFPOLICY_STATS``): sum m omega and the masked tokens whose weight was truncated or dropped.

``PreferenceLoss`` (DPO / cDPO / SimPO, SLiC, IPO) couples a chosen and a rejected sequence and is therefore no per-sequence callback:
see the class.  ``two_pass_backward`` runs it through any engine with a ``forward`` / ``backward`` surface.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

__all__ = ["PolicyLoss", "KL_ESTIMATORS", "AGGREGATIONS", "RATIOS", "STATS", "PreferenceLoss", "PREFERENCE_KINDS", "PREFERENCE_STATS",
           "two_pass_backward", "SURROGATES", "IS_LEVELS", "IS_MODES", "OFFPOLICY_STATS"]

KL_ESTIMATORS = ("k1", "k2", "k3")           # position = the estimator id of dta_policy_loss
AGGREGATIONS = ("seq_mean", "token_sum")     # position = the aggregation id of dta_policy_loss
RATIOS = ("token", "sequence")               # importance ratio per prediction (PPO / GRPO) or one per sequence (GSPO); position = the ratio_level id of dta_policy_loss
# entries of the statistics vector of the fused path (engine.loss_stats), in order
STATS = ("loss", "sum_pg", "sum_kl", "sum_entropy", "clipped_tokens", "masked_tokens")
SURROGATES = ("ppo", "cispo")                # position = the surrogate id of dta_policy_loss
IS_LEVELS = ("token", "sequence", "sequence_mean")   # rollout importance weight; position + 1 = the is_level id of dta_policy_loss (0: none)
IS_MODES = ("truncate", "mask")              # position = the is_mode id of dta_policy_loss
# entries of the statistics vector under an off-policy correction or CISPO, in order: all the kernel writes
OFFPOLICY_STATS = STATS + ("sum_is_weight", "is_clipped_tokens")
PREFERENCE_KINDS = ("sigmoid", "hinge", "ipo")   # position = the kind id of dta_preference_loss
# entries of the statistics vector of a PreferenceLoss (engine.loss_stats), in order
PREFERENCE_STATS = ("loss", "sum_pair_loss", "sum_sft", "reward_margin", "chosen_reward", "rejected_reward", "correct_pairs", "pairs")


def _finite(name: str, v) -> float:
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} = {v!r} is not finite")
    return v


def _per_token(key: str, v, n: int):
    """An attachment entry per prediction is a tensor [n], or absent (None)."""
    if v is None:
        return
    if not isinstance(v, torch.Tensor):
        raise ValueError(f"{key}: a tensor of {n} elements is expected, got {type(v).__name__}")
    if v.dim() != 1 or v.shape[0] != n:
        raise ValueError(f"{key}: shape {tuple(v.shape)} where [{n}] (len - 1) is expected")


def attachments_by_sequence(trie) -> list:
    """The attachments of a trie's sequences in sequence order (`_sequence_batch_id`), as `forward` orders the log-probs."""
    atts = {att["_sequence_batch_id"]: att for attach_list in trie.attach_lists for att, _ in attach_list}
    return [atts[s] for s in range(len(atts))]


class PolicyLoss:
    def __init__(self, clip_low: float = 0.2, clip_high: float = 0.2, dual_clip: Optional[float] = None, kl_coef: float = 0.0,
                 kl_estimator: str = "k3", entropy_coef: float = 0.0, agg: str = "seq_mean", scale: float = 1.0,
                 ratio: str = "token", surrogate: str = "ppo", is_level: Optional[str] = None, is_mode: str = "truncate",
                 is_cap: float = 2.0, is_floor: float = 0.0):
        self.clip_low, self.clip_high = _finite("clip_low", clip_low), _finite("clip_high", clip_high)
        if self.clip_low < 0:
            raise ValueError(f"clip_low = {clip_low!r} is negative")
        if self.clip_high < 0:
            raise ValueError(f"clip_high = {clip_high!r} is negative")
        self.dual_clip = None if dual_clip is None else _finite("dual_clip", dual_clip)
        if self.dual_clip is not None and self.dual_clip <= 1:
            raise ValueError(f"dual_clip = {dual_clip!r} must be > 1 (None: no dual clip)")
        self.kl_coef, self.entropy_coef = _finite("kl_coef", kl_coef), _finite("entropy_coef", entropy_coef)
        self.scale = _finite("scale", scale)
        if kl_estimator not in KL_ESTIMATORS:
            raise ValueError(f"kl_estimator = {kl_estimator!r}: one of {KL_ESTIMATORS}")
        if agg not in AGGREGATIONS:
            raise ValueError(f"agg = {agg!r}: one of {AGGREGATIONS}")
        if ratio not in RATIOS:
            raise ValueError(f"ratio = {ratio!r}: one of {RATIOS}")
        self.kl_estimator, self.agg, self.ratio = kl_estimator, agg, ratio
        if surrogate not in SURROGATES:
            raise ValueError(f"surrogate = {surrogate!r}: one of {SURROGATES}")
        if is_level is not None and is_level not in IS_LEVELS:
            raise ValueError(f"is_level = {is_level!r}: None or one of {IS_LEVELS}")
        if is_mode not in IS_MODES:
            raise ValueError(f"is_mode = {is_mode!r}: one of {IS_MODES}")
        self.is_cap, self.is_floor = _finite("is_cap", is_cap), _finite("is_floor", is_floor)
        if self.is_cap <= 0:
            raise ValueError(f"is_cap = {is_cap!r} must be > 0")
        if self.is_floor < 0 or self.is_floor >= self.is_cap:
            raise ValueError(f"is_floor = {is_floor!r} must be in [0, is_cap = {self.is_cap})")
        if self.is_floor != 0 and is_mode == "truncate":
            raise ValueError(f"is_floor = {is_floor!r} goes with is_mode 'mask' only: 'truncate' has no lower edge")
        if surrogate == "cispo" and ratio == "sequence":
            raise ValueError("surrogate = 'cispo' clips a per-token weight: it does not go with ratio = 'sequence'")
        if surrogate == "cispo" and self.dual_clip is not None:
            raise ValueError(f"dual_clip = {dual_clip!r} does not go with surrogate = 'cispo' (its gradient is never zeroed)")
        self.surrogate, self.is_level, self.is_mode = surrogate, is_level, is_mode

    @property
    def extended(self) -> bool:
        """an off-policy correction or CISPO is configured: the fused path reports OFFPOLICY_STATS"""
        return self.is_level is not None or self.surrogate != "ppo"

    def __repr__(self):
        more = ""
        if (self.surrogate, self.is_level, self.is_mode, self.is_cap, self.is_floor) != ("ppo", None, "truncate", 2.0, 0.0):
            more = (f", surrogate={self.surrogate!r}, is_level={self.is_level!r}, is_mode={self.is_mode!r}, is_cap={self.is_cap}, "
                    f"is_floor={self.is_floor}")
        return (f"PolicyLoss(clip_low={self.clip_low}, clip_high={self.clip_high}, dual_clip={self.dual_clip}, kl_coef={self.kl_coef}, "
                f"kl_estimator={self.kl_estimator!r}, entropy_coef={self.entropy_coef}, agg={self.agg!r}, scale={self.scale}, "
                f"ratio={self.ratio!r}{more})")

    # ------------------------------------------------------------------------------------------
    def fields(self, attachment: dict, n: int):
        """(advantages, old_logprobs, ref_logprobs, loss_mask) of one attachment for a sequence with n = len - 1 predictions,
        checked: advantages a float or a tensor [n]; the others tensors [n] or None (ref_logprobs is None exactly when kl_coef == 0:
        it is not looked at then).  KeyError / ValueError name the key."""
        if "advantages" not in attachment or attachment["advantages"] is None:
            raise KeyError("advantages")
        adv = attachment["advantages"]
        if not isinstance(adv, torch.Tensor):
            adv = float(adv)
        old = attachment.get("old_logprobs")
        ref = None
        if self.kl_coef != 0:
            ref = attachment.get("ref_logprobs")
            if ref is None:
                raise KeyError("ref_logprobs (required because kl_coef != 0)")
        mask = attachment.get("loss_mask")
        for key, v in (("advantages", adv), ("old_logprobs", old), ("ref_logprobs", ref), ("loss_mask", mask)):
            if not isinstance(v, float):
                _per_token(key, v, n)
        return adv, old, ref, mask

    def rollout(self, attachment: dict, n: int):
        """rollout_logprobs of one attachment, checked like the other per-token keys: a tensor [n]; None exactly when is_level is None
        (the key is not looked at then).  KeyError / ValueError name the key."""
        if self.is_level is None:
            return None
        roll = attachment.get("rollout_logprobs")
        if roll is None:
            raise KeyError(f"rollout_logprobs (required because is_level = {self.is_level!r})")
        _per_token("rollout_logprobs", roll, n)
        return roll

    def is_weight(self, y: torch.Tensor, m: Optional[torch.Tensor]) -> torch.Tensor:
        """omega from the detached log-ratios y = old - rollout [n] and the mask m ([n], or None for all ones): [n] under "token", a
        scalar under the sequence levels.  Comparisons on rho alone: an exponential that overflowed gives is_cap or 0, never NaN."""
        if self.is_level != "token":
            n = int(y.shape[0])
            y = y.sum() if m is None else (m * y).sum()
            if self.is_level == "sequence_mean":
                y = y / (max(n, 1) if m is None else torch.clamp(m.sum(), min=1.0))
        rho = torch.exp(y)
        if self.is_mode == "truncate":
            return torch.where(rho > self.is_cap, torch.full_like(rho, self.is_cap), rho)
        return torch.where((rho >= self.is_floor) & (rho <= self.is_cap), rho, torch.zeros_like(rho))

    def __call__(self, logprob: torch.Tensor, entropy: torch.Tensor, attachment: dict) -> torch.Tensor:
        n = int(logprob.shape[0])
        adv, old, ref, mask = self.fields(attachment, n)
        roll = self.rollout(attachment, n)
        to = lambda v: v.detach().to(device=logprob.device, dtype=logprob.dtype)
        A = torch.full_like(logprob, adv) if isinstance(adv, float) else to(adv)
        old = logprob.detach() if old is None else to(old)
        if self.ratio == "sequence":          # one ratio per sequence: the geometric mean of the masked tokens' ratios, differentiated
            x = logprob - old
            if mask is not None:
                x = to(mask) * x
                r = torch.exp(x.sum() / torch.clamp(to(mask).sum(), min=1.0))
            else:
                r = torch.exp(x.sum() / max(n, 1))
            r = r.expand(n)
        else:
            r = torch.exp(logprob - old)
        if self.surrogate == "cispo":         # the clamped ratio is a detached weight on lp: the gradient is never zeroed
            pg = -torch.clamp(r, 1.0 - self.clip_low, 1.0 + self.clip_high).detach() * A * logprob
        else:
            pg = torch.maximum(-r * A, -torch.clamp(r, 1.0 - self.clip_low, 1.0 + self.clip_high) * A)
        if self.dual_clip is not None:
            pg = torch.where(A < 0, torch.minimum(pg, -self.dual_clip * A), pg)
        term = pg
        if roll is not None:                  # the rollout importance weight: detached, on the surrogate alone
            term = self.is_weight(old - to(roll), None if mask is None else to(mask)) * pg
        if self.kl_coef != 0:
            d = to(ref) - logprob
            kl = -d if self.kl_estimator == "k1" else 0.5 * d * d if self.kl_estimator == "k2" else torch.exp(d) - d - 1.0
            term = term + self.kl_coef * kl
        if self.entropy_coef != 0:
            term = term - self.entropy_coef * entropy[:n]
        if mask is not None:
            m = to(mask)
            term = m * term
            w = self.scale / torch.clamp(m.sum(), min=1.0) if self.agg == "seq_mean" else self.scale
        else:
            w = self.scale / max(n, 1) if self.agg == "seq_mean" else self.scale
        return w * term.sum()


# --------------------------------------------------------------------------------------------------
# Preference objectives: DPO / cDPO / SimPO ("sigmoid"), SLiC ("hinge"), IPO ("ipo")
# --------------------------------------------------------------------------------------------------
def _softplus(x: torch.Tensor) -> torch.Tensor:
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-x.abs()))      # exact in every range (F.softplus switches form at 20)


class PreferenceLoss:
    """A pair objective over (chosen, rejected) completions.  It couples two sequences - the loss of a pair needs the summed
    log-probability of both members before either gradient is known - so it is NOT a per-sequence ``loss_fn``: ``__call__`` raises.
    Hand the object itself to ``TreeTrainingEngine.backward``: the packed pass evaluates it in one C-ABI call over the packed rows
    (``ops.preference_loss``, ``dta_preference_loss``); the block-wise walk and ``two_pass_backward`` use the two-pass form.

    Attachment keys, per sequence of ``len`` tokens (n = len - 1, index j the prediction of token j + 1, as for PolicyLoss):

        pair_id          hashable                                    required; each id exactly twice in a trie
        chosen           bool                                        required; once True and once False per pair_id
        loss_mask        bool or float tensor [n]; absent = all ones (normally zero over the prompt)
        ref_logprobs     tensor [n]                                  per-token reference log-probs, or
        ref_logprob_sum  float                                       their already masked sum

    exactly one form of the reference in a call and for every sequence of it; with ``reference_free`` neither is read.  Per sequence s

        n^ = max(sum m, 1),  P = sum_j m_j lp_j,  F = sum_j m_j ref_j | ref_logprob_sum | 0,  u = (P - F) / (n^ if length_normalize else 1)

    and per pair (c, r), z = beta (u_c - u_r) - gamma:

        "sigmoid"  L = (1 - eps) softplus(-z) + eps softplus(z)      DPO; eps = label_smoothing > 0: cDPO; reference_free +
                                                                     length_normalize + gamma: SimPO
        "hinge"    L = max(0, 1 - z)                                 SLiC; a tie z = 1 takes gradient 0
        "ipo"      L = (u_c - u_r - 1 / (2 beta))^2                  IPO

    total = scale sum_pairs L - scale sft_coef sum_pairs P_c / n^_c  (the NLL term on the chosen completion of RPO / the Llama-3
    recipe).  Under data parallelism put 1 / (global pair count) into ``scale``.  The gradient is linear in the rows once one
    coefficient per sequence is known: d total / d lp[row(s, j)] = g_s m_j (``coefficients``).  Entropy is not used."""

    def __init__(self, beta: float = 0.1, kind: str = "sigmoid", label_smoothing: float = 0.0, gamma: float = 0.0,
                 length_normalize: bool = False, reference_free: bool = False, sft_coef: float = 0.0, scale: float = 1.0):
        self.beta, self.label_smoothing = _finite("beta", beta), _finite("label_smoothing", label_smoothing)
        self.gamma, self.sft_coef, self.scale = _finite("gamma", gamma), _finite("sft_coef", sft_coef), _finite("scale", scale)
        if kind not in PREFERENCE_KINDS:
            raise ValueError(f"kind = {kind!r}: one of {PREFERENCE_KINDS}")
        if self.beta <= 0:
            raise ValueError(f"beta = {beta!r} must be > 0")
        if not 0 <= self.label_smoothing < 0.5:
            raise ValueError(f"label_smoothing = {label_smoothing!r} must be in [0, 0.5)")
        if self.label_smoothing != 0 and kind != "sigmoid":
            raise ValueError(f"label_smoothing = {label_smoothing!r} goes with kind 'sigmoid' only, not {kind!r}")
        if self.gamma != 0 and kind == "ipo":
            raise ValueError(f"gamma = {gamma!r} must be 0 with kind 'ipo'")
        if self.sft_coef < 0:
            raise ValueError(f"sft_coef = {sft_coef!r} is negative")
        self.kind, self.length_normalize, self.reference_free = kind, bool(length_normalize), bool(reference_free)

    def __repr__(self):
        return (f"PreferenceLoss(beta={self.beta}, kind={self.kind!r}, label_smoothing={self.label_smoothing}, gamma={self.gamma}, "
                f"length_normalize={self.length_normalize}, reference_free={self.reference_free}, sft_coef={self.sft_coef}, scale={self.scale})")

    def __call__(self, logprob, entropy, attachment):
        raise TypeError("a PreferenceLoss couples two sequences (chosen and rejected) and cannot be evaluated one sequence at a time: "
                        "pass the object itself to engine.backward (or to losses.two_pass_backward), not a callback that calls it")

    # ------------------------------------------------------------------------------------------
    def fields(self, attachment: dict, n: int):
        """(loss_mask, ref_logprobs, ref_logprob_sum) of one attachment for a sequence with n = len - 1 predictions, checked: the
        tensors [n] or None, the sum a float or None; with reference_free both reference forms are None (not looked at), otherwise
        exactly one is given.  pair_id and chosen must be present.  KeyError / ValueError name the key."""
        for key in ("pair_id", "chosen"):
            if key not in attachment or attachment[key] is None:
                raise KeyError(key)
        mask = attachment.get("loss_mask")
        ref, ref_sum = (None, None) if self.reference_free else (attachment.get("ref_logprobs"), attachment.get("ref_logprob_sum"))
        if not self.reference_free and (ref is None) == (ref_sum is None):
            raise (KeyError("ref_logprobs or ref_logprob_sum (required unless reference_free)") if ref is None else
                   ValueError("ref_logprobs and ref_logprob_sum are both given: exactly one form of the reference is used"))
        _per_token("ref_logprobs", ref, n)
        _per_token("loss_mask", mask, n)
        if ref_sum is not None:
            ref_sum = _finite("ref_logprob_sum", ref_sum)
        return mask, ref, ref_sum

    def _sequence_sums(self, logprobs, attachments):
        """(n^ [S], P [S] - differentiable -, F [S], pair_c, pair_r) over the whole list"""
        from . import packing
        if len(logprobs) != len(attachments):
            raise ValueError(f"{len(logprobs)} log-prob tensors for {len(attachments)} attachments")
        pair_c, pair_r = packing.preference_pair_tables([[(a, int(lp.shape[0]) + 1) for lp, a in zip(logprobs, attachments)]])
        nh, P, F, forms = [], [], [], set()
        for lp, att in zip(logprobs, attachments):
            mask, ref, ref_sum = self.fields(att, int(lp.shape[0]))
            to = lambda v: v.detach().to(device=lp.device, dtype=lp.dtype)
            m = torch.ones_like(lp) if mask is None else to(mask)
            forms.add("ref_logprobs" if ref is not None else "ref_logprob_sum" if ref_sum is not None else None)
            nh.append(torch.clamp(m.detach().sum(), min=1.0))
            P.append((m * lp).sum())
            F.append((m * to(ref)).sum() if ref is not None else torch.as_tensor(0.0 if ref_sum is None else ref_sum, device=lp.device, dtype=lp.dtype))
        if len(forms) > 1:
            raise ValueError("ref_logprobs for some sequences and ref_logprob_sum for others: one form of the reference per call")
        idx = lambda a: torch.as_tensor(a, dtype=torch.long, device=P[0].device)
        return torch.stack(nh), torch.stack(P), torch.stack(F), idx(pair_c), idx(pair_r)

    def _pair_loss(self, du):
        """(L, dL/d(u_c - u_r)) per pair"""
        if self.kind == "ipo":
            h = du - 1.0 / (2.0 * self.beta)
            return h * h, 2.0 * h
        z = self.beta * du - self.gamma
        if self.kind == "sigmoid":
            eps = self.label_smoothing
            return (1.0 - eps) * _softplus(-z) + eps * _softplus(z), self.beta * (torch.sigmoid(z) - (1.0 - eps))
        return torch.where(z < 1, 1.0 - z, torch.zeros_like(z)), self.beta * torch.where(z < 1, -torch.ones_like(z), torch.zeros_like(z))

    def total(self, logprobs, attachments) -> torch.Tensor:
        """The DEFINITION: the objective over the whole list of per-sequence log-prob tensors ([len_s - 1] each, lined up with
        `attachments`), in differentiable torch on any device."""
        nh, P, F, c, r = self._sequence_sums(logprobs, attachments)
        u = (P - F) / nh if self.length_normalize else P - F
        L, _ = self._pair_loss(u[c] - u[r])
        return self.scale * L.sum() - self.scale * self.sft_coef * (P[c] / nh[c]).sum()

    @torch.no_grad()
    def coefficients(self, logprobs, attachments):
        """(total, g [S], stats [8]) from detached log-probs: d total / d logprobs[s][j] = g[s] loss_mask_s[j]; stats in the order of
        PREFERENCE_STATS.  The first pass of the two-pass form."""
        nh, P, F, c, r = self._sequence_sums([lp.detach() for lp in logprobs], attachments)
        N = nh if self.length_normalize else torch.ones_like(nh)
        u = (P - F) / N
        du = u[c] - u[r]
        L, dL = self._pair_loss(du)
        sft = P[c] / nh[c]
        g = torch.zeros_like(u)
        g[c] = self.scale * dL / N[c] - self.scale * self.sft_coef / nh[c]
        g[r] = -self.scale * dL / N[r]
        total = self.scale * L.sum() - self.scale * self.sft_coef * sft.sum()
        stats = torch.stack([total, L.sum(), sft.sum(), (self.beta * du).sum(), (self.beta * u[c]).sum(), (self.beta * u[r]).sum(),
                             (u[c] > u[r]).to(u.dtype).sum(), torch.as_tensor(float(c.shape[0]), device=u.device, dtype=u.dtype)])
        return total, g, stats

    def surrogate(self, g):
        """The linear closure of the second pass: loss_fn(logprob, entropy, attachment) = g[s] (m logprob).sum(), s the attachment's
        `_sequence_batch_id` - its gradient is the objective's, its value is not."""
        def loss_fn(logprob, entropy, attachment):
            mask = attachment.get("loss_mask")
            x = logprob if mask is None else mask.detach().to(device=logprob.device, dtype=logprob.dtype) * logprob
            return g[attachment["_sequence_batch_id"]].to(device=logprob.device, dtype=logprob.dtype) * x.sum()
        return loss_fn


def two_pass_backward(engine, model, trie, loss: PreferenceLoss, block_size: int):
    """A PreferenceLoss through any engine with the `forward(model, trie)` / `backward(model, trie, loss_fn, block_size)` surface,
    at the cost of one more (no-grad) model forward: `forward` for the sequence log-probs, `loss.coefficients` on them, `backward`
    with the linear closure g_s (m logprob).sum().  Accumulates the gradient of the true objective and returns
    (its value as a float, stats [8] in the order of PREFERENCE_STATS)."""
    total, g, stats = loss.coefficients(engine.forward(model, trie), attachments_by_sequence(trie))
    engine.backward(model, trie, loss.surrogate(g), block_size)
    return float(total.item()), stats
