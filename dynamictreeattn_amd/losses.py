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
c_s = w_s r_s / max(sum m, 1) * sum_j m_j (-A_j) [pg_j not clipped].  The fused path evaluates it with ``dta_policy_loss_seq``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

__all__ = ["PolicyLoss", "KL_ESTIMATORS", "AGGREGATIONS", "RATIOS", "STATS"]

KL_ESTIMATORS = ("k1", "k2", "k3")           # position = the estimator id of dta_policy_loss
AGGREGATIONS = ("seq_mean", "token_sum")     # position = the aggregation id of dta_policy_loss
RATIOS = ("token", "sequence")               # importance ratio per prediction (PPO / GRPO) or one per sequence (GSPO: dta_policy_loss_seq)
# entries of the statistics vector of the fused path (engine.loss_stats), in order
STATS = ("loss", "sum_pg", "sum_kl", "sum_entropy", "clipped_tokens", "masked_tokens")


def _finite(name: str, v) -> float:
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} = {v!r} is not finite")
    return v


class PolicyLoss:
    def __init__(self, clip_low: float = 0.2, clip_high: float = 0.2, dual_clip: Optional[float] = None, kl_coef: float = 0.0,
                 kl_estimator: str = "k3", entropy_coef: float = 0.0, agg: str = "seq_mean", scale: float = 1.0,
                 ratio: str = "token"):
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

    def __repr__(self):
        return (f"PolicyLoss(clip_low={self.clip_low}, clip_high={self.clip_high}, dual_clip={self.dual_clip}, kl_coef={self.kl_coef}, "
                f"kl_estimator={self.kl_estimator!r}, entropy_coef={self.entropy_coef}, agg={self.agg!r}, scale={self.scale}, "
                f"ratio={self.ratio!r})")

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
            if v is None or isinstance(v, float):
                continue
            if not isinstance(v, torch.Tensor):
                raise ValueError(f"{key}: a tensor of {n} elements is expected, got {type(v).__name__}")
            if v.dim() != 1 or v.shape[0] != n:
                raise ValueError(f"{key}: shape {tuple(v.shape)} where [{n}] (len - 1) is expected")
        return adv, old, ref, mask

    def __call__(self, logprob: torch.Tensor, entropy: torch.Tensor, attachment: dict) -> torch.Tensor:
        n = int(logprob.shape[0])
        adv, old, ref, mask = self.fields(attachment, n)
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
        pg = torch.maximum(-r * A, -torch.clamp(r, 1.0 - self.clip_low, 1.0 + self.clip_high) * A)
        if self.dual_clip is not None:
            pg = torch.where(A < 0, torch.minimum(pg, -self.dual_clip * A), pg)
        term = pg
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
