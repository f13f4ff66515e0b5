"""Float64 restatement of the mixture-of-experts operators (HF Qwen3MoeTopKRouter / Qwen3MoeExperts) and per-element error bounds for
the HIP kernels.

The references take the kernels' rounded inputs, so a kernel's error is its fp32 arithmetic plus the one rounding of its output:

    GEMM / combine element:  ref64_common.bound (u |ref| + C32 sqrt(n) u32 (|A| |B|) + tiny).
    router weights: u |w| + 1e-6;  lse: 1e-5 (1 + |lse|);  dlogits: u |ref| + 1e-5 p_e (|dp_e| + sum_j |dp_j| p_j) + 1e-7 max|ref|.

Top-k ties: the lower expert index wins (a stable descending sort), as the kernel documents (include/dta.h)."""
import numpy as np
import torch

from ref64_common import C32, TINY, U, U32, bound  # noqa: F401  (the rounding model, shared with the other references)


def router_ref(logits: torch.Tensor, k: int, norm: bool):
    """-> ids [T, k] (long), weights [T, k] float64, lse [T], probs [T, E], margin [T] (k-th minus (k+1)-th probability)."""
    x = logits.double()
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse[:, None])
    srt, order = torch.sort(p, dim=-1, descending=True, stable=True)
    ids = order[:, :k]
    w = srt[:, :k].clone()
    if norm:
        w = w / w.sum(-1, keepdim=True)
    margin = srt[:, k - 1] - srt[:, k] if k < p.shape[1] else torch.full_like(lse, float("inf"))
    return ids, w, lse, p, margin


def router_bwd_ref(logits: torch.Tensor, ids: torch.Tensor, dw: torch.Tensor, norm: bool):
    """d(sum dw * w)/d logits for the FIXED selection ids, in float64; also the bound's per-element scale."""
    x = logits.double().clone().requires_grad_(True)
    p = torch.softmax(x, -1)
    sel = p.gather(1, ids.long())
    w = sel / sel.sum(-1, keepdim=True) if norm else sel
    (w * dw.double()).sum().backward()
    g = x.grad.detach()
    with torch.no_grad():
        dp = torch.zeros_like(p)
        dsel = dw.double() / sel.sum(-1, keepdim=True) if norm else dw.double()
        dp.scatter_(1, ids.long(), dsel.abs())
        scale = p * (dp + (dp * p).sum(-1, keepdim=True))
    return g, scale


def permute_ref(ids: torch.Tensor, E: int):
    """Stable sort of the pairs by expert: offsets [E+1], row_of_pair [P], src_token [P]."""
    T, k = ids.shape
    flat = ids.reshape(-1).cpu().numpy().astype(np.int64)
    order = np.argsort(flat, kind="stable")
    row_of_pair = np.empty_like(order)
    row_of_pair[order] = np.arange(len(order))
    counts = np.bincount(flat, minlength=E)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return offsets, row_of_pair, order // k


def gemm_ref(mode, x, w, dy, offsets, src_token, gather):
    """fwd / dgrad / wgrad of the grouped GEMM in float64, with |A||B| for the bound.  Rows are expert-sorted."""
    E = w.shape[0] if w is not None else len(offsets) - 1
    if mode == 0:
        xs = x.double()[src_token] if gather else x.double()
        out, mag = torch.zeros(xs.shape[0], w.shape[1], dtype=torch.float64), torch.zeros(xs.shape[0], w.shape[1], dtype=torch.float64)
        for e in range(E):
            a, b = offsets[e], offsets[e + 1]
            out[a:b] = xs[a:b] @ w[e].double().T
            mag[a:b] = xs[a:b].abs() @ w[e].double().abs().T
        return out, mag, w.shape[2]
    if mode == 1:
        out, mag = torch.zeros(dy.shape[0], w.shape[2], dtype=torch.float64), torch.zeros(dy.shape[0], w.shape[2], dtype=torch.float64)
        for e in range(E):
            a, b = offsets[e], offsets[e + 1]
            out[a:b] = dy[a:b].double() @ w[e].double()
            mag[a:b] = dy[a:b].double().abs() @ w[e].double().abs()
        return out, mag, w.shape[1]
    xs = x.double()[src_token] if gather else x.double()
    N, K = dy.shape[1], xs.shape[1]
    out, mag = torch.zeros(E, N, K, dtype=torch.float64), torch.zeros(E, N, K, dtype=torch.float64)
    n = 1
    for e in range(E):
        a, b = offsets[e], offsets[e + 1]
        out[e] = dy[a:b].double().T @ xs[a:b]
        mag[e] = dy[a:b].double().abs().T @ xs[a:b].abs()
        n = max(n, b - a)
    return out, mag, n


def combine_ref(y, w, row_of_pair, T, k):
    rows = torch.as_tensor(row_of_pair).long().view(T, k)
    yy = y.double()[rows]                                  # [T, k, H]
    ww = w.double()[..., None] if w is not None else torch.ones(T, k, 1, dtype=torch.float64)
    return (ww * yy).sum(1), (ww.abs() * yy.abs()).sum(1)
