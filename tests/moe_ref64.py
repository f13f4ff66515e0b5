"""Float64 restatement of the mixture-of-experts operators (HF Qwen3MoeTopKRouter / Qwen3MoeExperts) and per-element error bounds for
the HIP kernels.

The references take the kernels' rounded inputs, so a kernel's error is its fp32 arithmetic plus the one rounding of its output:

    GEMM / combine element:  ref64_common.bound (u |ref| + C32 sqrt(n) u32 (|A| |B|) + tiny).
    router weights: u |w| + 1e-6;  lse: 1e-5 (1 + |lse|);  dlogits: u |ref| + 1e-5 p_e (|dp_e| + sum_j |dp_j| p_j) + 1e-7 max|ref|.

Top-k ties: the lower expert index wins (a stable descending sort), as the kernel documents (include/dta.h).

The composed block (ops.moe_mlp) is restated by block_ref in float64 autograd with the selection fixed; routing_safe_rows names the
rows whose selection no rounding of the logits can change.  tests/test_moe_ref64.py checks both, and the generated inputs' conditions,
on the CPU."""
import numpy as np
import torch

from ref64_common import C32, TINY, U, U32, bound  # noqa: F401  (the rounding model, shared with the other references)


# (E, k) of the router tests: lane l of the kernel holds experts l, l+64, l+128, l+192, so 64 / 65, 128 / 129, 192 / 193 and 255 / 256
# sit on either side of a slot's edge; (16, 16) and (1, 1) select every expert
ROUTER_CASES = [(8, 1), (8, 2), (60, 2), (60, 8), (128, 8), (128, 1), (256, 16),
                (64, 4), (65, 4), (129, 8), (192, 8), (193, 8), (255, 16), (16, 16), (1, 1)]
ROUTER_T = 301
MARGIN = 1e-5               # rows whose k-th and (k+1)-th probability lie further apart keep their top-k under fp32 rounding
MARGIN_SHARE = 0.85         # share of the rows that must have that margin: a condition on the generated logits

# (T, H, I, E, k) of the composed block (tests/test_gpu_moe_block.py): two n-tiles and a k-tail behind full k-steps (144 = 128 + 16 =
# 2 * 64 + 16, 208 = 3 * 64 + 16), E > 64 with k 8, a single token, and k = E
BLOCK_SHAPES = [(333, 144, 80, 12, 3), (257, 208, 96, 130, 8), (1, 144, 80, 12, 3), (130, 64, 48, 8, 8)]
SAFE_SHARE = 2 / 3          # share of the rows routing_safe_rows must keep: a condition on the generated inputs


def router_logits(E: int, k: int, dtype):
    """The router tests' logits [ROUTER_T, E], rounded to dtype, and the generator that drew them (for the gradient that follows)."""
    g = torch.Generator().manual_seed(E * 31 + k)
    return (2.0 * torch.randn(ROUTER_T, E, generator=g)).to(dtype), g


def block_inputs(T: int, H: int, I: int, E: int, k: int, dtype):
    """h [T, H], router_w [E, H] (std 2 / sqrt(H): logits of std 2), gate_up_w [E, 2I, H], down_w [E, H, I] (std 1 / sqrt(fan-in)) and
    dout [T, H], rounded to dtype, on the host."""
    g = torch.Generator().manual_seed(T + H + E)
    r = lambda *shape: torch.randn(*shape, generator=g)
    return tuple(t.to(dtype) for t in (r(T, H), r(E, H) * 2 / H ** 0.5, r(E, 2 * I, H) / H ** 0.5, r(E, H, I) / I ** 0.5, r(T, H)))


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


def dropped_ids(T: int, k: int, E: int, seed: int = 3) -> torch.Tensor:
    """ids [T, k] of distinct experts per token in which every seventh pair is out of range, alternately -1 and E."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).reshape(-1)
    ids[0::14], ids[7::14] = -1, E
    return ids.view(T, k)


def permute_ref(ids: torch.Tensor, E: int):
    """Stable sort of the pairs by expert: offsets [E+1], row_of_pair [P], src_token [P].  A pair whose id lies outside [0, E) is
    dropped (include/dta.h): it takes no row and gets row_of_pair -1, offsets[E] counts the valid pairs, and src_token is defined for
    the rows below offsets[E] only (the entries behind them are whatever the sort left there)."""
    T, k = ids.shape
    flat = ids.reshape(-1).cpu().numpy().astype(np.int64)
    valid = (flat >= 0) & (flat < E)
    order = np.argsort(np.where(valid, flat, E), kind="stable")      # dropped pairs sort behind every expert
    row_of_pair = np.empty_like(order)
    row_of_pair[order] = np.arange(len(order))
    row_of_pair[~valid] = -1
    counts = np.bincount(flat[valid], minlength=E)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    return offsets, row_of_pair, order // k


def block_ref(h, router_w, gate_up_w, down_w, ids, norm: bool):
    """Qwen3MoeSparseMoeBlock.forward on float64 operands with the selection `ids` [T, k] FIXED: router GEMM, softmax over all experts,
    the selected probabilities (renormalised if `norm`), per expert SiLU(gate) * up on HF's (gate | up) row halves of gate_up_w
    [E, 2I, H], down_w [E, H, I], the weighted sum onto the token.  Plain torch autograd, nothing is rounded inside: the caller passes
    float64 leaves holding the product's rounded inputs and differentiates `out` for dh, d router_w, d gate_up_w and d down_w."""
    E, I = gate_up_w.shape[0], down_w.shape[2]
    ids = ids.long()
    p = torch.softmax(h @ router_w.t(), -1)
    sel = p.gather(1, ids)
    w = sel / sel.sum(-1, keepdim=True) if norm else sel
    out = torch.zeros_like(h)
    for e in range(E):
        t, j = torch.where(ids == e)
        if t.numel() == 0:
            continue
        gu = h[t] @ gate_up_w[e].t()
        act = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        out = out.index_add(0, t, (act @ down_w[e].t()) * w[t, j, None])
    return out


def routing_safe_rows(h: torch.Tensor, router_w: torch.Tensor, k: int, dtype) -> torch.Tensor:
    """bool [T]: the rows whose top-k no rounding of the router GEMM can change - the float64 logit gap between the k-th and the
    (k+1)-th expert exceeds twice the row's largest logit error bound u |logit| + C32 sqrt(H) u32 (|h| |W|).  k = E: every row."""
    hd, wd = h.double(), router_w.double()
    logits = hd @ wd.t()
    T, E = logits.shape
    if k >= E:
        return torch.ones(T, dtype=torch.bool)
    err = U[dtype] * logits.abs() + C32 * np.sqrt(hd.shape[1]) * U32 * (hd.abs() @ wd.abs().t())
    srt = torch.sort(logits, dim=-1, descending=True).values
    return (srt[:, k - 1] - srt[:, k]) > 2 * err.max(-1).values


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
    """out[t] = sum_j w[t, j] y[row(t, j)] over the slots that have a row (row_of_pair -1: a dropped pair adds nothing), and |w| |y|."""
    rows = torch.as_tensor(row_of_pair).long().view(T, k)
    yy = y.double()[rows.clamp(min=0)] * (rows >= 0)[..., None]      # [T, k, H]
    ww = w.double()[..., None] if w is not None else torch.ones(T, k, 1, dtype=torch.float64)
    return (ww * yy).sum(1), (ww.abs() * yy.abs()).sum(1)
