"""Float64 reference of the tree-attention operator and a per-(row, head) error bound for the HIP kernels.

Visibility: query row i sits at packed / stack position qi = q_offset + i and sees key j iff
j <= qi and qi < subtree_end[j] (no subtree bound in the stack form).

The forward reference takes the kernel's rounded inputs.  The backward is checked as an operator on the
kernel's own inputs: D_i = rowsum(dO_i * out_i) uses the `out` the forward kernel returned (the C ABI's
definition), so the gradient error is not mixed with the forward's output rounding.

Bound (u = 2^-8 bf16, 2^-11 f16, 2^-24 fp32; u32 = 2^-24; p exact probabilities, ds_ij = p_ij (dP_ij - D_i);
n = the row's visible-key count, or for a key row the number of (query, head) pairs that see it;
"sum_hi" runs over the rows and query heads of the kv group; |x| is a row's 2-norm):

    bound = c * [ u (R + |ref row|) + u32 (F + sqrt(n) |ref row|) + tiny Z ]
    R  out_i : sqrt(sum_j p_ij^2 |v_j|^2)                 dV_j : sqrt(sum_hi p_ij^2 |dO_i|^2)
       dQ_i  : scale sqrt(sum_j ds_ij^2 |k_j|^2)          dK_j : scale sqrt(sum_hi ds_ij^2 |q_i|^2)
    lse_i : c * 1e-5 * (1 + |lse_i|)   (absolute, natural log)

R is a root-sum-square because the roundings of P (to bf16/f16 for the PV and dV MFMAs) and of dS are
independent, so their errors add in quadrature.  A worst-case linear form (u sum_j p_ij |v_j|) would be up to
sqrt(n) times larger and would hide a dropped or extra key.  With the RSS form a one-key error (about |v| / n)
breaks the bound up to n ~ (1 / (c u))^2, a few thousand keys in bf16.  The |ref row| term covers the final
rounding of the output.

The u32 terms are the fp32 floor.  sqrt(n) |ref row| is fp32 accumulation over n terms.  F adds two more parts.
The first is the cancellation of dP - D, which both kernels form in fp32 from length-128 dots
(a_ij = |dO_i| (|v_j| + |out_i|) bounds |dP_ij - D_i|):
    dQ_i: scale sqrt(128 sum_j p_ij^2 a_ij^2 |k_j|^2),  dK_j: scale sqrt(128 sum_hi p_ij^2 a_ij^2 |q_i|^2).
This is the only term for a row whose exact gradient is zero, such as a row that sees only itself.  The second
part is the fp32 rounding of the scores, e_ij ~ scale |q_i| |k_j|, which the exponential turns into a relative
error of P.  It dominates the fp32 kernels when the scores are large:
    out_i: scale |q_i| (sqrt(sum_j p_ij^2 |k_j|^2 |v_j|^2) + sqrt(sum_j p_ij^2 |k_j|^2) |out_i|)
    dV_j : scale |k_j| sqrt(sum_hi p_ij^2 |q_i|^2 |dO_i|^2)
    dQ_i : scale^2 |q_i| sqrt(sum_j ds_ij^2 |k_j|^4),   dK_j: scale^2 |k_j| sqrt(sum_hi ds_ij^2 |q_i|^4)
Z is the range floor.  A P (or dS) below the smallest value the kernel resolves (TINY: fp32's normal range, which
bf16 shares; f16's subnormal spacing) may come out as 0:
    out_i: sqrt(sum_j vis |v_j|^2),  dV_j: sqrt(sum_hi vis |dO_i|^2),
    dQ_i: scale sqrt(sum_j vis (1 + a_ij)^2 |k_j|^2),  dK_j: scale sqrt(sum_hi vis (1 + a_ij)^2 |q_i|^2).

The constants c (one per tensor and input type) are in C below.  They were calibrated on the MI355X over the
cases of tests/test_gpu_attention_edges.py and tests/test_gpu_attention.py, so that the current kernels stay at
or below half the bound everywhere.  The largest observed ratios err / bound are listed in
tests/test_gpu_attention_edges.py's docstring.
"""
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U32 = 2.0 ** -24
# c per input dtype and tensor (see the module docstring)
C = {
    torch.bfloat16: {"out": 1.5, "lse": 1.0, "dq": 3.0, "dk": 1.5, "dv": 1.5},
    torch.float16: {"out": 1.5, "lse": 1.0, "dq": 3.0, "dk": 1.5, "dv": 1.5},
    torch.float32: {"out": 10.0, "lse": 1.0, "dq": 5.0, "dk": 25.0, "dv": 60.0},
}
LSE_U = 1e-5
# smallest P (and dS) the kernels resolve: fp32's normal range (bf16 shares it), f16's subnormal spacing
TINY = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -24, torch.float32: 2.0 ** -126}

# largest err / bound seen per (dtype, tensor) in this process (read by the calibration notes of the docstrings)
WORST = {}


def _f64(x):
    return None if x is None else x.detach().to("cpu", torch.float64)


def reference(q, k, v, do=None, out=None, subtree_end=None, q_offset=0, scale=None):
    """Float64 forward (and, given dO and the kernel's `out`, backward) with the bound terms.
    q/do/out [Tq,Hq,D], k/v [Tk,Hkv,D] (any dtype/device: the rounded values the kernel saw).
    Returns a dict of float64 CPU tensors: out, lse (natural log, [Tq,Hq]) and, with dO, dq/dk/dv, plus for every
    tensor X: X_R, X_F and X_Z (the bound terms of the module docstring, without c and u) and X_n (visible counts)."""
    q, k, v, do, out = (_f64(x) for x in (q, k, v, do, out))
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    rep = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    qi = q_offset + torch.arange(Tq)
    kj = torch.arange(Tk)
    vis = kj[None, :] <= qi[:, None]
    if subtree_end is not None:
        vis &= qi[:, None] < subtree_end.detach().cpu().long()[None, :Tk]
    visf = vis.double()
    nvis_q = visf.sum(1)                                   # [Tq]
    nvis_k = visf.sum(0)                                   # [Tk]
    nk2, nv2 = k.pow(2).sum(-1), v.pow(2).sum(-1)          # [Tk,Hkv]
    r = {"out": torch.empty(Tq, Hq, D, dtype=torch.float64), "lse": torch.empty(Tq, Hq, dtype=torch.float64),
         "out_R": torch.empty(Tq, Hq, dtype=torch.float64), "out_F": torch.empty(Tq, Hq, dtype=torch.float64),
         "out_Z": torch.empty(Tq, Hq, dtype=torch.float64),
         "out_n": nvis_q[:, None].expand(Tq, Hq), "lse_n": nvis_q[:, None].expand(Tq, Hq)}
    bwd = do is not None
    if bwd:
        r.update({"dq": torch.empty(Tq, Hq, D, dtype=torch.float64), "dq_R": torch.empty(Tq, Hq, dtype=torch.float64),
                  "dq_F": torch.empty(Tq, Hq, dtype=torch.float64), "dq_n": nvis_q[:, None].expand(Tq, Hq),
                  "dq_Z": torch.empty(Tq, Hq, dtype=torch.float64),
                  "dk_Z": torch.zeros(Tk, Hkv, dtype=torch.float64), "dv_Z": torch.zeros(Tk, Hkv, dtype=torch.float64),
                  "dk": torch.zeros(Tk, Hkv, D, dtype=torch.float64), "dv": torch.zeros(Tk, Hkv, D, dtype=torch.float64),
                  "dk_R": torch.zeros(Tk, Hkv, dtype=torch.float64), "dv_R": torch.zeros(Tk, Hkv, dtype=torch.float64),
                  "dk_F": torch.zeros(Tk, Hkv, dtype=torch.float64), "dv_F": torch.zeros(Tk, Hkv, dtype=torch.float64),
                  "dk_n": (rep * nvis_k)[:, None].expand(Tk, Hkv), "dv_n": (rep * nvis_k)[:, None].expand(Tk, Hkv)})
    blk = max(1, min(Tq, (1 << 22) // max(Tk, 1)))            # query rows per block: a few [blk, Tk] float64 temporaries
    for h in range(Hq):
        g = h // rep
        kk, vv = k[:, g], v[:, g]
        for i0 in range(0, Tq, blk):
            i1 = min(Tq, i0 + blk)
            s = (q[i0:i1, h] @ kk.T) * scale
            s = s.masked_fill(~vis[i0:i1], float("-inf"))
            lse = torch.logsumexp(s, dim=1)
            p = torch.exp(s - lse[:, None])
            p2 = p * p
            r["out"][i0:i1, h], r["lse"][i0:i1, h] = p @ vv, lse
            r["out_R"][i0:i1, h] = (p2 @ nv2[:, g]).sqrt()
            nq2 = q[i0:i1, h].pow(2).sum(1)
            r["out_F"][i0:i1, h] = scale * nq2.sqrt() * ((p2 @ (nk2[:, g] * nv2[:, g])).sqrt()
                                                         + (p2 @ nk2[:, g]).sqrt() * r["out"][i0:i1, h].norm(dim=1))
            r["out_Z"][i0:i1, h] = (visf[i0:i1] @ nv2[:, g]).sqrt()
            if not bwd:
                continue
            dd, qq = do[i0:i1, h], q[i0:i1, h]
            ndo = dd.norm(dim=1)
            Dl = (dd * out[i0:i1, h]).sum(1)
            ds = p * (dd @ vv.T - Dl[:, None])
            ds2 = ds * ds
            r["dq"][i0:i1, h] = scale * (ds @ kk)
            r["dk"][:, g] += scale * (ds.T @ qq)
            r["dv"][:, g] += p.T @ dd
            r["dq_R"][i0:i1, h] = scale * (ds2 @ nk2[:, g]).sqrt()
            r["dk_R"][:, g] += scale ** 2 * (ds2.T @ nq2)
            r["dv_R"][:, g] += p2.T @ (ndo * ndo)
            a = ndo[:, None] * (nv2[:, g].sqrt()[None, :] + out[i0:i1, h].norm(dim=1)[:, None])      # bounds |dP_ij - D_i|
            a2 = p2 * a * a
            r["dq_F"][i0:i1, h] = scale * (D * (a2 @ nk2[:, g]) + scale ** 2 * nq2 * (ds2 @ nk2[:, g].pow(2))).sqrt()
            r["dk_F"][:, g] += scale ** 2 * (D * (a2.T @ nq2) + scale ** 2 * nk2[:, g] * (ds2.T @ nq2.pow(2)))
            r["dv_F"][:, g] += scale ** 2 * nk2[:, g] * (p2.T @ (nq2 * ndo * ndo))
            z = visf[i0:i1] * (1 + a) ** 2
            r["dq_Z"][i0:i1, h] = scale * (z @ nk2[:, g]).sqrt()
            r["dk_Z"][:, g] += scale ** 2 * (z.T @ nq2)
            r["dv_Z"][:, g] += visf[i0:i1].T @ (ndo * ndo)
    if bwd:
        for x in ("dk_R", "dv_R", "dk_F", "dv_F", "dk_Z", "dv_Z"):
            r[x] = r[x].sqrt()
    return r


def check(name, got, ref, dtype, label="", base=None, c=None):
    """Asserts |got_row - ref_row|_2 <= bound for every (row, head) of tensor `name` (out / dq / dk / dv / lse);
    `got` in the kernel's layout (lse: the kernel's [Hq,Tq] log2 values).  `base`: what an accumulating launch added onto.
    Returns the largest err / bound."""
    c = C[dtype][name] if c is None else c
    if name == "lse":
        g = _f64(got).T * math.log(2.0)
        want = ref["lse"]
        err = (g - want).abs()
        bound = c * LSE_U * (1.0 + want.abs())
    else:
        want = ref[name] if base is None else ref[name] + _f64(base)
        g = _f64(got)
        err = (g - want).norm(dim=-1)
        N = want.norm(dim=-1)
        n = ref[name + "_n"]
        bound = c * (U[dtype] * (ref[name + "_R"] + N) + U32 * (ref[name + "_F"] + n.sqrt() * N) + TINY[dtype] * ref[name + "_Z"])
    ratio = err / (bound + 1e-300)
    ratio = torch.where(torch.isfinite(g if name == "lse" else g.sum(-1)), ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max())
    key = (str(dtype).split(".")[-1], name)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        row, head = divmod(int(ratio.argmax()), ratio.shape[1])
        raise AssertionError(f"{label} {name} ({key[0]}): row {row} head {head} err/bound {worst:.3g} "
                             f"(err {float(err[row, head]):.3e}, bound {float(bound[row, head]):.3e}, "
                             f"{int(ref[name + '_n'][row, head]) if name != 'lse' else int(ref['lse_n'][row, head])} visible)")
    return worst


def check_all(ref, dtype, label="", out=None, lse=None, dq=None, dk=None, dv=None, dk_base=None, dv_base=None):
    """check() on every tensor given; returns {name: worst ratio}."""
    res = {}
    for name, got, base in (("out", out, None), ("lse", lse, None), ("dq", dq, None), ("dk", dk, dk_base), ("dv", dv, dv_base)):
        if got is not None:
            res[name] = check(name, got, ref, dtype, label, base)
    return res
