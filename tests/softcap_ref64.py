"""Float64 reference of SOFT-CAPPED tree attention with an explicit visibility matrix, and its per-row error-bound terms.

With z_ij = scale (q_i . k_j), c the cap and t_ij = tanh(z_ij / c):

    s_ij = c t_ij  (capped FIRST, then masked by `vis`, then the softmax)        lse_i = log sum_j exp(s_ij)
    p = exp(s - lse),  out = p V,  ds = p (dP - D),  dz = ds (1 - t^2)
    dq = scale dz K,   dk = scale dz^T Q,   dv = p^T dO

It extends `reference_vis` of tests/test_gpu_attention_window.py and returns the same tensors and bound terms (X_R, X_F, X_Z, X_n of
tests/attn_ref64.py, to be used with attn_ref64.check / check_all and its constants C), with two changes:

* `ds` is replaced by `dz = ds (1 - t^2)` in the dQ / dK terms (R, and the score-rounding part of F);
* F gets one more part.  The kernels form tanh in fp32 with an absolute error of a few 2^-24, i.e. an absolute error of the order of
  c 2^-24 per capped score.  It is propagated the way the existing score-rounding part (e_ij ~ scale |q_i| |k_j|, a relative error of
  P) is, with e_ij = c:
      out_i: c (sqrt(sum_j p_ij^2 |v_j|^2) + sqrt(sum_j p_ij^2) |out_i|)
      dV_j : c sqrt(sum_hi p_ij^2 |dO_i|^2)
      dQ_i : scale c sqrt(sum_j dz_ij^2 |k_j|^2),   dK_j: scale c sqrt(sum_hi dz_ij^2 |q_i|^2)
  (added in quadrature where the existing parts are, linearly for out).

softcap = 0 / None: no cap - the terms of reference_vis exactly.

`cap_changes` states the condition a capped test case must meet to prove anything: the references with and without the cap differ,
for every tensor, by at least `factor` x the bound on some row."""
import math

import torch

import attn_ref64 as R


def reference_cap(q, k, v, vis, do=None, out=None, scale=None, softcap=0.0):
    """q/do/out [Tq,Hq,D], k/v [Tk,Hkv,D], vis [Tq,Tk] bool.  `out`: the kernel's forward output (delta = rowsum(dO * out) is
    the C ABI's definition); None: the reference's own."""
    f = R._f64
    q, k, v, do, out = (f(x) for x in (q, k, v, do, out))
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    rep = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    c = float(softcap or 0.0)
    visf = vis.double()
    nq, nk = visf.sum(1), visf.sum(0)
    nk2, nv2 = k.pow(2).sum(-1), v.pow(2).sum(-1)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    r = {"out": z(Tq, Hq, D), "lse": z(Tq, Hq), "out_R": z(Tq, Hq), "out_F": z(Tq, Hq), "out_Z": z(Tq, Hq),
         "out_n": nq[:, None].expand(Tq, Hq), "lse_n": nq[:, None].expand(Tq, Hq)}
    bwd = do is not None
    if bwd:
        r.update({"dq": z(Tq, Hq, D), "dq_R": z(Tq, Hq), "dq_F": z(Tq, Hq), "dq_Z": z(Tq, Hq), "dq_n": nq[:, None].expand(Tq, Hq),
                  "dk": z(Tk, Hkv, D), "dv": z(Tk, Hkv, D)})
        for x in ("dk_R", "dv_R", "dk_F", "dv_F", "dk_Z", "dv_Z"):
            r[x] = z(Tk, Hkv)
        r["dk_n"] = r["dv_n"] = (rep * nk)[:, None].expand(Tk, Hkv)
    for h in range(Hq):
        g = h // rep
        kk, vv = k[:, g], v[:, g]
        zz_ = (q[:, h] @ kk.T) * scale
        if c > 0:
            t = torch.tanh(zz_ / c)
            s, sech2 = c * t, 1.0 - t * t
        else:
            s, sech2 = zz_, torch.ones_like(zz_)
        s = s.masked_fill(~vis, float("-inf"))
        lse = torch.logsumexp(s, dim=1)
        p = torch.exp(s - lse[:, None])
        p2 = p * p
        r["out"][:, h], r["lse"][:, h] = p @ vv, lse
        r["out_R"][:, h] = (p2 @ nv2[:, g]).sqrt()
        nq2 = q[:, h].pow(2).sum(1)
        on = r["out"][:, h].norm(dim=1)
        r["out_F"][:, h] = (scale * nq2.sqrt() * ((p2 @ (nk2[:, g] * nv2[:, g])).sqrt() + (p2 @ nk2[:, g]).sqrt() * on)
                            + c * ((p2 @ nv2[:, g]).sqrt() + p2.sum(1).sqrt() * on))
        r["out_Z"][:, h] = (visf @ nv2[:, g]).sqrt()
        if not bwd:
            continue
        dd, qq = do[:, h], q[:, h]
        oo = out[:, h] if out is not None else r["out"][:, h]
        ndo = dd.norm(dim=1)
        ds = p * (dd @ vv.T - (dd * oo).sum(1)[:, None])
        dz = ds * sech2
        dz2 = dz * dz
        r["dq"][:, h] = scale * (dz @ kk)
        r["dk"][:, g] += scale * (dz.T @ qq)
        r["dv"][:, g] += p.T @ dd
        r["dq_R"][:, h] = scale * (dz2 @ nk2[:, g]).sqrt()
        r["dk_R"][:, g] += scale ** 2 * (dz2.T @ nq2)
        r["dv_R"][:, g] += p2.T @ (ndo * ndo)
        a = ndo[:, None] * (nv2[:, g].sqrt()[None, :] + oo.norm(dim=1)[:, None])
        a2 = p2 * a * a
        r["dq_F"][:, h] = scale * (D * (a2 @ nk2[:, g]) + scale ** 2 * nq2 * (dz2 @ nk2[:, g].pow(2)) + c * c * (dz2 @ nk2[:, g])).sqrt()
        r["dk_F"][:, g] += scale ** 2 * (D * (a2.T @ nq2) + scale ** 2 * nk2[:, g] * (dz2.T @ nq2.pow(2)) + c * c * (dz2.T @ nq2))
        r["dv_F"][:, g] += scale ** 2 * nk2[:, g] * (p2.T @ (nq2 * ndo * ndo)) + c * c * (p2.T @ (ndo * ndo))
        zz = visf * (1 + a) ** 2
        r["dq_Z"][:, h] = scale * (zz @ nk2[:, g]).sqrt()
        r["dk_Z"][:, g] += scale ** 2 * (zz.T @ nq2)
        r["dv_Z"][:, g] += visf.T @ (ndo * ndo)
    if bwd:
        for x in ("dk_R", "dv_R", "dk_F", "dv_F", "dk_Z", "dv_Z"):
            r[x] = r[x].sqrt()
    return r


def bound(name, ref, dtype):
    """The bound attn_ref64.check applies to tensor `name` of `ref`, per (row, head)."""
    c = R.C[dtype][name]
    if name == "lse":
        return c * R.LSE_U * (1.0 + ref["lse"].abs())
    N = ref[name].norm(dim=-1)
    return c * (R.U[dtype] * (ref[name + "_R"] + N) + R.U32 * (ref[name + "_F"] + ref[name + "_n"].sqrt() * N) + R.TINY[dtype] * ref[name + "_Z"])


def cap_changes(ref_cap, ref_nocap, dtype, names=("out", "lse", "dq", "dk", "dv")):
    """{tensor: largest over the rows of |capped - uncapped| / bound}: how far, in units of the kernel's error bound, the cap moves the
    result.  From the float64 references alone."""
    res = {}
    for name in names:
        if name not in ref_cap:
            continue
        d = (ref_cap[name] - ref_nocap[name]).abs() if name == "lse" else (ref_cap[name] - ref_nocap[name]).norm(dim=-1)
        res[name] = float((d / (bound(name, ref_cap, dtype) + 1e-300)).max())
    return res


def assert_cap_matters(ref_cap, ref_nocap, dtype, label="", factor=10.0, names=("out", "lse", "dq", "dk", "dv")):
    ch = cap_changes(ref_cap, ref_nocap, dtype, names)
    weak = {n: round(v, 2) for n, v in ch.items() if not v >= factor}
    assert not weak, f"{label}: the cap moves {weak} by less than {factor} x the bound - the case would pass without a cap"
    return ch


def plain_capped_attention(q, k, v, vis, scale, softcap):
    """The plain formula in torch (differentiable, any dtype): softmax(mask(c tanh(scale q k^T / c))) v with GQA head repetition."""
    rep = q.shape[1] // k.shape[1]
    kk, vv = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    s = torch.einsum("ihd,jhd->hij", q, kk) * scale
    if softcap:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~vis[None], -math.inf)
    return torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), vv), torch.logsumexp(s, dim=-1).T
