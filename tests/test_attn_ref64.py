"""CPU checks of the float64 attention reference and its per-row bound (tests/attn_ref64.py): the reference agrees
with the fp32 oracle's autograd, an emulated bf16 kernel passes the bound, and one dropped key in one tile breaks it."""
import numpy as np
import torch

import attn_ref64 as R
import hostmirror
from dynamictreeattn_amd import packing
from oracle import trie_oracle as to
from oracle.attn_oracle import tree_attention


def _case(T_branch=150, P=100, Hq=4, Hkv=2, seed=0):
    seqs = [list(range(1000, 1000 + P)) + [1] + [5] * T_branch, list(range(1000, 1000 + P)) + [2] + [6] * 40]
    t = to.TokenTrieOracle([np.array(s) for s in seqs]); t.backward_permute()
    plan = packing.plan_segments(t.lens, t.lcp_lens)
    se = torch.from_numpy(hostmirror.expand_plan_host(plan)[3]).long()
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(plan.T, H, 128, generator=g).bfloat16().float() for H in (Hq, Hkv, Hkv, Hq))
    return q, k, v, do, se


def test_float64_reference_matches_the_fp32_oracle():
    q, k, v, do, se = _case()
    qr, kr, vr = (x.clone().requires_grad_(True) for x in (q, k, v))
    o, lse = tree_attention(qr, kr, vr, se)
    (o * do).sum().backward()
    ref = R.reference(q, k, v, do, o.detach(), se)
    for a, b in ((ref["out"], o), (ref["lse"], lse), (ref["dq"], qr.grad), (ref["dk"], kr.grad), (ref["dv"], vr.grad)):
        assert float((a - b.detach().double()).abs().max()) < 1e-4 * max(1.0, float(b.detach().abs().max()))


def test_bound_accepts_rounding_and_rejects_one_dropped_key():
    """Emulates the kernel's roundings (P to bf16 in PV, output to bf16): within half the bound.  Dropping ONE visible key for
    the rows of one 64-row tile (each row off by about |v| / n) breaks it."""
    q, k, v, do, se = _case()
    T, Hq = q.shape[0], q.shape[1]
    rep = Hq // k.shape[1]
    ref = R.reference(q, k, v, None, None, se)

    def emulate(drop=None):
        out = torch.empty(T, Hq, 128, dtype=torch.float64)
        idx = torch.arange(T)
        vis = (idx[None, :] <= idx[:, None]) & (idx[:, None] < se[None, :])
        if drop is not None:
            rows, key = drop
            vis[rows, key] = False
        for h in range(Hq):
            s = (q[:, h].double() @ k[:, h // rep].double().T) * 128 ** -0.5
            s = s.masked_fill(~vis, float("-inf"))
            p = torch.exp(s - s.max(1, keepdim=True).values)
            l = p.sum(1, keepdim=True)
            out[:, h] = (p.bfloat16().double() @ v[:, h // rep].double()) / l
        return out.bfloat16()

    assert R.check("out", emulate(), ref, torch.bfloat16) <= 0.5
    bad = emulate((slice(128, 192), 64))
    try:
        R.check("out", bad, ref, torch.bfloat16)
    except AssertionError as e:
        assert "visible" in str(e)
    else:
        raise AssertionError("a dropped key passed the per-row bound")
