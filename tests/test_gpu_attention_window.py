"""Sliding-window tree attention (dta_tree_attn_fwd / _bwd with window > 0) against a float64 reference with the per-row error bound of
tests/attn_ref64.py (its check helpers and constants, imported).  Visibility: key s is seen by row t iff it is an ancestor-or-self
(s <= t < subtree_end[s]; stack form: s <= t) and depth[t] - depth[s] < W.  The cases put chain ends, forks, stack offsets and the
window itself on the 64 / 128 tile edges, for D = 64 and 128, bf16 / f16 / fp32 and several GQA geometries; forced dK/dV splits
must be bitwise reproducible; no window and a window wider than the trie must give the bits of the run without a window."""
import dataclasses

import numpy as np
import pytest
import torch

import attn_ref64 as R
import hostmirror
from dynamictreeattn_amd import ops, packing, synth
from dynamictreeattn_amd._lib import lib
from oracle import trie_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def reference_vis(q, k, v, vis, do=None, out=None, scale=None):
    """attn_ref64.reference with an explicit visibility matrix vis [Tq, Tk] (bool): the same tensors and bound terms."""
    f = R._f64
    q, k, v, do, out = (f(x) for x in (q, k, v, do, out))
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    rep = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
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
        s = ((q[:, h] @ kk.T) * scale).masked_fill(~vis, float("-inf"))
        lse = torch.logsumexp(s, dim=1)
        p = torch.exp(s - lse[:, None])
        p2 = p * p
        r["out"][:, h], r["lse"][:, h] = p @ vv, lse
        r["out_R"][:, h] = (p2 @ nv2[:, g]).sqrt()
        nq2 = q[:, h].pow(2).sum(1)
        r["out_F"][:, h] = scale * nq2.sqrt() * ((p2 @ (nk2[:, g] * nv2[:, g])).sqrt() + (p2 @ nk2[:, g]).sqrt() * r["out"][:, h].norm(dim=1))
        r["out_Z"][:, h] = (visf @ nv2[:, g]).sqrt()
        if not bwd:
            continue
        dd, qq = do[:, h], q[:, h]
        ndo = dd.norm(dim=1)
        ds = p * (dd @ vv.T - (dd * out[:, h]).sum(1)[:, None])
        ds2 = ds * ds
        r["dq"][:, h] = scale * (ds @ kk)
        r["dk"][:, g] += scale * (ds.T @ qq)
        r["dv"][:, g] += p.T @ dd
        r["dq_R"][:, h] = scale * (ds2 @ nk2[:, g]).sqrt()
        r["dk_R"][:, g] += scale ** 2 * (ds2.T @ nq2)
        r["dv_R"][:, g] += p2.T @ (ndo * ndo)
        a = ndo[:, None] * (nv2[:, g].sqrt()[None, :] + out[:, h].norm(dim=1)[:, None])
        a2 = p2 * a * a
        r["dq_F"][:, h] = scale * (D * (a2 @ nk2[:, g]) + scale ** 2 * nq2 * (ds2 @ nk2[:, g].pow(2))).sqrt()
        r["dk_F"][:, g] += scale ** 2 * (D * (a2.T @ nq2) + scale ** 2 * nk2[:, g] * (ds2.T @ nq2.pow(2)))
        r["dv_F"][:, g] += scale ** 2 * nk2[:, g] * (p2.T @ (nq2 * ndo * ndo))
        zz = visf * (1 + a) ** 2
        r["dq_Z"][:, h] = scale * (zz @ nk2[:, g]).sqrt()
        r["dk_Z"][:, g] += scale ** 2 * (zz.T @ nq2)
        r["dv_Z"][:, g] += visf.T @ (ndo * ndo)
    if bwd:
        for x in ("dk_R", "dv_R", "dk_F", "dv_F", "dk_Z", "dv_Z"):
            r[x] = r[x].sqrt()
    return r


def _trie(seqs, order="backward"):
    t = to.TokenTrieOracle([np.array(s) for s in seqs])
    getattr(t, order + "_permute")()
    return packing.plan_segments(t.lens, t.lcp_lens)


def _chain(L):
    return [[7] + list(range(100, 100 + L - 1))]


def _prefix_trie(P):
    pre = list(range(1000, 1000 + P))
    return [pre + [1] + [5] * (318 - P), pre + [2] + [6] * 64, pre + [3] + [8] * 64]


def _inputs(Tq, Tk, Hq, Hkv, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Tq, Hq, D, generator=g)
    k, v = torch.randn(Tk, Hkv, D, generator=g), torch.randn(Tk, Hkv, D, generator=g)
    do = torch.randn(Tq, Hq, D, generator=g)
    return tuple(x.to(dtype).to(DEV) for x in (q, k, v, do))


def _metas(plan, W, Hkv):
    """(full meta, windowed meta built through the packing functions whatever W is, host depth / subtree_end / win_lo)."""
    _, depth, _, se = hostmirror.expand_plan_host(plan)
    se_d = torch.from_numpy(se).to(DEV)
    full = ops.meta_from_plan(plan, se_d, DEV, Hkv)
    wl = packing.window_lo_host(plan, W)
    rp, runs = packing.plan_qtile_runs_window(plan, wl)
    kq = packing.ktile_qend_window(packing.ktile_qend_host(plan), wl)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
    win = ops.attach_dkv_units(ops.TreeAttnMeta(T=plan.T, subtree_end=se_d, run_ptr=up(rp), runs=up(runs).view(-1, 4), ktile_qend=up(kq),
                                                win_lo=up(wl), window=W), Hkv)
    return full, win, depth, se, wl


def _vis_packed(depth, se, W):
    T = depth.shape[0]
    s = torch.arange(T)
    d = torch.from_numpy(depth.astype(np.int64))
    return (s[None, :] <= s[:, None]) & (s[:, None] < torch.from_numpy(se.astype(np.int64))[None, :]) & ((d[:, None] - d[None, :]) < W)


def _run(q, k, v, do, meta, scale, **kw):
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, scale)
    dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale, **kw)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _packed_case(seqs, W, Hq, Hkv, D, dtype, order="backward", seed=0):
    plan = _trie(seqs, order)
    full, win, depth, se, wl = _metas(plan, W, Hkv)
    q, k, v, do = _inputs(plan.T, plan.T, Hq, Hkv, D, dtype, seed)
    out, lse, dq, dk, dv = _run(q, k, v, do, win, D ** -0.5)
    ref = reference_vis(q, k, v, _vis_packed(depth, se, W), do, out, D ** -0.5)
    R.check_all(ref, dtype, f"window W={W} T={plan.T} D={D} {Hq}/{Hkv} {order}", out=out, lse=lse, dq=dq, dk=dk, dv=dv)
    return plan, (full, win), (q, k, v, do), (out, lse, dq, dk, dv)


# ------------------------------------------------------------------------------------------------ packed trie: tile edges
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize("seqs", [_chain(1025), _chain(129), _prefix_trie(128)], ids=["chain1025", "chain129", "prefix128"])
def test_window_packed_against_float64(seqs, W, D, dtype):
    _packed_case(seqs, W, 2, 1, D, dtype, seed=W)


@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("hq,hkv", [(1, 1), (2, 1), (14, 2), (16, 8)])
def test_window_head_geometries(hq, hkv, D, dtype):
    for order in ("forward", "backward"):
        _packed_case(_prefix_trie(65), 100, hq, hkv, D, dtype, order, seed=hq + hkv)


def test_window_lo_device_matches_host():
    for seqs in (_chain(1025), _prefix_trie(64), synth.tau2(0)):
        plan = _trie(seqs)
        _, depth, _, _ = hostmirror.expand_plan_host(plan)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
        for W in (1, 64, 1024, 4096):
            got = ops.window_lo_device(up(depth), up(plan.seg_off), up(plan.seg_depth0), up(plan.parent_of_seg), W)
            np.testing.assert_array_equal(got.cpu().numpy(), packing.window_lo_host(plan, W))


# ------------------------------------------------------------------------------------------------ stack form
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("start", [0, 63, 128, 4095])
@pytest.mark.parametrize("W", [1, 64, 130])
def test_window_stack_form_offsets_and_accumulate(W, start, D, dtype):
    Hq, Hkv = 14, 2
    scale = D ** -0.5
    for B in (65, 129):
        q, k, v, do = _inputs(B, start + B, Hq, Hkv, D, dtype, seed=start + B + W)
        meta = ops.stack_meta(start, W)
        out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, scale)
        qi = start + torch.arange(B)[:, None]
        kj = torch.arange(start + B)[None, :]
        ref = reference_vis(q, k, v, (kj <= qi) & (qi - kj < W), do, out, scale)
        g = torch.Generator().manual_seed(start + 7 * B)
        bk, bv = (torch.randn(start + B, Hkv, D, generator=g) for _ in range(2))
        for acc in (0, 1, 2):
            if acc == 0:
                dk = dv = None
            elif acc == 1:
                dk, dv = bk.to(dtype).to(DEV), bv.to(dtype).to(DEV)
            else:
                dk, dv = bk.to(DEV), bv.to(DEV)
            base = None if acc == 0 else (dk.clone(), dv.clone())
            dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale, dk=dk, dv=dv, accumulate=acc)
            torch.cuda.synchronize()
            label = f"window stack W={W} start={start} B={B} D={D} accumulate={acc}"
            if acc == 0:
                R.check_all(ref, dtype, label, out=out, lse=lse)
            R.check("dq", dq, ref, dtype, label)
            R.check("dk", dk, ref, dtype, label, base=None if base is None else base[0])
            R.check("dv", dv, ref, dtype, label, base=None if base is None else base[1])


# ------------------------------------------------------------------------------------------------ forced dK/dV splits
@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("W", [64, 300])
def test_window_forced_dkv_splits(W, D, dtype):
    Hq, Hkv = 14, 2
    plan = _trie(_chain(1025))
    _, win, depth, se, _ = _metas(plan, W, Hkv)
    units, splits, n_slabs = packing.plan_dkv_units(win.ktile_qend.cpu().numpy(), plan.T, plan.T, 0, Hkv, n_cu=1 << 20, min_tiles=1)
    assert splits.shape[0] > 0
    split = dataclasses.replace(win, dkv_units=torch.from_numpy(units).to(DEV), dkv_splits=torch.from_numpy(splits).to(DEV), n_slabs=n_slabs)
    unsplit = dataclasses.replace(win, dkv_units=None, dkv_splits=None, n_slabs=0)
    q, k, v, do = _inputs(plan.T, plan.T, Hq, Hkv, D, dtype, seed=W)
    scale = D ** -0.5
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, split, scale)
    runs = [ops.attn_bwd_raw(q, k, v, out, do, lse, split, scale) for _ in range(2)]
    one = ops.attn_bwd_raw(q, k, v, out, do, lse, unsplit, scale)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "split windowed dK/dV sweep is not bitwise reproducible"
    ref = reference_vis(q, k, v, _vis_packed(depth, se, W), do, out, scale)
    R.check_all(ref, dtype, f"window split W={W} D={D}", dq=runs[0][0], dk=runs[0][1], dv=runs[0][2])
    assert torch.equal(runs[0][0], one[0])
    for i in (1, 2):
        a, b = runs[0][i].double().cpu(), one[i].double().cpu()
        assert bool(((a - b).norm(dim=-1) <= 2 * R.U[dtype] * b.norm(dim=-1) + 1e-30).all())


# ------------------------------------------------------------------------------------------------ no window = the kernels without one, bit for bit
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("D", [64, 128])
def test_no_window_and_wide_window_equal_ex_bitwise(D, dtype):
    Hq, Hkv = 16, 8
    plan = _trie(_prefix_trie(128))
    W = packing.max_depth(plan) + 1
    full, win, *_ = _metas(plan, W, Hkv)
    assert win.window == W and win.win_lo is not None
    q, k, v, do = _inputs(plan.T, plan.T, Hq, Hkv, D, dtype, seed=1)
    a = _run(q, k, v, do, full, D ** -0.5)
    b = _run(q, k, v, do, win, D ** -0.5)                           # the windowed kernels on a window wider than the trie
    c = _run(q, k, v, do, dataclasses.replace(full, window=0), D ** -0.5)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    # window_meta hands back the full meta when the window changes nothing
    assert ops.window_meta(full, plan, torch.zeros(plan.T, dtype=torch.int32, device=DEV), W, Hkv) is full
    # stack form: a window wider than the stack equals no window
    qs, ks, vs, ds = _inputs(129, 129 + 64, Hq, Hkv, D, dtype, seed=2)
    s0 = _run(qs, ks, vs, ds, ops.stack_meta(64), D ** -0.5)
    s1 = _run(qs, ks, vs, ds, ops.stack_meta(64, 100000), D ** -0.5)
    for x, y in zip(s0, s1):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ C interface
def test_window_c_interface_codes():
    P = lambda t: None if t is None else t.data_ptr()
    Hq, Hkv, hd, T = 2, 1, 64, 4
    q = torch.zeros(T, Hq, hd, dtype=BF, device=DEV); kv = torch.zeros(T, Hkv, hd, dtype=BF, device=DEV)
    o = torch.empty_like(q); lse = torch.zeros(Hq, T, device=DEV)
    se = torch.full((T,), T, dtype=torch.int32, device=DEV); wl = torch.zeros(T, dtype=torch.int32, device=DEV)
    dl = torch.zeros(Hq, T, device=DEV); dq = torch.empty_like(q); dk = torch.empty_like(kv); dv = torch.empty_like(kv)

    def fwd(se_, wl_, W):
        return lib().dta_tree_attn_fwd(P(q), P(kv), P(kv), P(o), P(lse), P(se_), None, None, T, T, 0, Hq, Hkv, hd,
                                       Hq * hd, hd, Hkv * hd, hd, Hkv * hd, hd, Hq * hd, hd, 0.1, 0, P(wl_), W, 0.0, None)

    def bwd(se_, wl_, W):
        return lib().dta_tree_attn_bwd(P(q), P(kv), P(kv), P(o), P(o), P(lse), P(dl), P(dq), P(dk), P(dv), P(se_), None, None, None,
                                       T, T, 0, Hq, Hkv, hd, Hq * hd, hd, Hkv * hd, hd, Hkv * hd, hd, Hq * hd, hd, Hq * hd, hd,
                                       Hkv * hd, hd, 0.1, 0, 0, 3, None, 0, None, 0, None, P(wl_), W, 0.0, None)
    for f in (fwd, bwd):
        assert f(se, wl, 0) == -1              # win_lo without a window
        assert f(None, wl, -3) == -1
        assert f(se, None, 8) == -1            # packed trie without win_lo
        assert f(se, None, 0) == 0             # no window
        assert f(se, wl, 8) == 0
        assert f(None, None, 8) == 0           # stack form
        torch.cuda.synchronize()
    assert lib().dta_window_lo(P(se), P(se), P(se), P(se), 1, T, 0, P(wl), None) == -1


# ------------------------------------------------------------------------------------------------ full size
@pytest.mark.parametrize("hq,hkv,D", [(16, 8, 128), (14, 2, 64)])
def test_window_full_size_tau2(hq, hkv, D):
    """The tau2 trie at W = 4096: the rows of one leaf path equal a windowed dense causal run over that path, forward and dQ."""
    plan = _trie(synth.tau2(0))
    T = plan.T
    _, depth, _, se = hostmirror.expand_plan_host(plan)
    se_d, depth_d = torch.from_numpy(se).to(DEV), torch.from_numpy(depth).to(DEV)
    W = 4096
    assert packing.max_depth(plan) >= W
    meta = ops.window_meta(ops.meta_from_plan(plan, se_d, DEV, hkv), plan, depth_d, W, hkv)
    assert meta.window == W
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(T, H, D, generator=g).bfloat16().to(DEV) for H in (hq, hkv, hkv, hq))
    scale = D ** -0.5
    o, lse, dq, dk, dv = _run(q, k, v, do, meta, scale)
    rel = lambda a, b: float((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm())
    leaf = max(range(plan.M), key=lambda i: plan.seg_off[i + 1] - plan.seg_off[i] + sum(e - b for b, e in plan.path_runs[i]))
    idx = np.concatenate([np.arange(b, e) for b, e in plan.path_runs[leaf]] + [np.arange(plan.seg_off[leaf], plan.seg_off[leaf + 1])])
    assert idx.size > W
    ix = torch.from_numpy(idx).to(DEV)
    od, lsed, dqd, _, _ = _run(q[ix].contiguous(), k[ix].contiguous(), v[ix].contiguous(), do[ix].contiguous(), ops.stack_meta(0, W), scale)
    assert rel(o[ix], od) < 4e-3
    assert rel(dq[ix], dqd) < 1e-2                  # dQ of a row depends on its own path alone
    assert bool(torch.isfinite(dk.float()).all()) and bool(torch.isfinite(dv.float()).all())
