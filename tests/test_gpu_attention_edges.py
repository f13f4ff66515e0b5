"""Tree attention at the kernels' tile edges, score ranges and work splits, every (row, head) checked against a float64
reference with the per-row bound of tests/attn_ref64.py (its docstring states the bound formulas and the constants c).

The kernels tile as follows: fwd and dQ take 128 query rows per workgroup (odd GQA groups a separate 4-wave path) and
64-key K/V tiles; dK/dV takes 128 keys per workgroup and sweeps 64-row query tiles split in two halves of 32 rows; the
fp32 kernels take 64 rows per workgroup.  The cases below put chain ends, forks, subtree ends and stack offsets on and
next to those edges, drive the forward's deferred maximum (rescale only when a row's maximum rises by more than 4 in
the log2 domain) through its rescale branch, underflow P to zero, force every dK/dV key tile into split units, and
reach the C-ABI paths the product only takes in special situations (no run list, no ktile_qend, the three-launch
backward of the kernel timer, strided fused buffers).

Largest err / bound observed on the MI355X with the constants c of attn_ref64.C, over this module and test_gpu_attention.py.
Each bound must stay at or below 0.5:

    tensor   c bf16 / f16 / fp32     largest ratio bf16 / f16 / fp32
    out      1.5 / 1.5 / 10          0.35 / 0.36 / 0.43
    lse      1   / 1   / 1           0.19 / 0.21 / 0.43
    dQ       3   / 3   / 5           0.42 / 0.36 / 0.48
    dK       1.5 / 1.5 / 25          0.43 / 0.41 / 0.45
    dV       1.5 / 1.5 / 60          0.39 / 0.37 / 0.46

The largest bf16/f16 ratios come from the rising-maximum and long-row cases (dQ) and the tile-edge chains (out).  The fp32
ratios come from the large-score cases, where the fp32 rounding of the scores dominates.

test_no_run_list_and_no_ktile_qend pins a kernel bug these tests found.  With runs = NULL and a subtree bound, the bf16/f16
forward and dQ kernels treated key tiles below the diagonal as unmasked: rows saw keys outside their root path.
"""
import dataclasses
import math

import numpy as np
import pytest
import torch

import attn_ref64 as R
import hostmirror
from dynamictreeattn_amd import ops, packing
from oracle import trie_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
SCALE = D ** -0.5
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


# ------------------------------------------------------------------------------------------------ inputs and runs
def _trie(seqs, order="backward"):
    t = to.TokenTrieOracle([np.array(s) for s in seqs])
    getattr(t, order + "_permute")()
    plan = packing.plan_segments(t.lens, t.lcp_lens)
    se = hostmirror.expand_plan_host(plan)[3]
    return plan, torch.from_numpy(se).long()


def _inputs(Tq, Tk, Hq, Hkv, dtype, seed=0, kind="randn", q_offset=0, sigma=1.0, beta=2.0, gamma=8.0):
    """q/do [Tq,Hq,D], k/v [Tk,Hkv,D] in `dtype` on the host.
    kind "randn": N(0,1) (q times sigma: scores with standard deviation sigma);
    "rising": q_i = b_i u + noise, k_j = (j/Tk) gamma u + noise along a shared direction u (|u|^2 = D): every row's maximum
        rises with every key tile; b_i runs over [0, beta] inside each 64-row tile so that some rows of a wave trigger the
        rescale and others ride along;
    "falling": k_j = (1 - 2j/Tk) gamma u + noise: the maximum sits in the first tile and P underflows to 0 further on."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Tq, Hq, D, generator=g) * sigma
    k, v = torch.randn(Tk, Hkv, D, generator=g), torch.randn(Tk, Hkv, D, generator=g)
    do = torch.randn(Tq, Hq, D, generator=g)
    if kind != "randn":
        u = torch.randn(D, generator=g)
        u = u / u.norm() * math.sqrt(D)
        pos = torch.arange(Tk, dtype=torch.float32) / Tk
        slope = pos * gamma if kind == "rising" else (1 - 2 * pos) * gamma
        k = k + slope[:, None, None] * u
        rows = q_offset + torch.arange(Tq)
        b = beta * ((rows % 64).float() / 63.0) if kind == "rising" else torch.full((Tq,), beta)
        hb = 1.0 - 0.25 * torch.arange(Hq, dtype=torch.float32) / max(Hq, 1)       # heads differ too
        q = q + b[:, None, None] * hb[None, :, None] * u
    return tuple(x.to(dtype) for x in (q, k, v, do))


def _dev(*xs):
    return tuple(x.to(DEV) for x in xs)


def _fwd_bwd(q, k, v, do, meta, **kw):
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, SCALE)
    dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, SCALE, **kw)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _check(label, q, k, v, do, out, lse, dq, dk, dv, se=None, q_offset=0, dtype=None):
    ref = R.reference(q, k, v, do, out, se, q_offset, SCALE)
    return ref, R.check_all(ref, dtype or q.dtype, label, out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _packed(seqs, Hq, Hkv, dtype, order="backward", seed=0, **kw):
    plan, se = _trie(seqs, order)
    T = plan.T
    q, k, v, do = _dev(*_inputs(T, T, Hq, Hkv, dtype, seed, **kw))
    meta = ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv)
    res = _fwd_bwd(q, k, v, do, meta)
    _check(f"T={T} Hq={Hq}/{Hkv} {order}", q, k, v, do, *res, se=se)
    return plan, se, meta, (q, k, v, do), res


def _stack(start, B, Hq, Hkv, dtype, seed=0, **kw):
    q, k, v, do = _dev(*_inputs(B, start + B, Hq, Hkv, dtype, seed + start + B, q_offset=start, **kw))
    res = _fwd_bwd(q, k, v, do, ops.stack_meta(start))
    _check(f"stack start={start} B={B}", q, k, v, do, *res, q_offset=start)


def _chain(L):
    return [[7] + list(range(100, 100 + L - 1))] if L > 1 else [[7]]


def _prefix_trie(P):
    """Shared prefix of depth P and three branches: in one DFS order the branch ends land at 319 (63 mod 64, the last row of
    a query tile), 384 (a multiple of 128) and 449 (one past 448)."""
    pre = list(range(1000, 1000 + P))
    return [pre + [1] + [5] * (318 - P), pre + [2] + [6] * 64, pre + [3] + [8] * 64]


def _star(root, n):
    return [list(range(1000, 1000 + root)) + [c] for c in range(1, n + 1)]


# ------------------------------------------------------------------------------------------------ tile-edge geometries
CHAINS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 255, 256, 257, 1023, 1024, 1025]


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("L", CHAINS)
def test_chain_lengths_at_tile_edges(L, dtype):
    _packed(_chain(L), 2, 1, dtype, seed=L)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("P", [63, 64, 65, 127, 128, 129])
def test_prefix_forks_at_tile_edges(P, dtype):
    for order in ("forward", "backward"):
        plan, se, *_ = _packed(_prefix_trie(P), 4, 2, dtype, order, seed=P)
        assert plan.T == 449


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("root,n", [(1, 200), (60, 128), (64, 150)])
def test_root_with_one_token_children(root, n, dtype):
    """Every row of a tile has its own visibility set: the root path plus itself."""
    _packed(_star(root, n), 4, 2, dtype, seed=root + n)


STARTS = [0, 1, 62, 63, 64, 126, 127, 128, 129, 4095]
BS = [1, 63, 64, 65, 128, 129]


@pytest.mark.parametrize("start", STARTS)
def test_stack_form_offsets_at_tile_edges(start):
    """q_offset not tile-aligned: 62 and 126 put a dK/dV query tile at k0 + 126 (one short of the 'no mask needed' edge)."""
    for B in BS:
        _stack(start, B, 4, 2, BF)
    for B in (1, 64, 129):
        _stack(start, B, 4, 2, F16)


# ------------------------------------------------------------------------------------------------ head geometries
@pytest.mark.parametrize("hq,hkv,dtype", [(1, 1, BF), (2, 1, F16), (3, 1, BF), (8, 2, F16), (5, 1, BF), (10, 2, F16),
                                          (7, 1, BF), (8, 1, BF), (16, 2, F16), (40, 8, BF), (64, 8, BF), (40, 8, F16)])
def test_head_geometries(hq, hkv, dtype):
    _packed(_prefix_trie(65)[:2], hq, hkv, dtype, seed=hq * 10 + hkv)


# ------------------------------------------------------------------------------------------------ score dynamic range
@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("kw", [{"sigma": 4.0}, {"sigma": 16.0}, {"kind": "rising"}, {"kind": "rising", "beta": 0.5, "gamma": 4.0},
                                {"kind": "falling"}, {"kind": "falling", "sigma": 4.0}], ids=str)
def test_score_dynamic_range(kw, dtype):
    """Peaked rows, maxima rising in every key tile (the deferred-maximum rescale of O and lsum), maxima in the first tile with
    P underflowing to zero later — on a chain (causal) and on a forked trie."""
    _packed(_chain(1024), 2, 1, dtype, seed=3, **kw)
    _packed(_prefix_trie(128), 3, 1, dtype, "backward", seed=4, **kw)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("kind", ["randn", "rising"])
def test_long_rows_stack_form(kind, dtype):
    """64 queries over 16 384 keys."""
    _stack(16384 - 64, 64, 2, 1, dtype, kind=kind, gamma=64.0 if kind == "rising" else 8.0)


# ------------------------------------------------------------------------------------------------ forced dK/dV splits
def _split_meta(meta, Hkv, min_tiles):
    units, splits, n_slabs = packing.plan_dkv_units(meta.ktile_qend.cpu().numpy(), meta.T, meta.T, meta.q_offset, Hkv,
                                                    n_cu=1 << 20, min_tiles=min_tiles)
    return dataclasses.replace(meta, dkv_units=torch.from_numpy(units).to(DEV), n_slabs=n_slabs,
                               dkv_splits=torch.from_numpy(splits).to(DEV) if splits.shape[0] else None), splits


def _unsplit(meta):
    return dataclasses.replace(meta, dkv_units=None, dkv_splits=None, n_slabs=0)


def _close_rows(a, b, tol, label):
    """Row-wise |a - b| <= tol |b|: the same sums in another order (a few fp32 ulps, then at most one ulp of the output)."""
    a, b = a.double().cpu(), b.double().cpu()
    err, nb = (a - b).norm(dim=-1), b.norm(dim=-1)
    assert bool((err <= tol * nb + 1e-30).all()), f"{label}: split vs unsplit, worst {float((err / (nb + 1e-30)).max()):.3g}"


def test_forced_split_slab_counts_cover_every_residue():
    plan, se = _trie(_chain(1025))
    kq = ops.ktile_qend_from(se.to(torch.int32)).numpy()
    _, splits, _ = packing.plan_dkv_units(kq, plan.T, plan.T, 0, 2, n_cu=1 << 20, min_tiles=2)
    assert {int(n) % 4 for n in splits[:, 2]} == {0, 1, 2, 3}          # the finalize's 4-way loop and every tail length


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("min_tiles", [1, 2, 3])
@pytest.mark.parametrize("seqs", [_chain(1025), _prefix_trie(128)], ids=["chain1025", "prefix128"])
def test_forced_dkv_splits_and_accumulate(seqs, min_tiles, dtype):
    Hq, Hkv = 4, 2
    plan, se = _trie(seqs)
    T = plan.T
    q, k, v, do = _dev(*_inputs(T, T, Hq, Hkv, dtype, seed=min_tiles))
    base_meta = ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv)
    meta, splits = _split_meta(base_meta, Hkv, min_tiles)
    assert splits.shape[0] > 0
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, SCALE)
    ref = R.reference(q, k, v, do, out, se, 0, SCALE)
    g = torch.Generator().manual_seed(11)
    bk, bv = (torch.randn(T, Hkv, D, generator=g) for _ in range(2))
    for acc in (0, 1, 2):
        res = {}
        for name, m in (("split", meta), ("unsplit", _unsplit(base_meta))):
            if acc == 0:
                dk = dv = None
            elif acc == 1:
                dk, dv = bk.to(dtype).to(DEV), bv.to(dtype).to(DEV)
            else:
                dk, dv = bk.to(DEV), bv.to(DEV)
            base = None if acc == 0 else (dk.clone(), dv.clone())
            dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, m, SCALE, dk=dk, dv=dv, accumulate=acc)
            torch.cuda.synchronize()
            label = f"T={T} min_tiles={min_tiles} accumulate={acc} {name}"
            R.check("dq", dq, ref, dtype, label)
            R.check("dk", dk, ref, dtype, label, base=None if base is None else base[0])
            R.check("dv", dv, ref, dtype, label, base=None if base is None else base[1])
            res[name] = (dq, dk, dv)
        assert torch.equal(res["split"][0], res["unsplit"][0])         # dQ does not depend on the dK/dV units
        tol = 1e-5 if acc == 2 else 2 * R.U[dtype]
        for i, nm in ((1, "dk"), (2, "dv")):
            _close_rows(res["split"][i], res["unsplit"][i], tol, f"{nm} min_tiles={min_tiles} accumulate={acc}")


# ------------------------------------------------------------------------------------------------ API paths
@pytest.mark.parametrize("dtype", [BF, F16, F32])
def test_no_run_list_and_no_ktile_qend(dtype):
    """runs = NULL with a subtree bound (every key tile up to the row, masked) and ktile_qend = NULL (every query tile up
    to the end) on a packed trie: same per-row bound as the planned path."""
    Hq, Hkv = 4, 2
    plan, se = _trie(_prefix_trie(64), "forward")
    T = plan.T
    q, k, v, do = _dev(*_inputs(T, T, Hq, Hkv, dtype, seed=8))
    meta = _unsplit(ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv))
    planned = _fwd_bwd(q, k, v, do, meta)
    _check("planned", q, k, v, do, *planned, se=se)
    no_runs = dataclasses.replace(meta, run_ptr=None, runs=None)
    _check("runs=NULL", q, k, v, do, *_fwd_bwd(q, k, v, do, no_runs), se=se)
    no_kq = dataclasses.replace(meta, ktile_qend=None)
    out, lse = planned[0], planned[1]
    dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, no_kq, SCALE)
    torch.cuda.synchronize()
    _check("ktile_qend=NULL", q, k, v, do, out, lse, dq, dk, dv, se=se)


@pytest.mark.parametrize("dtype", [BF, F16])
def test_three_launch_backward_is_bit_identical(dtype):
    """bench.py's kernel timer runs the backward as which = 1, then 2|8, then 4 (finalize): the same bits as which = 3."""
    Hq, Hkv = 4, 2
    plan, se = _trie(_chain(1025))
    T = plan.T
    q, k, v, do = _dev(*_inputs(T, T, Hq, Hkv, dtype, seed=9))
    meta, splits = _split_meta(ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv), Hkv, 2)
    assert splits.shape[0] > 0
    out, lse, dq, dk, dv = _fwd_bwd(q, k, v, do, meta)
    ops.KernelTimer.active = tm = ops.KernelTimer()
    try:
        dq3, dk3, dv3 = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, SCALE)
    finally:
        ops.KernelTimer.active = None
    torch.cuda.synchronize()
    assert {n: c for n, (_, c) in tm.totals_ms().items()} == {"fwd": 0, "bwd_dq": 1, "bwd_dkv": 1, "bwd_dkv_finalize": 1}
    assert torch.equal(dq, dq3) and torch.equal(dk, dk3) and torch.equal(dv, dv3)
    _check("three-launch", q, k, v, do, out, lse, dq3, dk3, dv3, se=se)


@pytest.mark.parametrize("dtype", [BF, F16, F32])
def test_strided_fused_qkv_and_gradient_buffers(dtype):
    """q/k/v as head slices of one fused [T, Hq+2Hkv, 128] buffer and dQ/dK/dV written into the fused gradient buffer that
    _TreeAttention.backward uses, through the head-stride arguments: the same bits as contiguous operands."""
    Hq, Hkv = 6, 2
    plan, se = _trie(_prefix_trie(127))
    T = plan.T
    q, k, v, do = _dev(*_inputs(T, T, Hq, Hkv, dtype, seed=10))
    meta = ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv)
    ref_res = _fwd_bwd(q, k, v, do, meta)
    fused = torch.cat([q, k, v], dim=1)
    qs, ks, vs = fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
    out, lse, _, _ = ops.attn_fwd_raw(qs, ks, vs, meta, SCALE)
    g = torch.full((T, Hq + 2 * Hkv, D), float("nan"), dtype=dtype, device=DEV)
    dq, dk, dv = g[:, :Hq], g[:, Hq:Hq + Hkv], g[:, Hq + Hkv:]
    ops.attn_bwd_raw(qs, ks, vs, out, do, lse, meta, SCALE, dk=dk, dv=dv, dq=dq)
    torch.cuda.synchronize()
    for a, b in zip((out, lse, dq, dk, dv), ref_res):
        assert torch.equal(a, b)
    _check("fused", q, k, v, do, out, lse, dq, dk, dv, se=se)
    # through autograd: _TreeAttention.backward writes its own fused buffer
    qa, ka, va = (x.clone().requires_grad_(True) for x in (qs, ks, vs))
    o = ops.tree_attention(qa, ka, va, meta)
    o.backward(do)
    torch.cuda.synchronize()
    assert torch.equal(o.detach(), out) and torch.equal(qa.grad, dq) and torch.equal(ka.grad, dk) and torch.equal(va.grad, dv)


# ------------------------------------------------------------------------------------------------ fp32 kernels
@pytest.mark.parametrize("L", [1, 63, 64, 65, 127, 128, 129, 1025])
def test_fp32_chain_lengths_at_tile_edges(L):
    _packed(_chain(L), 2, 1, F32, seed=L)


@pytest.mark.parametrize("P", [63, 64, 65, 128])
def test_fp32_prefix_forks(P):
    _packed(_prefix_trie(P), 3, 1, F32, seed=P)


def test_fp32_stack_offsets():
    for start in (0, 1, 63, 64, 127, 4095):
        for B in (1, 63, 64, 65, 129):
            _stack(start, B, 4, 2, F32)


@pytest.mark.parametrize("kw", [{"sigma": 4.0}, {"sigma": 16.0}, {"kind": "rising"}, {"kind": "falling"}], ids=str)
def test_fp32_score_dynamic_range(kw):
    _packed(_chain(1024), 2, 1, F32, seed=3, **kw)
    _packed(_prefix_trie(128), 3, 1, F32, seed=4, **kw)
    _stack(16384 - 64, 64, 2, 1, F32, **kw)
