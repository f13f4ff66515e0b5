"""Tree attention at head_dim 64 (Qwen2 / Qwen2.5-0.5B geometry: 14 query / 2 kv heads) against the float64 reference of
tests/attn_ref64.py.  Its per-row bound is stated for any D (the dot-product length enters through the tensors' shape), with the
constants c calibrated at D = 128; the D = 64 kernels accumulate half as many products per dot, so the same c is the tighter
test.  The cases put chain ends, forks and stack offsets on the 64 / 128 tile edges, cover pairs, odd GQA groups and the
0.5B group of 7, all three dtypes, the stack form with accumulate 0/1/2, and forced dK/dV split units (bitwise reproducible,
in agreement with the unsplit sweep).  The D = 64 kernels use a 128-B-row LDS image with a swizzle of their own
(DESIGN.md §D = 64), so every read path of the image is exercised here."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import attn_ref64 as R
import hostmirror
from dynamictreeattn_amd import ops, packing, synth
from oracle import trie_oracle as to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64
SCALE = D ** -0.5
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _trie(seqs, order="backward"):
    t = to.TokenTrieOracle([np.array(s) for s in seqs])
    getattr(t, order + "_permute")()
    plan = packing.plan_segments(t.lens, t.lcp_lens)
    se = hostmirror.expand_plan_host(plan)[3]
    return plan, torch.from_numpy(se).long()


def _inputs(Tq, Tk, Hq, Hkv, dtype, seed=0, sigma=1.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Tq, Hq, D, generator=g) * sigma
    k, v = torch.randn(Tk, Hkv, D, generator=g), torch.randn(Tk, Hkv, D, generator=g)
    do = torch.randn(Tq, Hq, D, generator=g)
    return tuple(x.to(dtype).to(DEV) for x in (q, k, v, do))


def _fwd_bwd(q, k, v, do, meta, **kw):
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, SCALE)
    dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, SCALE, **kw)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _check(label, q, k, v, do, out, lse, dq, dk, dv, se=None, q_offset=0):
    ref = R.reference(q, k, v, do, out, se, q_offset, SCALE)
    return R.check_all(ref, q.dtype, label, out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _packed(seqs, Hq, Hkv, dtype, order="backward", seed=0, **kw):
    plan, se = _trie(seqs, order)
    q, k, v, do = _inputs(plan.T, plan.T, Hq, Hkv, dtype, seed, **kw)
    meta = ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv)
    res = _fwd_bwd(q, k, v, do, meta)
    _check(f"D=64 T={plan.T} Hq={Hq}/{Hkv} {order}", q, k, v, do, *res, se=se)
    return plan, se, meta, (q, k, v, do), res


def _chain(L):
    return [[7] + list(range(100, 100 + L - 1))] if L > 1 else [[7]]


def _prefix_trie(P):
    """Shared prefix of depth P and three branches ending at 319, 384 and 449 in one DFS order (as test_gpu_attention_edges.py)."""
    pre = list(range(1000, 1000 + P))
    return [pre + [1] + [5] * (318 - P), pre + [2] + [6] * 64, pre + [3] + [8] * 64]


# ------------------------------------------------------------------------------------------------ tile edges, dtypes, head geometries
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("L", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 1025])
def test_d64_chain_lengths_at_tile_edges(L, dtype):
    _packed(_chain(L), 2, 1, dtype, seed=L)


@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("P", [63, 64, 65, 127, 128, 129])
def test_d64_prefix_forks_at_tile_edges(P, dtype):
    for order in ("forward", "backward"):
        plan, *_ = _packed(_prefix_trie(P), 4, 2, dtype, order, seed=P)
        assert plan.T == 449


@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("hq,hkv", [(1, 1), (2, 1), (4, 2), (7, 1), (14, 2), (16, 8)])
def test_d64_head_geometries(hq, hkv, dtype):
    """Pairs of query heads share a workgroup, the odd head of a group runs alone: 7/1 and 14/2 take both launches."""
    _packed(_prefix_trie(65)[:2], hq, hkv, dtype, seed=hq * 10 + hkv)


@pytest.mark.parametrize("dtype", [BF, F16])
def test_d64_peaked_scores(dtype):
    """Large scores: the forward's deferred-maximum rescale and P underflow."""
    _packed(_chain(1024), 2, 1, dtype, seed=3, sigma=8.0)


# ------------------------------------------------------------------------------------------------ stack form, accumulate
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("start", [0, 1, 63, 64, 127, 128, 129, 4095])
def test_d64_stack_form_offsets_and_accumulate(start, dtype):
    """subtree_end = NULL at q_offset = start; dK/dV overwritten (0), added in the model dtype (1) and added into fp32 (2)."""
    Hq, Hkv = 14, 2
    for B in (1, 64, 65, 129):
        q, k, v, do = _inputs(B, start + B, Hq, Hkv, dtype, seed=start + B)
        meta = ops.stack_meta(start)
        out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, SCALE)
        ref = R.reference(q, k, v, do, out, None, start, SCALE)
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
            dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, SCALE, dk=dk, dv=dv, accumulate=acc)
            torch.cuda.synchronize()
            label = f"D=64 stack start={start} B={B} accumulate={acc}"
            if acc == 0:
                R.check_all(ref, dtype, label, out=out, lse=lse)
            R.check("dq", dq, ref, dtype, label)
            R.check("dk", dk, ref, dtype, label, base=None if base is None else base[0])
            R.check("dv", dv, ref, dtype, label, base=None if base is None else base[1])


# ------------------------------------------------------------------------------------------------ forced dK/dV splits
def _split_meta(meta, Hkv, min_tiles):
    units, splits, n_slabs = packing.plan_dkv_units(meta.ktile_qend.cpu().numpy(), meta.T, meta.T, meta.q_offset, Hkv,
                                                    n_cu=1 << 20, min_tiles=min_tiles)
    return dataclasses.replace(meta, dkv_units=torch.from_numpy(units).to(DEV), n_slabs=n_slabs,
                               dkv_splits=torch.from_numpy(splits).to(DEV) if splits.shape[0] else None), splits


def _unsplit(meta):
    return dataclasses.replace(meta, dkv_units=None, dkv_splits=None, n_slabs=0)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("min_tiles", [1, 2, 3])
@pytest.mark.parametrize("seqs", [_chain(1025), _prefix_trie(128)], ids=["chain1025", "prefix128"])
def test_d64_forced_dkv_splits(seqs, min_tiles, dtype):
    """The split sweep writes D-wide fp32 slabs that the finalize sums in a fixed order: two runs give the same bits, and the split
    result agrees with the unsplit one row by row (the same sums in another order)."""
    Hq, Hkv = 14, 2
    plan, se = _trie(seqs)
    T = plan.T
    q, k, v, do = _inputs(T, T, Hq, Hkv, dtype, seed=min_tiles)
    base_meta = ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv)
    meta, splits = _split_meta(base_meta, Hkv, min_tiles)
    assert splits.shape[0] > 0
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, SCALE)
    ref = R.reference(q, k, v, do, out, se, 0, SCALE)
    runs = [ops.attn_bwd_raw(q, k, v, out, do, lse, meta, SCALE) for _ in range(2)]
    unsplit = ops.attn_bwd_raw(q, k, v, out, do, lse, _unsplit(base_meta), SCALE)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "split dK/dV sweep is not bitwise reproducible"
    dq, dk, dv = runs[0]
    label = f"D=64 T={T} min_tiles={min_tiles} split"
    R.check("dq", dq, ref, dtype, label); R.check("dk", dk, ref, dtype, label); R.check("dv", dv, ref, dtype, label)
    assert torch.equal(dq, unsplit[0])
    for i, nm in ((1, "dk"), (2, "dv")):
        a, b = runs[0][i].double().cpu(), unsplit[i].double().cpu()
        err, nb = (a - b).norm(dim=-1), b.norm(dim=-1)
        assert bool((err <= 2 * R.U[dtype] * nb + 1e-30).all()), f"{nm}: split vs unsplit, worst {float((err / (nb + 1e-30)).max()):.3g}"


# ------------------------------------------------------------------------------------------------ C interface
def test_d64_c_interface_codes():
    from dynamictreeattn_amd._lib import lib
    P = lambda t: t.data_ptr()
    Hq, Hkv = 2, 1
    for hd, want in ((64, 0), (128, 0), (32, -2), (96, -2), (256, -2)):
        q = torch.zeros(4, Hq, hd, dtype=BF, device=DEV); kv = torch.zeros(4, Hkv, hd, dtype=BF, device=DEV)
        o = torch.empty_like(q); lse = torch.zeros(Hq, 4, device=DEV)
        st = lib().dta_tree_attn_fwd(P(q), P(kv), P(kv), P(o), P(lse), None, None, None, 4, 4, 0, Hq, Hkv, hd,
                                     Hq * hd, hd, Hkv * hd, hd, Hkv * hd, hd, Hq * hd, hd, 0.1, 0, None, 0, 0.0, None)
        torch.cuda.synchronize()
        assert st == want, (hd, st)
        dl = torch.zeros(Hq, 4, device=DEV); dq = torch.empty_like(q); dk = torch.empty_like(kv); dv = torch.empty_like(kv)
        st = lib().dta_tree_attn_bwd(P(q), P(kv), P(kv), P(o), P(o), P(lse), P(dl), P(dq), P(dk), P(dv), None, None, None, None,
                                     4, 4, 0, Hq, Hkv, hd, Hq * hd, hd, Hkv * hd, hd, Hkv * hd, hd, Hq * hd, hd, Hq * hd, hd,
                                     Hkv * hd, hd, 0.1, 0, 0, 3, None, 0, None, 0, None, None, 0, 0.0, None)
        torch.cuda.synchronize()
        assert st == want, ("bwd", hd, st)


# ------------------------------------------------------------------------------------------------ full size
def test_d64_full_size_properties_tau2():
    """The tau2 trie (T = 25 482 packed tokens) at Qwen2.5-0.5B head geometry (14 / 2, D = 64), attention only: rows of one leaf
    path equal a dense causal run over that path; linearity in V (as test_gpu_attention.test_full_size_properties_tau2)."""
    plan, se = _trie(synth.tau2(0))
    T = plan.T
    assert T == 25482
    Hq, Hkv = synth.QWEN25_0P5B["num_attention_heads"], synth.QWEN25_0P5B["num_key_value_heads"]
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(T, H, D, generator=g).bfloat16().to(DEV) for H in (Hq, Hkv, Hkv))
    meta = ops.meta_from_plan(plan, se.to(DEV, torch.int32), DEV, Hkv)
    rel = lambda a, b: float((a.float().cpu() - b).norm() / b.norm())
    o, _, _, _ = ops.attn_fwd_raw(q, k, v, meta, SCALE)
    o2, _, _, _ = ops.attn_fwd_raw(q, k, (2 * v.float()).bfloat16(), meta, SCALE)
    assert rel(o2, 2 * o.float().cpu()) < 4e-3
    leaf = plan.M - 1
    idx = np.concatenate([np.arange(b, e) for b, e in plan.path_runs[leaf]] + [np.arange(plan.seg_off[leaf], plan.seg_off[leaf + 1])])
    idx_d = torch.from_numpy(idx).to(DEV)
    od, _, _, _ = ops.attn_fwd_raw(q[idx_d].contiguous(), k[idx_d].contiguous(), v[idx_d].contiguous(), ops.stack_meta(0), SCALE)
    assert rel(o[idx_d], od.float().cpu()) < 4e-3
    assert math.isfinite(float(o.float().abs().max()))
