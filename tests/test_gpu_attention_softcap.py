"""Soft-capped tree attention (dta_tree_attn_fwd / _bwd with softcap > 0) against the float64 reference of tests/softcap_ref64.py with the
per-row error bound of tests/attn_ref64.py (check_all and its constants C, unchanged; the limit is err / bound <= 1).  Scores are
c tanh(scale q.k / c), capped before the visibility mask.  Cases: packed tries whose chain ends and forks sit on the 64 / 128 tile edges
(the generators of the window tests), the stack form with a non-zero q_offset and 1 .. 200 query rows, D = 64 and 128, (4, 2),
(2, 1) and (3, 1) heads (head pairs; one pair plus the odd head of the one-head launch), bf16 / f16 / fp32, the cap alone and with a
window whose edge lies inside a tile; a saturated case (|z| / c about 8);
softcap <= 0 must give the bits of the uncapped run; forced dK/dV splits must be bitwise reproducible; accumulate 1 and 2.

Condition on the inputs: in every counted case the float64 references WITH and WITHOUT the cap differ, for every tensor, by at least
10 x the bound on some row (softcap_ref64.assert_cap_matters, from the references alone) - otherwise an uncapped kernel would pass.
With unit-normal q, k at scale D^-1/2 the cap is 2.0.  The one-row packed trie (a row that sees only itself: out = v and dQ = 0 with
or without a cap) cannot meet it and is run as an extra, uncounted check.

Largest err / bound observed on the MI355X over this module (constants c of attn_ref64.C; the dQ row was taken with the cap applied in
a separate pass over the scores - the same arithmetic per element as the present in-loop form):

    tensor   largest ratio bf16 / f16 / fp32
    out      0.28 / 0.29 / 0.06
    lse      0.03 / 0.03 / 0.03
    dQ       0.18 / 0.17 / 0.04
    dK       0.39 / 0.36 / 0.01
    dV       0.37 / 0.43 / 0.02
"""
import dataclasses

import pytest
import torch

import attn_ref64 as R
import softcap_ref64 as SR
import test_gpu_attention_window as W
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CAP = 2.0
HEADS = [(4, 2), (2, 1), (3, 1)]
ROWS = [1, 63, 64, 65, 129, 200]


def _run(q, k, v, do, meta, scale, softcap, **kw):
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, scale, softcap)
    dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale, softcap=softcap, **kw)
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _check(label, q, k, v, do, vis, res, scale, softcap, dtype, counted=True):
    out, lse, dq, dk, dv = res
    ref = SR.reference_cap(q, k, v, vis, do, out, scale, softcap)
    if counted:
        SR.assert_cap_matters(SR.reference_cap(q, k, v, vis, do, None, scale, softcap), SR.reference_cap(q, k, v, vis, do, None, scale, 0.0),
                              dtype, label)
    for t in res:
        assert bool(torch.isfinite(t.float()).all()), label
    return R.check_all(ref, dtype, label, out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _packed(seqs, Wn, hq, hkv, D, dtype, softcap=CAP, seed=0, sigma=1.0, counted=True, order="backward"):
    """A packed trie; Wn > 0: with that window (the windowed plan), else the full meta."""
    plan = W._trie(seqs, order)
    full, win, depth, se, _ = W._metas(plan, Wn if Wn > 0 else 1 << 20, hkv)
    meta = win if Wn > 0 else full
    q, k, v, do = W._inputs(plan.T, plan.T, hq, hkv, D, dtype, seed)
    if sigma != 1.0:
        q = (q.float() * sigma).to(dtype)
    scale = D ** -0.5
    res = _run(q, k, v, do, meta, scale, softcap)
    vis = W._vis_packed(depth, se, Wn if Wn > 0 else 1 << 20)
    return _check(f"cap {softcap} W={Wn} T={plan.T} D={D} {hq}/{hkv} {order}", q, k, v, do, vis, res, scale, softcap, dtype, counted), \
        (plan, meta, (q, k, v, do), res)


# ------------------------------------------------------------------------------------------------ packed tries at the tile edges
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_cap_packed_chains_and_forks(hq, hkv, D, dtype):
    for T in ROWS[1:]:
        _packed(W._chain(T), 0, hq, hkv, D, dtype, seed=T)
        _packed(W._chain(T), 40, hq, hkv, D, dtype, seed=T + 1)                 # the window's edge inside a 64-key tile
    _packed(W._chain(1), 0, hq, hkv, D, dtype, counted=False)                   # a row that sees only itself: not counted (see above)
    for P in (64, 128):
        for order in ("forward", "backward"):
            _packed(W._prefix_trie(P), 0, hq, hkv, D, dtype, seed=P, order=order)
    _packed(W._prefix_trie(65), 100, hq, hkv, D, dtype, seed=3)


# ------------------------------------------------------------------------------------------------ stack form, offsets, accumulate
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("hq,hkv", HEADS)
def test_cap_stack_form_offsets_and_accumulate(hq, hkv, D, dtype):
    scale = D ** -0.5
    for B, start, Wn in [(1, 70, 0), (63, 1, 0), (64, 64, 0), (65, 63, 40), (129, 130, 0), (200, 57, 100)]:
        q, k, v, do = W._inputs(B, start + B, hq, hkv, D, dtype, seed=start + B)
        meta = ops.stack_meta(start, Wn)
        out, lse, _, _ = ops.attn_fwd_raw(q, k, v, meta, scale, CAP)
        qi, kj = start + torch.arange(B)[:, None], torch.arange(start + B)[None, :]
        vis = (kj <= qi) & ((qi - kj < Wn) if Wn > 0 else torch.ones_like(kj <= qi))
        ref = SR.reference_cap(q, k, v, vis, do, out, scale, CAP)
        label = f"cap stack start={start} B={B} W={Wn} D={D} {hq}/{hkv}"
        SR.assert_cap_matters(SR.reference_cap(q, k, v, vis, do, None, scale, CAP), SR.reference_cap(q, k, v, vis, do, None, scale, 0.0), dtype, label)
        g = torch.Generator().manual_seed(start + 7 * B)
        bk, bv = (torch.randn(start + B, hkv, D, generator=g) for _ in range(2))
        for acc in (0, 1, 2):
            if acc == 0:
                dk = dv = None
            elif acc == 1:
                dk, dv = bk.to(dtype).to(DEV), bv.to(dtype).to(DEV)
            else:
                dk, dv = bk.to(DEV), bv.to(DEV)
            base = None if acc == 0 else (dk.clone(), dv.clone())
            dq, dk, dv = ops.attn_bwd_raw(q, k, v, out, do, lse, meta, scale, dk=dk, dv=dv, accumulate=acc, softcap=CAP)
            torch.cuda.synchronize()
            if acc == 0:
                R.check_all(ref, dtype, label, out=out, lse=lse)
            R.check("dq", dq, ref, dtype, f"{label} accumulate={acc}")
            R.check("dk", dk, ref, dtype, f"{label} accumulate={acc}", base=None if base is None else base[0])
            R.check("dv", dv, ref, dtype, f"{label} accumulate={acc}", base=None if base is None else base[1])


# ------------------------------------------------------------------------------------------------ saturation
@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
def test_cap_saturated_scores_stay_finite(D, dtype):
    """q scaled by 4: z ~ N(0, 4), so |z| / c reaches about 8 (tanh = +-1 to fp32 precision well before that)."""
    plan = W._trie(W._prefix_trie(128))
    q, k, _, _ = W._inputs(plan.T, plan.T, 4, 2, D, dtype, seed=11)
    z = torch.einsum("ihd,jhd->hij", q.double().cpu() * 4.0, k.double().cpu().repeat_interleave(2, dim=1)) * D ** -0.5
    assert 7.0 <= float(z.abs().max()) / CAP <= 12.0
    _packed(W._prefix_trie(128), 0, 4, 2, D, dtype, seed=11, sigma=4.0)
    _packed(W._prefix_trie(128), 70, 4, 2, D, dtype, seed=11, sigma=4.0)


# ------------------------------------------------------------------------------------------------ softcap <= 0: the uncapped run, bit for bit
def _cap_entry(q, k, v, do, meta, scale, softcap, accumulate=0):
    """dta_tree_attn_fwd / _bwd called directly (ops refuses a negative cap; the entries take it as no cap)."""
    Tq, Hq, D = q.shape
    Tk, Hkv, _ = k.shape
    out = torch.empty_like(q); lse = torch.empty(Hq, Tq, dtype=F32, device=DEV); delta = torch.empty_like(lse)
    dq = torch.empty_like(q); dk = torch.zeros_like(k); dv = torch.zeros_like(v)
    st = lambda t: (t.stride(0), t.stride(1))
    win = (ptr(meta.win_lo), int(meta.window)) if meta.window > 0 else (None, 0)
    units, splits = meta.dkv_units, meta.dkv_splits
    if q.dtype == F32:
        units = splits = None
    nu, ns = (0 if units is None else units.shape[0]), (0 if splits is None else splits.shape[0])
    ws = torch.empty((meta.n_slabs, Hkv, 2, packing.KTILE, D), dtype=F32, device=DEV) if (units is not None and meta.n_slabs) else None
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib().dta_tree_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(meta.subtree_end), ptr(meta.run_ptr), ptr(meta.runs),
                                 Tq, Tk, meta.q_offset, Hq, Hkv, D, *st(q), *st(k), *st(v), *st(out), scale, ops._DT[q.dtype], *win, softcap, stream)
    assert rc == 0, rc
    rc = lib().dta_tree_attn_bwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
                                 ptr(meta.subtree_end), ptr(meta.run_ptr), ptr(meta.runs), ptr(meta.ktile_qend),
                                 Tq, Tk, meta.q_offset, Hq, Hkv, D, *st(q), *st(k), *st(v), *st(out), *st(dq), *st(dk), scale, ops._DT[q.dtype],
                                 accumulate, 3, ptr(units), nu, ptr(splits) if ns else None, ns, ptr(ws), *win, softcap, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
def test_softcap_zero_is_the_win_entry_bitwise(D, dtype):
    plan = W._trie(W._prefix_trie(128))
    full, win, *_ = W._metas(plan, 70, 2)
    q, k, v, do = W._inputs(plan.T, plan.T, 4, 2, D, dtype, seed=5)
    scale = D ** -0.5
    for meta in (full, win):
        for cap in (0.0, -1.0):
            for a, b in zip(_run(q, k, v, do, meta, scale, 0.0), _cap_entry(q, k, v, do, meta, scale, cap)):
                assert torch.equal(a, b)
        for a, b in zip(_run(q, k, v, do, meta, scale, CAP), _cap_entry(q, k, v, do, meta, scale, CAP)):       # and ops reaches the same entry
            assert torch.equal(a, b)
    qs, ks, vs, ds = W._inputs(65, 65 + 63, 4, 2, D, dtype, seed=6)
    for meta in (ops.stack_meta(63), ops.stack_meta(63, 40)):
        for a, b in zip(_run(qs, ks, vs, ds, meta, scale, 0.0), _cap_entry(qs, ks, vs, ds, meta, scale, 0.0)):
            assert torch.equal(a, b)
    # a NaN or infinite cap is refused
    for bad in (float("nan"), float("inf")):
        out = torch.empty_like(q); lse = torch.empty(4, plan.T, dtype=F32, device=DEV)
        st = lambda t: (t.stride(0), t.stride(1))
        assert lib().dta_tree_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(full.subtree_end), ptr(full.run_ptr), ptr(full.runs),
                                       plan.T, plan.T, 0, 4, 2, D, *st(q), *st(k), *st(v), *st(out), scale, ops._DT[dtype], None, 0, bad, None) == -1


# ------------------------------------------------------------------------------------------------ forced dK/dV splits
@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Wn", [0, 300])
def test_cap_forced_dkv_splits_are_bitwise_reproducible(Wn, D, dtype):
    hq, hkv = 4, 2
    plan = W._trie(W._chain(1025))
    full, win, depth, se, _ = W._metas(plan, Wn if Wn > 0 else 1 << 20, hkv)
    meta = win if Wn > 0 else full
    units, splits, n_slabs = packing.plan_dkv_units(meta.ktile_qend.cpu().numpy(), plan.T, plan.T, 0, hkv, n_cu=1 << 20, min_tiles=1)
    assert splits.shape[0] > 0
    split = dataclasses.replace(meta, dkv_units=torch.from_numpy(units).to(DEV), dkv_splits=torch.from_numpy(splits).to(DEV), n_slabs=n_slabs)
    unsplit = dataclasses.replace(meta, dkv_units=None, dkv_splits=None, n_slabs=0)
    q, k, v, do = W._inputs(plan.T, plan.T, hq, hkv, D, dtype, seed=Wn + 1)
    scale = D ** -0.5
    out, lse, _, _ = ops.attn_fwd_raw(q, k, v, split, scale, CAP)
    runs = [ops.attn_bwd_raw(q, k, v, out, do, lse, split, scale, softcap=CAP) for _ in range(2)]
    one = ops.attn_bwd_raw(q, k, v, out, do, lse, unsplit, scale, softcap=CAP)
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "split capped dK/dV sweep is not bitwise reproducible"
    vis = W._vis_packed(depth, se, Wn if Wn > 0 else 1 << 20)
    ref = SR.reference_cap(q, k, v, vis, do, out, scale, CAP)
    R.check_all(ref, dtype, f"cap split W={Wn} D={D}", dq=runs[0][0], dk=runs[0][1], dv=runs[0][2])
    assert torch.equal(runs[0][0], one[0])
    for i in (1, 2):
        a, b = runs[0][i].double().cpu(), one[i].double().cpu()
        assert bool(((a - b).norm(dim=-1) <= 2 * R.U[dtype] * b.norm(dim=-1) + 1e-30).all())


# ------------------------------------------------------------------------------------------------ autograd operators and the tape
@pytest.mark.parametrize("dtype", [BF, F32])
def test_tree_attention_autograd_and_replay_carry_the_cap(dtype):
    """ops.tree_attention(softcap=...) through autograd equals the raw calls; an AttentionTape replay (the forward kernel skipped)
    still runs the CAPPED backward, and a replay under another cap is refused."""
    D, hq, hkv = 64, 4, 2
    plan = W._trie(W._prefix_trie(64))
    full, *_ = W._metas(plan, 1 << 20, hkv)
    q, k, v, do = W._inputs(plan.T, plan.T, hq, hkv, D, dtype, seed=2)
    want = _run(q, k, v, do, full, D ** -0.5, CAP)
    plain = _run(q, k, v, do, full, D ** -0.5, 0.0)
    assert not torch.equal(want[2], plain[2])
    items = []
    with torch.no_grad(), ops.AttentionTape("record", items):
        o0 = ops.tree_attention(q, k, v, full, softcap=CAP)
    assert torch.equal(o0, want[0]) and len(items) == 1
    for tape in (None, ops.AttentionTape("replay", items)):
        qa, ka, va = (x.clone().requires_grad_(True) for x in (q, k, v))
        if tape is None:
            o = ops.tree_attention(qa, ka, va, full, softcap=CAP)
        else:
            with tape:
                o = ops.tree_attention(qa, ka, va, full, softcap=CAP)
            assert tape.pos == 1
        o.backward(do)
        for a, b in zip((o, qa.grad, ka.grad, va.grad), (want[0], want[2], want[3], want[4])):
            assert torch.equal(a.detach(), b)
    with pytest.raises(RuntimeError, match="softcap"), ops.AttentionTape("replay", items):
        ops.tree_attention(q, k, v, full, softcap=1.0)
    with pytest.raises(ValueError, match="softcap"):
        ops.tree_attention(q, k, v, full, softcap=-2.0)
