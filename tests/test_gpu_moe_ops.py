"""Mixture-of-experts kernels (dta_moe_*) against the float64 restatement of tests/moe_ref64.py: router forward / backward (with exact
ties), the permutation (empty experts, one expert taking every pair, bitwise repeatability), the grouped GEMMs in bf16 / f16 / fp32 with
per-expert row counts around the tile edges, the combine, and the argument checks of the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

import moe_ref64 as R
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BM = 128


def _within(out, ref, bnd, what):
    err = (out.double().cpu() - ref).abs()
    bad = err > bnd
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements out of bound, worst err/bound {float((err / bnd).max()):.3g}"


@pytest.mark.parametrize("E,k", R.ROUTER_CASES)
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_router_forward_backward(E, k, norm, dtype):
    logits, g = R.router_logits(E, k, dtype)
    T = R.ROUTER_T
    ids, w, lse = ops.moe_router_fwd_raw(logits.to(DEV), k, norm)
    rid, rw, rlse, p, margin = R.router_ref(logits, k, norm)
    ok = margin > R.MARGIN                    # rows whose top-k a fp32 rounding cannot reorder
    assert int(ok.sum()) >= R.MARGIN_SHARE * T          # tests/test_moe_ref64.py checks this share of every case on the CPU
    assert torch.equal(ids.cpu().long()[ok], rid[ok])
    _within(w.float()[ok.to(DEV)], rw[ok], R.U[dtype] * rw[ok].abs() + 1e-6, "weights")
    _within(lse, rlse, 1e-5 * (1 + rlse.abs()), "lse")
    dw = torch.randn(T, k, generator=g).to(dtype)
    dl = ops.moe_router_bwd_raw(logits.to(DEV), lse, ids, dw.to(DEV), norm)
    ref, scale = R.router_bwd_ref(logits, ids.cpu(), dw, norm)
    _within(dl, ref, R.U[dtype] * ref.abs() + 1e-5 * scale + 1e-7 * float(ref.abs().max()), "dlogits")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_router_ties_lower_expert_index_wins(dtype):
    E, k = 60, 8
    logits = torch.zeros(4, E)
    logits[1, [7, 3, 50, 20]] = 1.0                       # four equal maxima, the rest tie below them
    logits[2, ::3] = 0.5
    logits[3] = torch.arange(E) % 5                       # groups of 12 equal values
    ids, w, _ = ops.moe_router_fwd_raw(logits.to(dtype).to(DEV), k, True)
    ids = ids.cpu().tolist()
    assert ids[0] == list(range(8))
    assert ids[1] == [3, 7, 20, 50, 0, 1, 2, 4]
    assert ids[2] == [0, 3, 6, 9, 12, 15, 18, 21]
    assert ids[3] == [4, 9, 14, 19, 24, 29, 34, 39]
    assert torch.allclose(w.float().cpu()[0], torch.full((8,), 1 / 8))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_router_ties_across_the_slots_of_one_lane(dtype):
    """E 200: lane 5 holds experts 5, 69, 133, 197 in its four slots, lanes 4 and 6 their neighbours.  Equal maxima must come out in
    ascending expert index whether the tie is between slots of one lane, between lanes, or both; 200 equal logits give 0..7."""
    E, k = 200, 8
    logits = torch.zeros(4, E)
    logits[0, [197, 133, 69, 5]] = 1.0                    # one lane's four slots; the rest tie below them
    logits[1, [197, 133, 69, 5, 4, 6, 68, 70]] = 1.0      # ... and two slots of each neighbouring lane: exactly k equal maxima
    logits[2, [5, 69]], logits[2, [133, 197]], logits[2, [4, 132]] = 2.0, 1.0, 1.0    # two tie groups in descending value
    logits[3] = 0.75                                      # every expert ties
    ids, w, _ = ops.moe_router_fwd_raw(logits.to(dtype).to(DEV), k, True)
    ids, w = ids.cpu().tolist(), w.double().cpu()
    assert ids[0] == [5, 69, 133, 197, 0, 1, 2, 3]
    assert ids[1] == [4, 5, 6, 68, 69, 70, 133, 197]
    assert ids[2] == [5, 69, 4, 132, 133, 197, 0, 1]
    assert ids[3] == list(range(8))
    eighth = torch.full((8,), 1 / 8, dtype=torch.float64)
    for row in (1, 3):                                    # eight equal probabilities renormalise to 1/8 each
        assert bool(((w[row] - eighth).abs() <= R.U[dtype] / 8 + 1e-6).all()), (row, w[row])


def _route(ids, E):
    r = ops.moe_permute(ids.to(DEV).int(), E)
    return r


@pytest.mark.parametrize("case", ["random", "empty_experts", "one_expert", "big", "P1", "P255", "P256", "P257", "T0", "dropped"])
def test_permutation(case):
    """P1 .. P257: P = T * k on either side of the 256-pair chunk of the counting sort.  T0: no pair at all.  dropped: every seventh id
    outside [0, E) - such a pair takes no row, row_of_pair is -1, and src_token is defined below offsets[E] only."""
    g = torch.Generator().manual_seed(3)
    if case in ("P1", "P255", "P256", "P257", "T0"):
        T, k, E = {"P1": (1, 1, 8), "P255": (85, 3, 8), "P256": (128, 2, 8), "P257": (257, 1, 8), "T0": (0, 2, 8)}[case]
        ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]) if T else torch.empty((0, k), dtype=torch.long)
    elif case == "dropped":
        T, k, E = 300, 2, 60
        ids = R.dropped_ids(T, k, E)
    elif case == "random":
        T, k, E = 517, 2, 8
        ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    elif case == "empty_experts":
        T, k, E = 300, 2, 60
        ids = torch.stack([torch.tensor([5, 40]) if i % 3 else torch.tensor([40, 59]) for i in range(T)])
    elif case == "one_expert":
        T, k, E = 700, 1, 128
        ids = torch.full((T, k), 77)
    else:
        T, k, E = 4099, 8, 128
        ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    a, b = _route(ids, E), _route(ids, E)
    offs, rop, src = R.permute_ref(ids, E)
    n_valid = int(offs[E])                                         # src_token is written below offsets[E] only
    assert n_valid == T * k or case == "dropped"
    for x, y in ((a.expert_offsets, b.expert_offsets), (a.row_of_pair, b.row_of_pair), (a.src_token[:n_valid], b.src_token[:n_valid]), (a.tiles, b.tiles)):
        assert torch.equal(x, y)                                   # bitwise repeatable
    assert a.expert_offsets.cpu().tolist() == offs.tolist()
    assert a.row_of_pair.cpu().numpy().tolist() == rop.tolist()
    assert a.src_token.shape == (T * k,) and a.src_token.cpu().numpy()[:n_valid].tolist() == src[:n_valid].tolist()
    tiles = a.tiles.cpu().view(-1, 2)
    assert tiles.shape[0] == -(-T * k // BM) + E
    want = [(e, int(o)) for e in range(E) for o in range(offs[e], offs[e + 1], BM)]
    assert [tuple(t) for t in tiles[:len(want)].tolist()] == want
    assert bool((tiles[len(want):, 0] == -1).all()) and bool((tiles[len(want):, 1] == 0).all())
    if case == "T0":
        assert offs.tolist() == [0] * (E + 1) and not want
    if case == "dropped":
        flat = ids.reshape(-1)
        out_of_range = (flat < 0) | (flat >= E)
        assert int(out_of_range.sum()) == T * k - n_valid > 0 and bool((a.row_of_pair.cpu()[out_of_range] == -1).all())


COUNTS = [0, 1, BM - 1, BM, BM + 1, 0, 2 * BM + 3, 5]


def _gemm_case(E, counts, H, N, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    counts = (counts * (E // len(counts) + 1))[:E]
    ids = torch.cat([torch.full((c,), e) for e, c in enumerate(counts)])
    ids = ids[torch.randperm(len(ids), generator=g)][:, None]               # k = 1: T = sum(counts)
    T = ids.shape[0]
    route = _route(ids, E)
    offs, rop, src = R.permute_ref(ids, E)
    x = torch.randn(T, H, generator=g).to(dtype)
    w = (torch.randn(E, N, H, generator=g) / H ** 0.5).to(dtype)
    dy = torch.randn(T, N, generator=g).to(dtype)
    return route, offs, src, x, w, dy


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("shape", [(8, 32, 96), (8, 48, 32), (5, 2048, 1536), (4, 768, 2048), (3, 208, 144), (3, 144, 208)])
def test_grouped_gemm_fwd_dgrad_wgrad(dtype, shape):
    """The last two shapes put a partial tile behind a full one in every role: 144 = 128 + 16 (a second n-tile of the MFMA path with
    masked columns, a third 64-tile of the fp32 path) = 2 * 64 + 16 and 208 = 3 * 64 + 16 (a k-tail behind full k-steps).  Without the
    gather (k = 1: P = T) x stands for an expert-sorted [P, H] operand: the down projection's forward and weight gradient."""
    E, H, N = shape
    route, offs, src, x, w, dy = _gemm_case(E, COUNTS, H, N, dtype, seed=H + N)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    for mode, args, gather in ((ops.MOE_FWD, dict(x=xd, w=wd), True), (ops.MOE_FWD, dict(x=xd, w=wd), False),
                               (ops.MOE_DGRAD, dict(w=wd, dy=dyd), False), (ops.MOE_WGRAD, dict(x=xd, dy=dyd), True),
                               (ops.MOE_WGRAD, dict(x=xd, dy=dyd), False)):
        out = ops.moe_grouped_gemm(mode, route, w.shape, dtype, gather=gather, **args)
        ref, mag, n = R.gemm_ref(mode, x, w, dy, offs, src, gather)
        _within(out, ref, R.bound(ref, mag, n, dtype), f"mode {mode} gather {gather}")
        if mode == ops.MOE_WGRAD:
            empty = [e for e in range(E) if offs[e + 1] == offs[e]]
            assert empty and all(bool((out[e] == 0).all()) for e in empty)          # empty experts: zero gradient


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grouped_gemm_qwen3_30b_a3b_geometry(dtype):
    """H 2048, I 768, E 128, k 8 on routed tokens: gate/up forward (gathered), down dgrad and the gate/up wgrad."""
    E, k, H, I, T = 128, 8, 2048, 768, 384
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(T, E, generator=g).to(dtype).to(DEV)
    ids, _, _ = ops.moe_router_fwd_raw(logits, k, True)
    route = ops.moe_permute(ids, E)
    offs, rop, src = R.permute_ref(ids.cpu(), E)
    x = torch.randn(T, H, generator=g).to(dtype)
    wgu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(dtype)
    wdn = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(dtype)
    dy = torch.randn(T * k, H, generator=g).to(dtype)
    dgu = torch.randn(T * k, 2 * I, generator=g).to(dtype)
    out = ops.moe_grouped_gemm(ops.MOE_FWD, route, wgu.shape, dtype, x=x.to(DEV), w=wgu.to(DEV), gather=True)
    ref, mag, n = R.gemm_ref(0, x, wgu, None, offs, src, True)
    _within(out, ref, R.bound(ref, mag, n, dtype), "gate/up fwd")
    out = ops.moe_grouped_gemm(ops.MOE_DGRAD, route, wdn.shape, dtype, w=wdn.to(DEV), dy=dy.to(DEV))
    ref, mag, n = R.gemm_ref(1, None, wdn, dy, offs, src, False)
    _within(out, ref, R.bound(ref, mag, n, dtype), "down dgrad")
    out = ops.moe_grouped_gemm(ops.MOE_WGRAD, route, wgu.shape, dtype, x=x.to(DEV), dy=dgu.to(DEV), gather=True)
    ref, mag, n = R.gemm_ref(2, x, None, dgu, offs, src, True)
    _within(out, ref, R.bound(ref, mag, n, dtype), "gate/up wgrad")


DROPPED = (300, 2, 60)          # T, k, E of the routing with ids outside [0, E) (R.dropped_ids)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_grouped_gemm_dropped_routing(dtype):
    """Ids outside [0, E): the P - offsets[E] dropped pairs own no row.  Every mode meets its bound on the rows below offsets[E] (the
    rows behind them belong to no tile and are left unwritten), and the weight gradient sums an expert's own rows only."""
    T, k, E = DROPPED
    H, N = 144, 80
    ids = R.dropped_ids(T, k, E)
    route = _route(ids, E)
    offs, rop, src = R.permute_ref(ids, E)
    nv, P = int(offs[E]), T * k
    assert 0 < nv < P and route.expert_offsets.cpu().tolist() == offs.tolist()
    g = torch.Generator().manual_seed(H + N)
    x, xs = torch.randn(T, H, generator=g).to(dtype), torch.randn(P, H, generator=g).to(dtype)
    w = (torch.randn(E, N, H, generator=g) / H ** 0.5).to(dtype)
    dy = torch.randn(P, N, generator=g).to(dtype)
    xd, xsd, wd, dyd = x.to(DEV), xs.to(DEV), w.to(DEV), dy.to(DEV)
    for mode, args, gather in ((ops.MOE_FWD, dict(x=xd, w=wd), True), (ops.MOE_FWD, dict(x=xsd, w=wd), False),
                               (ops.MOE_DGRAD, dict(w=wd, dy=dyd), False), (ops.MOE_WGRAD, dict(x=xd, dy=dyd), True),
                               (ops.MOE_WGRAD, dict(x=xsd, dy=dyd), False)):
        out = ops.moe_grouped_gemm(mode, route, w.shape, dtype, gather=gather, **args)
        ref, mag, n = R.gemm_ref(mode, x if gather else xs, w, dy, offs, src, gather)
        if mode != ops.MOE_WGRAD:
            assert out.shape[0] == P
            out, ref, mag = out[:nv], ref[:nv], mag[:nv]
        _within(out, ref, R.bound(ref, mag, n, dtype), f"dropped routing: mode {mode} gather {gather}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_empty_batch(dtype, monkeypatch):
    """T = 0 through every wrapper: the entries return before launching, the weight gradient of no rows is all zeros, and the forward
    and dgrad wrappers hand back an empty [0, .] tensor without a call into the library."""
    E, k, H, N = 8, 2, 48, 32
    logits = torch.empty((0, E), dtype=dtype, device=DEV)
    ids, w, lse = ops.moe_router_fwd_raw(logits, k, True)
    assert ids.shape == (0, k) and w.shape == (0, k) and w.dtype == dtype and lse.shape == (0,)
    assert ops.moe_router_bwd_raw(logits, lse, ids, w, True).shape == (0, E)
    route = ops.moe_permute(ids, E)
    assert route.expert_offsets.cpu().tolist() == [0] * (E + 1) and route.row_of_pair.shape == (0,) and route.src_token.shape == (0,)
    x, wt, dy = torch.empty((0, H), dtype=dtype, device=DEV), torch.ones((E, N, H), dtype=dtype, device=DEV), torch.empty((0, N), dtype=dtype, device=DEV)
    for gather in (True, False):
        dw = ops.moe_grouped_gemm(ops.MOE_WGRAD, route, wt.shape, dtype, x=x, dy=dy, gather=gather)
        assert dw.shape == wt.shape and dw.dtype == dtype and bool((dw == 0).all())
    y = torch.empty((0, H), dtype=dtype, device=DEV)
    assert ops.moe_combine_fwd_raw(y, w, route).shape == (0, H)
    dyc, dwc = ops.moe_combine_bwd_raw(y, y, w, route)
    assert dyc.shape == (0, H) and dwc.shape == (0, k)

    def no_launch(name, *a, **kw):
        raise AssertionError(f"{name} was launched for an empty batch")
    monkeypatch.setattr(ops, "_launch", no_launch)
    out = ops.moe_grouped_gemm(ops.MOE_FWD, route, wt.shape, dtype, x=x, w=wt, gather=True)
    assert out.shape == (0, N) and out.dtype == dtype
    out = ops.moe_grouped_gemm(ops.MOE_DGRAD, route, wt.shape, dtype, w=wt, dy=dy)
    assert out.shape == (0, H) and out.dtype == dtype


COMBINE_SHAPES = [(203, 4, 96), (5, 1, 16), (64, 16, 48), (130, 3, 208)]          # T, k, H; E 16, so k 16 takes every expert


@pytest.mark.parametrize("T,k,H", COMBINE_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_combine_forward_backward(dtype, T, k, H):
    g = torch.Generator().manual_seed(2)
    E = 16
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    route = _route(ids, E)
    _, rop, _ = R.permute_ref(ids, E)
    y = torch.randn(T * k, H, generator=g).to(dtype)
    w = torch.rand(T, k, generator=g).to(dtype)
    out = ops.moe_combine_fwd_raw(y.to(DEV), w.to(DEV), route)
    ref, mag = R.combine_ref(y, w, rop, T, k)
    _within(out, ref, R.bound(ref, mag, k, dtype), "combine")
    out1 = ops.moe_combine_fwd_raw(y.to(DEV), None, route)
    ref1, mag1 = R.combine_ref(y, None, rop, T, k)
    _within(out1, ref1, R.bound(ref1, mag1, k, dtype), "scatter-back")
    dout = torch.randn(T, H, generator=g).to(dtype)
    dy, dw = ops.moe_combine_bwd_raw(dout.to(DEV), y.to(DEV), w.to(DEV), route)
    rows = torch.as_tensor(rop).view(T, k)
    ref_dy = torch.zeros(T * k, H, dtype=torch.float64)
    ref_dy[rows.reshape(-1)] = (w.double()[..., None] * dout.double()[:, None, :]).reshape(-1, H)
    _within(dy, ref_dy, R.U[dtype] * ref_dy.abs() + R.TINY[dtype], "combine dY")
    ref_dw = (dout.double()[:, None, :] * y.double()[rows]).sum(-1)
    mag_dw = (dout.double().abs()[:, None, :] * y.double().abs()[rows]).sum(-1)
    _within(dw, ref_dw, R.bound(ref_dw, mag_dw, H, dtype), "combine dw")
    dy2, dw2 = ops.moe_combine_bwd_raw(dout.to(DEV), y.to(DEV), w.to(DEV), route)
    assert torch.equal(dy, dy2) and torch.equal(dw, dw2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_combine_dropped_routing(dtype):
    """row_of_pair -1 (an id outside [0, E)): the forward sums the valid slots only, the slot's weight gradient is exactly zero, and
    dY is written - and bounded - on the rows below offsets[E], the only rows there are."""
    T, k, E = DROPPED
    H = 48
    ids = R.dropped_ids(T, k, E)
    route = _route(ids, E)
    offs, rop, _ = R.permute_ref(ids, E)
    nv = int(offs[E])
    rows = torch.as_tensor(rop).view(T, k)
    dropped = rows < 0
    assert int(dropped.sum()) == T * k - nv > 0 and route.row_of_pair.cpu().tolist() == rop.tolist()
    g = torch.Generator().manual_seed(2)
    y = torch.randn(T * k, H, generator=g).to(dtype)
    w = torch.rand(T, k, generator=g).to(dtype)
    dout = torch.randn(T, H, generator=g).to(dtype)
    for ww in (w, None):
        out = ops.moe_combine_fwd_raw(y.to(DEV), None if ww is None else ww.to(DEV), route)
        ref, mag = R.combine_ref(y, ww, rop, T, k)
        _within(out, ref, R.bound(ref, mag, k, dtype), "combine over dropped pairs" if ww is not None else "scatter-back over dropped pairs")
    both = dropped.all(1)
    if bool(both.any()):
        assert bool((out[both.to(DEV)] == 0).all())
    dy, dw = ops.moe_combine_bwd_raw(dout.to(DEV), y.to(DEV), w.to(DEV), route)
    assert bool((dw.cpu()[dropped] == 0).all())
    ref_dy = torch.zeros(T * k, H, dtype=torch.float64)
    ref_dy[rows[~dropped]] = (w.double()[..., None] * dout.double()[:, None, :])[~dropped]
    _within(dy[:nv], ref_dy[:nv], R.U[dtype] * ref_dy[:nv].abs() + R.TINY[dtype], "combine dY below offsets[E]")
    yv = y.double()[rows.clamp(min=0)] * (~dropped)[..., None]
    ref_dw = (dout.double()[:, None, :] * yv).sum(-1)
    mag_dw = (dout.double().abs()[:, None, :] * yv.abs()).sum(-1)
    _within(dw, ref_dw, R.bound(ref_dw, mag_dw, H, dtype), "combine dw")


def test_moe_return_codes():
    L = lib()
    s = torch.cuda.current_stream().cuda_stream
    t = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = t.data_ptr()
    torch.cuda.synchronize()
    assert L.dta_moe_router_fwd(p, p, p, p, 4, 300, 2, 1, 0, s) == -2            # E > 256
    assert L.dta_moe_router_fwd(p, p, p, p, 4, 64, 17, 1, 0, s) == -2            # k > 16
    assert L.dta_moe_router_fwd(p, p, p, p, 4, 8, 9, 1, 0, s) == -1             # k > E
    assert L.dta_moe_router_fwd(None, p, p, p, 4, 8, 2, 1, 0, s) == -1
    assert L.dta_moe_router_bwd(p, p, p, p, None, 4, 8, 2, 1, 0, s) == -1
    assert L.dta_moe_router_fwd(p, p, p, p, 4, 8, 2, 1, 7, s) == -2             # dtype
    assert L.dta_moe_permute(p, 4, 2, 300, p, p, p, p, p, s) == -2
    assert L.dta_moe_permute(p, 4, 2, 8, None, p, p, p, p, s) == -1
    assert L.dta_moe_grouped_gemm(0, p, p, None, p, None, p, p, 8, 4, 40, 32, 0, s) == -2     # N % 16
    assert L.dta_moe_grouped_gemm(0, p, p, None, p, None, p, p, 8, 4, 32, 24, 0, s) == -2     # K % 16
    assert L.dta_moe_grouped_gemm(3, p, p, None, p, None, p, p, 8, 4, 32, 32, 0, s) == -1     # mode
    assert L.dta_moe_grouped_gemm(0, None, p, None, p, None, p, p, 8, 4, 32, 32, 0, s) == -1  # fwd without x
    assert L.dta_moe_grouped_gemm(0, p + 2, p, None, p, None, p, p, 8, 4, 32, 32, 0, s) == -3  # alignment
    assert L.dta_moe_combine_fwd(p, p, None, p, 4, 2, 16, 0, s) == -1
    assert L.dta_moe_combine_bwd(p, p, p, p, p, None, 4, 2, 16, 0, s) == -1
    assert L.dta_moe_tile_bound(1000, 128) == -(-1000 // BM) + 128
    assert L.dta_moe_permute_workspace(1000, 128) == 4 * 128
    torch.cuda.synchronize()
