"""Containment of the ten mixture-of-experts kernels (router forward / backward, the three permutation kernels, the grouped GEMM in its
three modes on the MFMA and the fp32 path, combine forward / backward): every entry is called through the C ABI on guarded arenas
(tests/arena.py) and must return 0, leave every guard byte of its outputs and workspaces alone, write every output element
(bit-identical payloads under the NaN / 0x7f7f7f7f and the -3.0 / 0x01010101 fill, floats finite under NaN), not depend on memory past
an input's extent (floats: NaN against +inf; index tables: 0 against the table's largest valid value) and give, bit for bit, what the
allocating ops.* wrapper gives for the same inputs - whose values tests/test_gpu_moe_ops.py bounds against float64 (every form called
here, the weight gradient without the gather included).

Dropped pairs (an id outside [0, E)) take no row, so the permutation leaves src_token, and the combine backward dY, unwritten from row
offsets[E] on: those two payloads are passed as scratch (guards checked, content not) and their first offsets[E] rows compared afterwards.

Guards: 128 rows (DTA_MOE_BM) at the payload's pitch around the GEMM operands and outputs, one workgroup's rows (4) around the router's
and the combine's buffers, a chunk of pairs around the permutation's tables.  dta_moe_combine_bwd refuses a NULL topk_w, so the
"w NULL" form exists for the forward alone (the scatter-back of the gathered GEMM input).

Limits (tests/arena.py): a stray load whose value is discarded is not seen; a stray store further than the guard band is not caught;
no time is measured and no tolerance is used - every comparison is bitwise."""
import functools

import pytest
import torch

import arena as A
import moe_ref64 as R
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib
from test_gpu_moe_ops import BM, COUNTS, DROPPED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
DTYPES = [BF, F16, F32]


_in, _out, _same = functools.partial(A.in_arena, device=DEV), functools.partial(A.out_arena, device=DEV), A.assert_matches


# ------------------------------------------------------------------------------------------------ router
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,k", [(8, 1), (60, 8), (256, 16)])
def test_router_forward_backward(E, k, dtype):
    T = 5
    g = torch.Generator().manual_seed(E + k)
    logits, dw = (2.0 * torch.randn(T, E, generator=g)).to(dtype), torch.randn(T, k, generator=g).to(dtype)
    for norm in (1, 0):
        label = f"router T={T} E={E} k={k} norm={norm}"

        def fwd(fill, poison):
            a = {"logits": _in("logits", logits, poison, guard_rows=4), "topk_ids": _out("topk_ids", (T, k), I32, fill, guard_rows=4),
                 "topk_w": _out("topk_w", (T, k), dtype, fill, guard_rows=4), "lse": _out("lse", (T,), F32, fill, guard_rows=64)}
            A.launch("dta_moe_router_fwd", a["logits"], a["topk_ids"], a["topk_w"], a["lse"], T, E, k, norm, ops._DT[dtype])
            return a
        got = A.check_case(fwd, label + " fwd")
        ids, w, lse = ops.moe_router_fwd_raw(logits.to(DEV), k, bool(norm))
        _same(got, {"topk_ids": ids, "topk_w": w, "lse": lse}, label + " fwd")
        ids_h, lse_h = ids.cpu(), lse.cpu()

        def bwd(fill, poison):
            a = {"logits": _in("logits", logits, poison, guard_rows=4), "lse": _in("lse", lse_h, poison, guard_rows=64),
                 "topk_ids": _in("topk_ids", ids_h, poison, hi=E - 1, guard_rows=4), "dtopk_w": _in("dtopk_w", dw, poison, guard_rows=4),
                 "dlogits": _out("dlogits", (T, E), dtype, fill, guard_rows=4)}
            A.launch("dta_moe_router_bwd", a["logits"], a["lse"], a["topk_ids"], a["dtopk_w"], a["dlogits"], T, E, k, norm, ops._DT[dtype])
            return a
        _same(A.check_case(bwd, label + " bwd"), {"dlogits": ops.moe_router_bwd_raw(logits.to(DEV), lse, ids, dw.to(DEV), bool(norm))}, label + " bwd")


# ------------------------------------------------------------------------------------------------ permutation
def _permute_run(ids, E):
    T, k = ids.shape
    P = T * k
    n_ws, bound = lib().dta_moe_permute_workspace(P, E), lib().dta_moe_tile_bound(P, E)

    def run(fill, poison):
        a = {"topk_ids": _in("topk_ids", ids, poison, hi=E - 1, guard_rows=256), "workspace": _out("workspace", (n_ws,), I32, fill, guard_rows=256),
             "expert_offsets": _out("expert_offsets", (E + 1,), I32, fill, guard_rows=256), "row_of_pair": _out("row_of_pair", (P,), I32, fill, guard_rows=256),
             "src_token": _out("src_token", (P,), I32, fill, guard_rows=256), "tiles": _out("tiles", (2 * bound,), I32, fill, guard_rows=256)}
        A.launch("dta_moe_permute", a["topk_ids"], T, k, E, a["workspace"], a["expert_offsets"], a["row_of_pair"], a["src_token"], a["tiles"])
        run.arenas = a
        return a
    return run


@pytest.mark.parametrize("case", ["empty_experts", "one_expert", "dropped"])
def test_permutation(case):
    """The workspace has exactly dta_moe_permute_workspace(P, E) ints and starts as 0x7f7f7f7f or 0x01010101: the kernels may not need it
    zeroed.  tiles has exactly 2 * dta_moe_tile_bound(P, E) ints, and every entry past the last tile is written as {-1, 0}."""
    if case == "empty_experts":
        T, k, E = 300, 2, 60
        ids = torch.stack([torch.tensor([5, 40]) if i % 3 else torch.tensor([40, 59]) for i in range(T)]).int()
    elif case == "one_expert":
        T, k, E = 700, 1, 128
        ids = torch.full((T, k), 77, dtype=I32)
    else:
        T, k, E = DROPPED
        ids = R.dropped_ids(T, k, E).int()
    run = _permute_run(ids, E)
    got = A.check_case(run, f"permute {case}", scratch=("src_token",) if case == "dropped" else ())
    r = ops.moe_permute(ids.to(DEV), E)
    offs, rop, src = R.permute_ref(ids.long(), E)
    nv = int(offs[E])
    assert (nv < T * k) == (case == "dropped")
    got.setdefault("src_token", run.arenas["src_token"].payload())          # dropped: the tail from row offsets[E] on is unwritten
    _same(got, {"expert_offsets": r.expert_offsets, "row_of_pair": r.row_of_pair, "tiles": r.tiles}, f"permute {case}")
    A.assert_same_bits(got["src_token"][:nv], r.src_token[:nv], f"permute {case} src_token below offsets[E]: the arena call against the ops wrapper")
    assert got["expert_offsets"].cpu().tolist() == offs.tolist() and got["row_of_pair"].cpu().tolist() == rop.tolist()
    assert got["src_token"].cpu()[:nv].tolist() == src[:nv].tolist()
    tiles = got["tiles"].cpu().view(-1, 2)
    want = [(e, int(o)) for e in range(E) for o in range(offs[e], offs[e + 1], BM)]
    assert [tuple(t) for t in tiles[:len(want)].tolist()] == want
    assert bool((tiles[len(want):, 0] == -1).all()) and bool((tiles[len(want):, 1] == 0).all()), "padding entries of the tile table"


# ------------------------------------------------------------------------------------------------ grouped GEMM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,H,N", [(8, 32, 96), (8, 48, 32)])
def test_grouped_gemm(E, H, N, dtype):
    """Per-expert row counts 0, 1, 127, 128, 129, 0, 259, 5; forward and wgrad with the gather and without, dgrad (which reads no x).
    The wgrad slabs of the two empty experts must come back as written zeros under the NaN fill."""
    g = torch.Generator().manual_seed(H + N)
    ids = torch.cat([torch.full((c,), e) for e, c in enumerate(COUNTS)])
    ids = ids[torch.randperm(len(ids), generator=g)][:, None].int()                     # k = 1: T = sum(COUNTS)
    T = ids.shape[0]
    route = ops.moe_permute(ids.to(DEV), E)
    offs, tiles, src = route.expert_offsets.cpu(), route.tiles.cpu(), route.src_token.cpu()
    assert tiles.numel() == 2 * lib().dta_moe_tile_bound(T, E)
    x, w, dy = torch.randn(T, H, generator=g).to(dtype), (torch.randn(E, N, H, generator=g) / H ** 0.5).to(dtype), torch.randn(T, N, generator=g).to(dtype)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    for mode, gather in ((0, True), (0, False), (1, False), (2, True), (2, False)):
        label = f"grouped_gemm mode={mode} gather={gather} E={E} H={H} N={N}"
        shape = (T, N) if mode == 0 else (T, H) if mode == 1 else (E, N, H)
        rows = BM if mode < 2 else -(-BM // N)                                        # 128 rows of the output at its pitch

        def run(fill, poison):
            a = {"expert_offsets": _in("expert_offsets", offs, poison, hi=T, guard_rows=64),
                 "tiles": _in("tiles", tiles, poison, hi=min(E - 1, T - 1), guard_rows=64), "out": _out("out", shape, dtype, fill, guard_rows=rows)}
            if mode != 1:
                a["x"] = _in("x", x, poison, guard_rows=BM)
            if mode != 2:
                a["w"] = _in("w", w, poison, guard_rows=-(-BM // N))
            if mode != 0:
                a["dy"] = _in("dy", dy, poison, guard_rows=BM)
            if gather:
                a["gather"] = _in("gather", src, poison, hi=T - 1, guard_rows=BM)
            A.launch("dta_moe_grouped_gemm", mode, a.get("x"), a.get("w"), a.get("dy"), a["out"], a.get("gather"), a["expert_offsets"], a["tiles"],
                     T, E, N, H, ops._DT[dtype])
            return a
        got = A.check_case(run, label)
        args = dict(x=xd, w=wd) if mode == 0 else dict(w=wd, dy=dyd) if mode == 1 else dict(x=xd, dy=dyd)
        _same(got, {"out": ops.moe_grouped_gemm(mode, route, w.shape, dtype, gather=gather, **args)}, label)
        if mode == 2:
            empty = [e for e in range(E) if offs[e + 1] == offs[e]]
            assert len(empty) == 2 and all(bool((got["out"][e] == 0).all()) for e in empty), label + ": the slab of an empty expert is not zero"


# ------------------------------------------------------------------------------------------------ combine
def _combine_case(dtype, T, k, E, H, ids):
    """Combine forward (with and without weights) and backward over the routing of ids [T, k].  nv = offsets[E] rows exist; with dropped
    pairs nv < T * k, dY is unwritten from row nv on (scratch: guards only) and its first nv rows are compared afterwards."""
    g = torch.Generator().manual_seed(2)
    route = ops.moe_permute(ids.to(DEV), E)
    rop, nv = route.row_of_pair.cpu(), int(route.expert_offsets[E])
    assert int((rop < 0).sum()) == T * k - nv
    y, w, dout = torch.randn(T * k, H, generator=g).to(dtype), torch.rand(T, k, generator=g).to(dtype), torch.randn(T, H, generator=g).to(dtype)
    for with_w in (True, False):
        label = f"combine_fwd w={with_w} rows={nv}/{T * k}"

        def fwd(fill, poison):
            a = {"y": _in("y", y, poison, guard_rows=4), "row_of_pair": _in("row_of_pair", rop, poison, hi=T * k - 1, guard_rows=64),
                 "out": _out("out", (T, H), dtype, fill, guard_rows=4)}
            if with_w:
                a["topk_w"] = _in("topk_w", w, poison, guard_rows=4)
            A.launch("dta_moe_combine_fwd", a["y"], a.get("topk_w"), a["row_of_pair"], a["out"], T, k, H, ops._DT[dtype])
            return a
        _same(A.check_case(fwd, label), {"out": ops.moe_combine_fwd_raw(y.to(DEV), w.to(DEV) if with_w else None, route)}, label)

    label = f"combine_bwd rows={nv}/{T * k}"
    last = {}

    def bwd(fill, poison):
        a = {"dout": _in("dout", dout, poison, guard_rows=4), "y": _in("y", y, poison, guard_rows=4), "topk_w": _in("topk_w", w, poison, guard_rows=4),
             "row_of_pair": _in("row_of_pair", rop, poison, hi=T * k - 1, guard_rows=64), "dy": _out("dy", (T * k, H), dtype, fill, guard_rows=4),
             "dtopk_w": _out("dtopk_w", (T, k), dtype, fill, guard_rows=4)}
        A.launch("dta_moe_combine_bwd", a["dout"], a["y"], a["topk_w"], a["row_of_pair"], a["dy"], a["dtopk_w"], T, k, H, ops._DT[dtype])
        last[fill, poison] = a["dy"]
        return a
    dy, dw = ops.moe_combine_bwd_raw(dout.to(DEV), y.to(DEV), w.to(DEV), route)
    got = A.check_case(bwd, label, scratch=("dy",) if nv < T * k else ())
    if nv == T * k:
        _same(got, {"dy": dy, "dtopk_w": dw}, label)
        return
    _same(got, {"dtopk_w": dw}, label)
    assert bool((got["dtopk_w"][(rop < 0).view(T, k).to(DEV)] == 0).all()), label + ": the weight gradient of a dropped pair is not zero"
    rows = {key: a.payload()[:nv] for key, a in last.items()}            # the written rows, under both fills and both input poisons
    A.assert_written(rows["A", 0], "A", label + " dy below offsets[E]")
    A.assert_same_bits(rows["A", 0], rows["B", 0], label + " dy below offsets[E]: fill A against fill B")
    A.assert_same_bits(rows["A", 0], rows["A", 1], label + " dy below offsets[E]: input poison NaN/0 against +inf/max")
    A.assert_same_bits(rows["A", 0], dy[:nv], label + " dy below offsets[E]: the arena call against the ops wrapper")
    for (fill, _), a in last.items():                                    # ... and from row offsets[E] on nothing was stored: still the fill
        tail = a.payload()[nv:]
        assert bool(torch.isnan(tail).all() if fill == "A" else (tail == A.fill_value(dtype, fill)).all()), label + ": a store behind offsets[E]"


@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_forward_backward(dtype):
    g = torch.Generator().manual_seed(2)
    T, k, E, H = 203, 4, 16, 96
    _combine_case(dtype, T, k, E, H, torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).int())


@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_dropped_routing(dtype):
    T, k, E = DROPPED
    _combine_case(dtype, T, k, E, 48, R.dropped_ids(T, k, E).int())
