"""The log-prob / entropy kernels (dta_logprob_entropy_fwd, _shard_stats, _bwd; plain and soft-capped) against float64, element by
element: every output of every call within the bound tests/logprob_ref64.py derives from the kernels' documented arithmetic - at the
vocabulary sizes where the vector loop makes 0, 1, exactly one full and a partial second pass, with and without a scalar tail; at every
label position that takes another branch; with 0, 1, 7, 300 and (capped) 2050 extra picks, a CSR slice with absolute offsets, padded and
differing row strides, the NULL-pointer forms of the raw entries, peaked / flat / monotone / large-magnitude / masked rows, bf16, f16 and
fp32 storage.  Every call is repeated and must be bit-identical; the in-place backward must equal the out-of-place one bitwise.
tests/test_logprob_ref64.py shows on the CPU that the bounds hold for an honest emulation and reject the corruptions a whole-tensor norm
lets through.  The float64 references run on the device.

Each test prints its worst err / bound per output (pytest -s shows them)."""
import json

import numpy as np
import pytest
import torch

import logprob_ref64 as L
import ref64_common
from dynamictreeattn_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
SENTINEL = 777.0


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def _report(name, dtype, worst):
    print(f"\nWORST {name} {str(dtype).split('.')[-1]} " + json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _strided(x, pad):
    """x [R, V] on the device inside a buffer whose row stride is V rounded up to 8 plus `pad`; the padding holds NaN (never read)."""
    R, V = x.shape
    buf = torch.full((R, (V + 7) // 8 * 8 + pad), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, :V] = x.to(DEV)
    return buf[:, :V]


def _rand(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _full_case(x, labels, ptr, exl, glp, gex, gent, T, cap, worst, label, in_pad=8, out_pad=24):
    """Forward, shard statistics, out-of-place and in-place backward of one problem, every output against its bound.  x: CPU [R, V]
    (the rows of this call); ptr [R + 1] may hold absolute offsets into larger exl / gex arrays."""
    R, V = x.shape
    xd = _strided(x, in_pad)
    labels, ptr, exl, glp, gex, gent = _dev(labels, ptr, exl, glp, gex, gent)
    F = 0 if exl is None else exl.numel()
    f0, f1 = (int(ptr[0]), int(ptr[R])) if ptr is not None else (0, 0)

    def fwd():
        lp2 = torch.full((F,), SENTINEL, dtype=F32, device=DEV) if ptr is not None else None
        return (*ops.logprob_entropy_fwd_raw(xd, labels, True, T, ptr, exl, lp2, cap), lp2)

    lse, ent, lp, lp2 = fwd()
    for a, b in zip((lse, ent, lp, lp2), fwd()):
        assert a is None or _same(a, b), label + ": a repeated forward differs"
    ref = L.fwd_ref(xd, labels, ptr, exl, T, cap)
    _merge(worst, L.check_all("fwd", {"lse": lse, "entropy": ent, "logprob": lp, "extra_logprob": None if lp2 is None else lp2[f0:f1]},
                              ref, label))
    if lp2 is not None:
        assert bool((lp2[:f0] == SENTINEL).all()) and bool((lp2[f1:] == SENTINEL).all()), label + ": wrote outside its CSR slice"

    def stats():
        pk = torch.full((F,), SENTINEL, dtype=F32, device=DEV) if ptr is not None else None
        return ops.logprob_entropy_shard_stats_raw(xd, labels, T, ptr, exl, pk, cap), pk

    st, pk = stats()
    st2, pk2 = stats()
    assert _same(st, st2) and (pk is None or _same(pk, pk2)), label + ": repeated shard statistics differ"
    view = L.stats_view(st); view["extra_picked"] = None if pk is None else pk[f0:f1]
    _merge(worst, L.check_all("stats", view, L.stats_ref(xd, labels, ptr, exl, T, cap), label))

    def bwd(inplace):
        if inplace:
            xi = _strided(x, in_pad)
            return ops.logprob_entropy_bwd_raw(xi, labels, lse, ent, glp, gent, T, ptr, exl, gex, softcap=cap)
        out = _strided(torch.zeros_like(x), out_pad)
        return ops.logprob_entropy_bwd_raw(xd, labels, lse, ent, glp, gent, T, ptr, exl, gex, out=out, softcap=cap)

    dl = bwd(False)
    assert _same(xd, x.to(DEV)), label + ": the out-of-place backward changed its input"
    _merge(worst, L.check_all("bwd", {"dlogits": dl}, L.bwd_ref(xd, labels, ptr, exl, lse, ent, glp, gex, gent, T, cap), label))
    assert _same(dl, bwd(False)), label + ": a repeated backward differs"
    assert _same(dl, bwd(True)), label + ": the in-place backward differs from the out-of-place one"
    return xd, lse, ent, dl


def _sweep(V, dtype, cap, worst, kinds, R=3):
    """Every row kind at one V: T cycles through {0.25, 1, 4} (large rows: their own), the labels through label_positions(V) so that all
    of them appear, the extra picks per row through 0 / 1 / 7."""
    npos = len(L.label_positions(V))
    for i, kind in enumerate(kinds):
        for j in range(-(-npos // R)):
            n = i * 3 + j
            T = L.large_temp(dtype) if kind == "large" else (0.25, 1.0, 4.0)[n % 3]
            x = L.rows(kind, R, V, dtype, 1000 * V + n)
            labels = L.labels_for(R, V, shift=j * R)
            per_row = (0, 1, 7)[(n + i) % 3]
            ptr, exl = L.extras(R, V, labels, per_row, n) if per_row else (None, None)
            gex = _rand(exl.numel(), n + 1) if per_row else None
            _full_case(x, labels, ptr, exl, _rand(R, n + 2), gex, _rand(R, n + 3), T, cap, worst,
                       f"{kind} V={V} T={T} cap={cap} picks={per_row} labels={labels.tolist()}")


# ------------------------------------------------------------------------------------------------ a - d: sizes, temperatures, labels, picks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1, 7, 8, 9, 2040, 2048, 2049, 2056, 4104])
def test_every_vocabulary_size(V, dtype):
    """0, 1, exactly one full and a partial second pass of the vector loop, with and without a tail; every row kind from V = 2056 on."""
    worst = {}
    _sweep(V, dtype, 0.0, worst, L.KINDS if V >= 2056 else ("randn", "flat", "asc"))
    _report(f"plain V={V}", dtype, worst)


def test_largest_vocabulary():
    """V = 151 936 + 5: 75 passes of the vector loop and a tail; labels in the last vector, the first tail element."""
    worst = {}
    V, R = 151941, 2
    x = L.rows("randn", R, V, BF, 5)
    labels = torch.tensor([8 * (V // 8) - 1, 8 * (V // 8)])
    ptr, exl = L.extras(R, V, labels, 7, 5)
    _full_case(x, labels, ptr, exl, _rand(R, 1), _rand(exl.numel(), 2), _rand(R, 3), 1.0, 0.0, worst, f"V={V}")
    _report(f"plain V={V}", BF, worst)


@pytest.mark.parametrize("dtype", DTYPES)
def test_300_picks_and_a_csr_slice(dtype):
    """300 distinct picks on a row (the `f += 256` loops wrap); rows [2, 5) of a 6-row problem with absolute offsets (the chunked call of
    ops._HeadRows): nothing outside the slice is read or written."""
    worst = {}
    R, V = 2, 2061
    x = L.rows("randn", R, V, dtype, 3)
    labels = torch.tensor([2048 + 13, 7])
    ptr, exl = L.extras(R, V, labels, 300, 3)
    _full_case(x, labels, ptr, exl, _rand(R, 1), _rand(exl.numel(), 2), _rand(R, 3), 1.0, 0.0, worst, "300 picks")
    R, V = 6, 264
    x = L.rows("randn", R, V, dtype, 4)
    labels = L.labels_for(R, V)
    ptr, exl = L.extras(R, V, labels, 7, 4)
    _full_case(x[2:5], labels[2:5], ptr[2:6], exl, _rand(3, 1), _rand(exl.numel(), 2), _rand(3, 3), 4.0, 0.0, worst, "CSR slice")
    _full_case(x[2:5], labels[2:5], ptr[2:6], exl, _rand(3, 1), _rand(exl.numel(), 2), _rand(3, 3), 1.0, 30.0, worst, "capped CSR slice")
    _report("300 picks, CSR slice", dtype, worst)


# ------------------------------------------------------------------------------------------------ e: strides
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_strides(dtype):
    """A tight input stride with a padded output, a padded input with a tight output, both padded alike (every other test: 8 and 24)."""
    worst = {}
    R, V = 3, 2061
    x = L.rows("randn", R, V, dtype, 9)
    labels = L.labels_for(R, V, 3)
    ptr, exl = L.extras(R, V, labels, 7, 9)
    for in_pad, out_pad in ((0, 4096), (4096, 0), (16, 16)):
        _full_case(x, labels, ptr, exl, _rand(R, 1), _rand(exl.numel(), 2), _rand(R, 3), 1.0, 0.0, worst, f"pads {in_pad} {out_pad}",
                   in_pad, out_pad)
    _report("strides", dtype, worst)


# ------------------------------------------------------------------------------------------------ f: NULL pointers at the raw entries
@pytest.mark.parametrize("cap", [0.0, 30.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_pointer_forms(dtype, cap):
    worst = {}
    R, V, T = 3, 2061, 1.0
    x = L.rows("randn", R, V, dtype, 11)
    labels = L.labels_for(R, V, 2)
    ptr, exl = L.extras(R, V, labels, 7, 11)
    glp, gex, gent = _rand(R, 1), _rand(exl.numel(), 2), _rand(R, 3)
    xd, lse, ent, _ = _full_case(x, labels, ptr, exl, glp, gex, gent, T, cap, worst, "all pointers")
    labels, ptr, exl, glp, gex, gent = _dev(labels, ptr, exl, glp, gex, gent)
    l2, e2, p2 = ops.logprob_entropy_fwd_raw(xd, labels, False, T, softcap=cap)                     # no entropy
    assert e2 is None and _same(l2, lse)
    _merge(worst, L.check_all("fwd", {"logprob": p2}, L.fwd_ref(xd, labels, None, None, T, cap), "no entropy"))
    l3, e3, p3 = ops.logprob_entropy_fwd_raw(xd, None, True, T, softcap=cap)                        # no labels / logprob
    assert p3 is None and _same(l3, lse) and _same(e3, ent)
    for name, a in (("only g_logprob", dict(labels=labels, glp=glp)), ("only g_entropy", dict(ent=ent, gent=gent)),
                    ("only g_extra", dict(ptr=ptr, exl=exl, gex=gex))):
        a = {**dict(labels=None, glp=None, ent=None, gent=None, ptr=None, exl=None, gex=None), **a}
        out = _strided(torch.zeros_like(x), 24)
        ops.logprob_entropy_bwd_raw(xd, a["labels"], lse, a["ent"], a["glp"], a["gent"], T, a["ptr"], a["exl"], a["gex"], out=out, softcap=cap)
        ref = L.bwd_ref(xd, a["labels"], a["ptr"], exl, lse, a["ent"], a["glp"], a["gex"], a["gent"], T, cap)
        _merge(worst, L.check_all("bwd", {"dlogits": out}, ref, name))
    _report(f"NULL forms cap={cap}", dtype, worst)


# ------------------------------------------------------------------------------------------------ g: the soft-capped form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cap", [3.0, 30.0])
@pytest.mark.parametrize("V", [7, 264, 2056])
def test_capped_form(V, cap, dtype):
    worst = {}
    _sweep(V, dtype, cap, worst, L.KINDS if V >= 2056 else ("randn", "flat", "asc"))
    _report(f"capped {cap} V={V}", dtype, worst)


@pytest.mark.parametrize("dtype", [BF, F32])
def test_capped_backward_beyond_its_pick_stash(dtype):
    """2050 distinct extra picks on one row: out of place every element is within its bound; in place exactly the elements of picks
    2048 and 2049 are NaN (dta.h) and every other element has the out-of-place bits."""
    worst = {}
    V, T, cap = 2056, 1.0, 30.0
    x = L.rows("randn", 1, V, dtype, 21)
    labels = torch.tensor([9])
    ptr, exl = L.extras(1, V, None, 2050, 21)
    assert exl.unique().numel() == 2050
    glp, gex, gent = _rand(1, 1), _rand(2050, 2), _rand(1, 3)
    xd = _strided(x, 8)
    labels, ptr, exl, glp, gex, gent = _dev(labels, ptr, exl, glp, gex, gent)
    lp2 = torch.empty(2050, dtype=F32, device=DEV)
    lse, ent, lp = ops.logprob_entropy_fwd_raw(xd, labels, True, T, ptr, exl, lp2, cap)
    _merge(worst, L.check_all("fwd", {"lse": lse, "entropy": ent, "logprob": lp, "extra_logprob": lp2}, L.fwd_ref(xd, labels, ptr, exl, T, cap)))
    out = _strided(torch.zeros_like(x), 24)
    ops.logprob_entropy_bwd_raw(xd, labels, lse, ent, glp, gent, T, ptr, exl, gex, out=out, softcap=cap)
    _merge(worst, L.check_all("bwd", {"dlogits": out}, L.bwd_ref(xd, labels, ptr, exl, lse, ent, glp, gex, gent, T, cap)))
    xi = _strided(x, 8)
    ops.logprob_entropy_bwd_raw(xi, labels, lse, ent, glp, gent, T, ptr, exl, gex, softcap=cap)
    beyond = torch.zeros(V, dtype=torch.bool, device=DEV); beyond[exl[2048:]] = True
    assert bool(torch.isnan(xi[0, beyond]).all()) and int(torch.isnan(xi).sum()) == 2
    assert _same(xi[0, ~beyond], out[0, ~beyond])
    _report("capped, 2050 picks", dtype, worst)


# ------------------------------------------------------------------------------------------------ h: shard statistics
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,cuts", [(304, (96, 208)), (2056, (8, 1024, 1024))])
def test_shard_statistics_and_their_combine(V, cuts, dtype):
    """stats of every shard per element (local labels, -1 = owned elsewhere); row 0's maximum lies in one shard by a margin of 200, so
    the other shards' s 2^(m - M) underflow; combined by the arithmetic of ops.combine_shard_stats (plain sums for the all-reduces)
    the result lies within the bounds of the unsharded float64 lse / entropy / logprob."""
    worst = {}
    R, T = 4, 1.0
    x = L.rows("randn", R, V, dtype, V).float()
    x[0, cuts[0] + 5] += 200.0
    x = x.to(dtype)
    labels = torch.tensor([cuts[0] + 5, 3, V - 1, cuts[0]])
    ptr, exl = L.extras(R, V, labels, 7, V)
    exl = exl.clamp(0, V - 1)
    xd = _strided(x, 8)
    labels_d, ptr_d, exl_d = _dev(labels, ptr, exl)
    parts, extra_parts, a = [], [], 0
    for n in cuts:
        xs = xd[:, a:a + n]                                                     # a slice of the whole: base 16 / 32-byte aligned, row stride of the whole
        ll, el = ops.local_labels(labels_d, a, n), ops.local_labels(exl_d, a, n)
        pk = torch.empty(exl.numel(), dtype=F32, device=DEV)
        st = ops.logprob_entropy_shard_stats_raw(xs, ll, T, ptr_d, el, pk)
        st2 = ops.logprob_entropy_shard_stats_raw(xs, ll, T, ptr_d, el, torch.empty_like(pk))
        assert _same(st, st2)
        view = L.stats_view(st); view["extra_picked"] = pk
        _merge(worst, L.check_all("stats", view, L.stats_ref(xs, ll, ptr_d, el, T), f"shard at {a}"))
        parts.append(st); extra_parts.append(pk)
        a += n
    # ops.combine_shard_stats with sums in place of the all-reduces
    M = torch.stack([p[:, 0] for p in parts]).max(0).values
    f = [torch.exp2(p[:, 0] - M) for p in parts]
    assert min(float(fi[0]) for fi in f) == 0.0, "row 0: the other shards underflow"
    S, Tt = sum(p[:, 1] * fi for p, fi in zip(parts, f)), sum(p[:, 2] * fi for p, fi in zip(parts, f))
    picked, extra = sum(p[:, 3] for p in parts), sum(extra_parts)
    lse = (M + torch.log2(S)) * ops._LN2
    ent = lse - (Tt / S) * ops._LN2
    rw = torch.repeat_interleave(torch.arange(R, device=DEV), (ptr_d[1:] - ptr_d[:-1]).long())
    got = {"lse": lse, "entropy": ent, "logprob": picked - lse, "extra_logprob": extra - lse[rw]}
    _merge(worst, {"combined." + k: v for k, v in L.check_all("combined", got, L.fwd_ref(xd, labels_d, ptr_d, exl_d, T)).items()})
    _report(f"shards {cuts}", dtype, worst)


# ------------------------------------------------------------------------------------------------ i: the public autograd functions
@pytest.mark.parametrize("dtype", [BF, F32])
def test_public_logprob_entropy_gradient(dtype):
    worst = {}
    R, V, T = 5, 2061, 0.7
    x = L.rows("randn", R, V, dtype, 31)
    labels = L.labels_for(R, V, 1).clamp(-1, V - 1)
    g1, g2 = _dev(_rand(R, 1), _rand(R, 2))
    xd = ops._rows_for_kernel(x.to(DEV)).detach().requires_grad_(True)
    lab = labels.to(DEV)
    lp, ent = ops.logprob_entropy(xd, lab, T, True)
    ((lp * g1).sum() + (ent * g2).sum()).backward()
    ref = L.fwd_ref(xd.detach(), lab, None, None, T)
    _merge(worst, L.check_all("public", {"logprob": lp.detach(), "entropy": ent.detach()}, ref))
    lse32, ent32, _ = ops.logprob_entropy_fwd_raw(xd.detach(), lab, True, T)          # the lse the backward received (bit-identical repeat)
    assert _same(ent32, ent.detach())
    assert xd.grad.dtype == dtype
    _merge(worst, L.check_all("public", {"dlogits": xd.grad}, L.bwd_ref(xd.detach(), lab, None, None, lse32, ent32, g1, None, g2, T)))
    _report("ops.logprob_entropy", dtype, worst)


def test_public_lm_head_rows_gradient():
    """ops.lm_head_rows with chunked rows (recomputed logits) and forks on both sides of the chunk edges: dh element-wise.  dh = dlogits W
    is a GEMM over V of the kernel's rounded dlogits: the bound carries each element's dlogits bound through |W|, and the GEMM term of
    ref64_common.bound."""
    worst = {}
    g = torch.Generator().manual_seed(0)
    T_, H, V, chunk = 300, 64, 1000, 128
    h = (torch.randn(T_, H, generator=g) * 0.5).bfloat16().to(DEV).requires_grad_(True)
    W = (torch.randn(V, H, generator=g) * 0.2).bfloat16().to(DEV).requires_grad_(True)
    nxt = torch.randint(0, V, (T_,), generator=g).to(DEV)
    fork_rows = torch.tensor([3, 3, 127, 128, 250, 299]); fork_tok = torch.tensor([5, 9, 77, 500, 999, 0]).to(DEV)
    fork_ptr = torch.searchsorted(fork_rows, torch.arange(T_ + 1)).to(torch.int32).to(DEV)
    bounds = np.searchsorted(fork_rows.numpy(), np.arange(0, T_ + chunk, chunk)).tolist()
    go = _dev(_rand(T_, 1), _rand(6, 2), _rand(T_, 3))
    a, b, c = ops.lm_head_rows(h, W, nxt, fork_ptr, fork_tok, fork_rows.to(DEV), bounds, True, chunk, 0)
    ((a * go[0]).sum() + (b * go[1]).sum() + (c * go[2]).sum()).backward()
    with torch.no_grad():
        logits = torch.cat([torch.mm(h[s:s + chunk], W.t()) for s in range(0, T_, chunk)])          # as _HeadRows forms them, chunk by chunk
        lp2 = torch.empty(6, dtype=F32, device=DEV)
        lse, ent, lp = ops.logprob_entropy_fwd_raw(logits, nxt, True, 1.0, fork_ptr, fork_tok, lp2)
        assert _same(lp, a.detach()) and _same(lp2, b.detach()) and _same(ent, c.detach()), "the chunked calls differ from one call over all rows"
        _merge(worst, L.check_all("head", {"logprob": a, "extra_logprob": b, "entropy": c}, L.fwd_ref(logits, nxt, fork_ptr, fork_tok, 1.0)))
        gref, gbound = L.bwd_ref(logits, nxt, fork_ptr, fork_tok, lse, ent, go[0], go[1], go[2], 1.0)["dlogits"]
        W64 = W.double()
        dh, mag = gref @ W64, gref.abs() @ W64.abs()
        _merge(worst, {"dh": L.check("head.dh", h.grad, dh, gbound @ W64.abs() + ref64_common.bound(dh, mag, V, BF))})
    _report("ops.lm_head_rows", BF, worst)


# ------------------------------------------------------------------------------------------------ masked columns
@pytest.mark.parametrize("with_ent", [True, False])
@pytest.mark.parametrize("cap", [0.0, 30.0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_masked_columns(dtype, cap, with_ent):
    """A -inf logit, and a finite one whose scaled value overflows (finfo.min at T = 1; -1e9 in fp32 at T = 0.25, which underflows p),
    has probability 0: nothing added to lse, entropy or any shard statistic, a gradient of exactly 0, and the rest of the row equal to
    the float64 result of the row WITHOUT that column.  One and 40 masked columns, in the vector part and in the tail.  A label on a
    -inf column yields logprob = -inf.  (Under a cap a -inf logit is x' = -c; its gradient is exactly 0 through 1 - tanh^2.)"""
    worst = {}
    R, V = 2, 2061
    fmin = float(torch.finfo(dtype).min)
    cases = [("vector", 1, None, 1.0), ("vector", 40, None, 1.0), ("tail", 1, None, 1.0), ("tail", 5, fmin, 1.0), ("vector", 40, fmin, 1.0)]
    if dtype == F32:
        cases.append(("vector", 40, -1e9, 0.25))
    for i, (where, n, value, T) in enumerate(cases):
        x, cols = L.mask_columns(L.rows("randn", R, V, dtype, 40 + i), n, where, value)
        labels = torch.tensor([2048 + 5, 6])
        assert not bool(torch.isin(labels, cols).any())
        label = f"{n} masked in the {where} part, value {value}, T={T}"
        gent = _rand(R, 3) if with_ent else None
        xd, lse, ent, dl = _full_case(x, labels, None, None, _rand(R, 1), None, gent, T, cap, worst, label)
        assert bool((dl[:, cols.to(DEV)] == 0).all()), label + ": the gradient of a masked column is not exactly 0"
        if not with_ent:                                                        # the backward proper, without the entropy operand
            out = _strided(torch.zeros_like(x), 24)
            ops.logprob_entropy_bwd_raw(xd, labels.to(DEV), lse, None, _rand(R, 1).to(DEV), None, T, out=out, softcap=cap)
            assert _same(out, dl)
        if cap == 0:
            keep = torch.ones(V, dtype=torch.bool); keep[cols] = False
            small = L.fwd_ref(x[:, keep].to(DEV), None, None, None, T)
            _merge(worst, {"removed." + k: v for k, v in L.check_all("removed", {"lse": lse, "entropy": ent}, small, label).items()})
            dsmall = L.bwd_ref(x[:, keep].to(DEV), None, None, None, lse, ent if with_ent else None, None, None,
                               None if gent is None else gent.to(DEV), T)
            if with_ent:                                                        # no label here: the entropy gradient of the shorter row
                out = _strided(torch.zeros_like(x), 24)
                ops.logprob_entropy_bwd_raw(xd, None, lse, ent, None, gent.to(DEV), T, out=out)
                _merge(worst, {"removed.dlogits": L.check("removed.dlogits", out[:, keep.to(DEV)], *dsmall["dlogits"], label)})
            if value is None:
                on = torch.tensor([int(cols[0]), 6]).to(DEV)
                _, _, lp = ops.logprob_entropy_fwd_raw(xd, on, True, T)
                assert float(lp[0]) == float("-inf")
                _merge(worst, L.check_all("fwd", {"logprob": lp}, L.fwd_ref(xd, on, None, None, T), label))
    _report(f"masked cap={cap} entropy gradient={with_ent}", dtype, worst)
