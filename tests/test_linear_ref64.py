"""CPU: the bounds of tests/linear_ref64.py hold for an honest restatement of ops._wgrad's split-K arithmetic and of the LM head's weight
gradient, and reject every corruption of them - among those the ones the whole-tensor norm of 3e-3
(tests/test_gpu_properties.py::test_split_k_weight_gradient_equals_the_single_gemm) lets through, which stays on record here as the reason
for the per-element tests of tests/test_gpu_linear_bounds.py.

Operands.  "gauss": N(0, 1), the operands of the GPU tests.  The product of T = 8 k rows cancels to |ref| ~ sqrt(T) while the fp32 term of
the bound follows |dy|ᵀ|x| ~ T: in bf16 the output rounding u |ref| still carries three quarters of the bound and a second rounding shows
(1.5 - 1.7 x); in f16 (u eight times smaller) the fp32 term is 2.5 x the rounding term, the honest form sits at 0.5 and a second rounding
of the result or of the slabs reaches only 0.7 - 1.04 - below what the bound resolves.  "one_signed": |N(0, 1)| (x scaled by 1/4 to stay
far from f16's range): nothing cancels, u |ref| is the bound, and f16 shows both double roundings at 1.3 - 1.5 x.  So the two corruptions
that are a second ROUNDING (`round_slabs`, `round_then_rest`) are asserted on gauss operands in bf16 and on one-signed operands in f16;
every other corruption on gauss operands in both types."""
import functools

import pytest
import torch

import linear_ref64 as R
import logprob_ref64 as L
from ref64_common import bound

BF, F16 = torch.bfloat16, torch.float16
TS = [8192, 8193, 8447]                   # no left-over row, one, 255
PAIRS = [(256, 512), (72, 200)]           # (out, in)
NORM_BAR = 3e-3
SECOND_ROUNDINGS = ("round_slabs", "round_then_rest")
ID = {BF: "bf16", F16: "f16"}


@functools.lru_cache(maxsize=None)
def _problem(kind, dtype, T, out_f, in_f):
    """(x, dy, ref, bound) - built once, shared by every test and left unchanged."""
    g = torch.Generator().manual_seed(1000 * out_f + T)
    x, dy = torch.randn(T, in_f, generator=g), torch.randn(T, out_f, generator=g)
    if kind == "one_signed":
        x, dy = x.abs() * 0.25, dy.abs()
    x, dy = x.to(dtype), dy.to(dtype)
    ref, mag, n = R.wgrad_ref(x, dy)
    return x, dy, ref, bound(ref, mag, n, dtype)


def _changes_anything(corrupt, T, transposed):
    if corrupt in R.LEFT_OVER_ONLY:
        return R.split_plan(T)[1] < T
    return transposed if corrupt == "not_transposed_back" else True


def test_the_row_counts_are_the_three_left_over_cases():
    assert [T - R.split_plan(T)[1] for T in TS] == [0, 1, 255] and all(R.takes_split(T, 256, 512, BF) for T in TS)
    assert not R.takes_split(8191, 256, 512, BF) and not R.takes_split(8193, 2048, 2304, BF) and R.takes_split(8193, 2048, 2048, BF)
    assert not R.takes_split(8193, 256, 512, torch.float32)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dtype,kind", [(BF, "gauss"), (F16, "gauss"), (F16, "one_signed")], ids=["bf16-gauss", "f16-gauss", "f16-one_signed"])
def test_honest_split_is_inside_the_bound(dtype, kind, T, pair, transposed):
    x, dy, ref, bnd = _problem(kind, dtype, T, *pair)
    got = R.emulate_wgrad(x, dy, dtype, None, transposed)
    worst = R.check(f"cpu.wgrad.{kind}", got, ref, bnd, f"T={T} {pair} transposed={transposed}")
    print(f"\nWORST cpu wgrad honest {ID[dtype]} {kind} T={T} {pair} transposed={transposed}: {worst:.3f}, norm {R.norm_error(got, ref):.2e}")
    assert R.norm_error(got, ref) <= NORM_BAR


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("corrupt", R.CORRUPTIONS)
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
def test_every_corruption_is_rejected(dtype, corrupt, T, pair, transposed):
    if not _changes_anything(corrupt, T, transposed):
        x, dy, ref, bnd = _problem("gauss", dtype, T, *pair)          # nothing to corrupt here: the corrupted form IS the honest one
        assert torch.equal(R.emulate_wgrad(x, dy, dtype, corrupt, transposed), R.emulate_wgrad(x, dy, dtype, None, transposed))
        return
    kind = "one_signed" if (dtype == F16 and corrupt in SECOND_ROUNDINGS) else "gauss"
    x, dy, ref, bnd = _problem(kind, dtype, T, *pair)
    got = R.emulate_wgrad(x, dy, dtype, corrupt, transposed)
    worst = R.ratio(got, ref, bnd)
    print(f"\nWORST cpu wgrad {corrupt} {ID[dtype]} {kind} T={T} {pair} transposed={transposed}: {worst:.3g}, norm {R.norm_error(got, ref):.2e}")
    assert worst > 1.0


def test_check_raises_on_an_element_over_the_bound_and_on_a_shape():
    x, dy, ref, bnd = _problem("gauss", BF, 8193, 72, 200)
    got = R.emulate_wgrad(x, dy, BF, None, False)
    assert R.check("cpu.check", got, ref, bnd) <= 1.0
    bad = got.clone(); bad[3, 7] += 8.0
    with pytest.raises(AssertionError, match=r"1 of 14400 elements over the bound.*\(row 3, column 7\)"):
        R.check("cpu.check.bad", bad, ref, bnd)
    with pytest.raises(AssertionError, match="shape"):
        R.check("cpu.check.bad", got.t(), ref, bnd)
    assert R.ratio(got.t(), ref, bnd) == float("inf") and R.ratio(torch.full_like(got, float("nan")), ref, bnd) == float("inf")


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("T,corrupt", [(8192, "round_slabs"), (8193, "round_slabs"), (8447, "round_slabs"), (8193, "round_then_rest"), (8447, "round_then_rest")])
@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
def test_the_whole_tensor_norm_lets_the_second_roundings_through(dtype, T, corrupt, pair):
    """Why the per-element tests exist: slabs rounded to the model dtype (the batched GEMM without its fp32 output type) and a result
    rounded before the left-over rows are added both pass the 3e-3 norm, in either type and on either kind of operand."""
    for kind in ("gauss", "one_signed"):
        x, dy, ref, bnd = _problem(kind, dtype, T, *pair)
        got = R.emulate_wgrad(x, dy, dtype, corrupt, False)
        assert not torch.equal(got, R.emulate_wgrad(x, dy, dtype, None, False))
        assert R.norm_error(got, ref) <= NORM_BAR


def test_the_norm_does_catch_the_gross_corruptions():
    """... and the norm is not useless: a dropped or doubled left-over row and a slab taken twice exceed it (so does the element bound)."""
    for T, corrupt in ((8193, "drop_rest"), (8193, "rest_twice"), (8192, "slab_twice")):
        x, dy, ref, bnd = _problem("gauss", BF, T, 256, 512)
        assert R.norm_error(R.emulate_wgrad(x, dy, BF, corrupt, False), ref) > NORM_BAR


# ------------------------------------------------------------------------------------------------ the head's chunk term
@functools.lru_cache(maxsize=None)
def _head_problem(kind, dtype):
    """T = 2 x 4096 rows, V = 64, H = 64.  "random": Gaussian rows.  "aligned": the rows of a chunk all equal (two different rows for the
    two chunks), so that the rounding of a dlogits element and of a chunk's product point the same way in all 4096 rows - the input at
    which a bound has to hold, not the typical one."""
    T, V, H = 8192, 64, 64
    g = torch.Generator().manual_seed(0)
    if kind == "random":
        h, x = torch.randn(T, H, generator=g) * 0.5, torch.randn(T, V, generator=g) * 3
        labels, g1, g2 = torch.randint(0, V, (T,), generator=g), torch.randn(T, generator=g), torch.randn(T, generator=g)
    else:
        h = (torch.randn(2, H, generator=g) * 0.5).repeat_interleave(T // 2, 0)
        x = (torch.randn(2, V, generator=g) * 3).repeat_interleave(T // 2, 0)
        labels, g1, g2 = torch.full((T,), 5), torch.full((T,), 0.731), torch.full((T,), -0.377)
    h, x = h.to(dtype), x.to(dtype)
    f = L.fwd_ref(x, labels, None, None, 1.0)
    lse32, ent32 = f["lse"][0].float(), f["entropy"][0].float()
    refs = {ch: R.head_dw_ref(h, x, labels, None, None, lse32, ent32, g1, None, g2, chunk=ch) for ch in (None, 4096)}
    gref, gbound = refs[None][2:]
    gk = gref.float().to(dtype)                   # the kernel's dlogits: ONE rounding of the exact value
    assert R.ratio(gk, gref, gbound) <= 1.0
    return h, gk, refs


@pytest.mark.parametrize("dtype", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind", ["random", "aligned"])
def test_head_weight_gradient_bound_with_and_without_the_chunk_term(kind, dtype):
    h, gk, refs = _head_problem(kind, dtype)
    once, per_chunk = R.emulate_head_dw(gk, h, dtype, None), R.emulate_head_dw(gk, h, dtype, 4096)
    (dw, plain), with_term = refs[None][:2], refs[4096][1]
    r = {"once/plain": R.ratio(once, dw, plain), "chunks/with": R.ratio(per_chunk, dw, with_term), "chunks/plain": R.ratio(per_chunk, dw, plain)}
    print(f"\nWORST cpu head dW {ID[dtype]} {kind} " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert r["once/plain"] <= 1.0                    # one rounding: inside without the term
    assert r["chunks/with"] <= 1.0                   # a rounding per chunk: inside with it
    assert not torch.equal(once, per_chunk)
    if kind == "aligned" and dtype == BF:
        assert r["chunks/plain"] > 1.0               # ... and outside without it (1.17; f16 1.08, printed): the term is needed, not slack
