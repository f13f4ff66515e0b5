"""GPU: the LoRA entry points (dta_lora_down, dta_lora_wgrad; csrc/lora_kernels.hip) against float64 on the kernels' rounded inputs
(tests/lora_ref64.py) with the project's per-element bound ref64_common.bound - bf16 and f16, every row count (a single row, masked tails,
the bench's 28 160), every rank class (1, not a multiple of 8, 16, 64, 200, 256) and K of one 16-step, 1024 and a non-multiple of the
tiles - bit-identical results across two calls, and the status codes; and ops.lora_linear (the operator the model layer calls: base
GEMM + adapters, each low-rank product in the form ops.py chooses for its shape - kernel or GEMM expression) against float64 with
segment layouts (one, three unequal, one missing).  An in-place y += s xa B^T kernel (scripts/diag/lora_up_add_experiment.hip) lost to addmm_ at every shape
(profiles/lora_probe.json) and is not in the product: that product is covered through lora_linear."""
import numpy as np
import pytest
import torch

import lora_ref64 as ref64
from ref64_common import U, bound
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
TS = [1, 63, 257, 4099, 28160]
RS = [1, 4, 6, 16, 64, 96, 200, 256]
KS = [16, 1024, 4096 + 16]


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)).to(dtype)


def _check(out, ref, mag, n, dtype, what):
    lim = bound(ref, mag, n, dtype)
    err = (out.double() - ref).abs()
    worst = float((err / lim).max())
    print(f"{what}: worst err / bound {worst:.3f}, max |err| {float(err.max()):.3e}")
    assert torch.isfinite(out.float()).all() and worst <= 1.0, (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("T", TS)
def test_down(T, R, K, dtype):
    x, m = _rand((T, K), dtype, 1), _rand((R, K), dtype, 2, 0.2)
    rs = (0.5 + np.arange(R) % 5).astype(np.float32) if R % 2 == 0 else None
    out = ops.lora_down(x, m, rs)
    assert out.shape == (T, R) and out.dtype == dtype
    _check(out, *ref64.down_ref(x, m, rs), dtype, f"down T={T} R={R} K={K}")
    assert torch.equal(out, ops.lora_down(x, m, rs))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("T", TS)
def test_wgrad(T, R, K, dtype):
    l, x = _rand((T, R), dtype, 9), _rand((T, K), dtype, 10)
    rs = (0.5 + np.arange(R) % 3).astype(np.float32) if R % 2 == 0 else None
    r, mag, n = ref64.wgrad_ref(l, x, rs)
    for out_dtype in (torch.float32, dtype):                              # fp32 adapters get the unrounded slab sum; else rounded once
        g = ops.lora_wgrad(l, x, out_dtype, rs)
        assert g.shape == (R, K) and g.dtype == out_dtype
        _check(g, r, mag, n, out_dtype, f"wgrad T={T} R={R} K={K} -> {out_dtype}")
        assert torch.equal(g, ops.lora_wgrad(l, x, out_dtype, rs))


def test_strided_operands_and_slab_count():
    """Row pitches larger than the row (column slices of a fused buffer) and the slab plan of the weight gradient."""
    dtype = torch.bfloat16
    big = _rand((513, 2048 + 64), dtype, 11)
    x = big[:, 64:64 + 1024]                                              # pitch 2112, 16-byte aligned start
    m = _rand((48, 1024), dtype, 12, 0.2)
    _check(ops.lora_down(x, m), *ref64.down_ref(x, m), dtype, "down strided")
    l = big[:, 3:51]                                                      # unaligned start: element loads
    _check(ops.lora_wgrad(l, x, torch.float32), *ref64.wgrad_ref(l, x), torch.float32, "wgrad strided")
    L = lib()
    assert L.dta_lora_wgrad_slabs(1, 1024) == 1 and L.dta_lora_wgrad_slabs(63, 16) == 1
    s = L.dta_lora_wgrad_slabs(28160, 1024)
    assert 32 <= s <= 64 and L.dta_lora_wgrad_slabs(28160, 4096) <= s


def test_status_codes():
    L = lib()
    x = torch.zeros((64, 1024), dtype=torch.bfloat16, device=DEV)
    m = torch.zeros((16, 1024), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((64, 16), dtype=torch.bfloat16, device=DEV)
    part = torch.zeros((1, 16, 1024), dtype=torch.float32, device=DEV)
    p = lambda t: t.data_ptr()
    EINVAL, EUNSUPPORTED = -1, -2
    assert L.dta_lora_down(p(x), 1024, p(m), 1024, p(out), 16, None, 64, 16, 1024, 0, None) == 0
    assert L.dta_lora_down(p(x), 1024, p(m), 1024, p(out), 16, None, 64, 16, 1000, 0, None) == EUNSUPPORTED      # K % 16
    assert L.dta_lora_down(p(x), 1024, p(m), 1024, p(out), 257, None, 64, 257, 1024, 0, None) == EUNSUPPORTED    # r > 256
    assert L.dta_lora_down(p(x), 1024, p(m), 1024, p(out), 16, None, 64, 16, 1024, 2, None) == EUNSUPPORTED      # fp32
    assert L.dta_lora_down(None, 1024, p(m), 1024, p(out), 16, None, 64, 16, 1024, 0, None) == EINVAL
    assert L.dta_lora_down(p(x), 1024, p(m), 1024, None, 16, None, 64, 16, 1024, 0, None) == EINVAL
    assert L.dta_lora_down(p(x), 512, p(m), 1024, p(out), 16, None, 64, 16, 1024, 0, None) == EINVAL             # pitch < row
    wg = lambda l_, x_, part_, R=16, K=1024: L.dta_lora_wgrad(l_, 16, x_, 1024, part_, None, 64, R, K, 0, None)
    assert wg(p(out), p(x), p(part)) == 0
    assert wg(None, p(x), p(part)) == EINVAL and wg(p(out), None, p(part)) == EINVAL and wg(p(out), p(x), None) == EINVAL
    assert wg(p(out), p(x), p(part), K=1000) == EUNSUPPORTED
    assert L.dta_lora_wgrad(p(out), 300, p(x), 1024, p(part), None, 64, 257, 1024, 0, None) == EUNSUPPORTED
    assert L.dta_lora_wgrad_slabs(-1, 16) == EINVAL
    torch.cuda.synchronize()


# (in, [(n0, nlen, r, scaling)], N): the q|k|v columns with their own ranks and scalings; shapes on both sides of the kernel / expression
# choices of ops._down_by_kernel and ops._wgrad_by_kernel
LINEAR_CASES = {"one": (1024, [(0, 1024, 16, 2.0)], 1024),
                "three_unequal": (2048, [(0, 2048, 6, 2.0), (2048, 1040, 16, 0.5), (3088, 1024, 4, 4.0)], 4112),
                "one_missing": (4096, [(0, 2048, 8, 2.0), (3072, 1024, 4, 4.0)], 4096),
                "wide_output": (1024, [(0, 6144, 8, 2.0), (6144, 6160, 8, 2.0)], 12304),
                "small_all_kernels": (256, [(0, 256, 6, 2.0), (384, 128, 8, 1.0)], 512)}


@pytest.mark.parametrize("adapter_dtype", ["fp32", "model"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("layout", list(LINEAR_CASES))
@pytest.mark.parametrize("T", [63, 4099])
def test_lora_linear_against_float64(T, layout, dtype, adapter_dtype):
    """y, dx and every dA / dB of ops.lora_linear against float64 autograd on the same rounded operands.  Bound: relative Frobenius
    error <= 4 u with u = 2^-8 (bf16) / 2^-11 (f16), the half-spacing of the format: xa / dxa are stored rounded (u), the base GEMM's
    output is rounded before the adapter term is added (u), the result is rounded (u) - three roundings on the worst path, one spare."""
    K, spec, N = LINEAR_CASES[layout]
    adt = torch.float32 if adapter_dtype == "fp32" else dtype
    x, w, b = _rand((T, K), dtype, 20), _rand((N, K), dtype, 21, K ** -0.5), _rand((N,), dtype, 22)
    ab = [(_rand((r, K), dtype, 30 + i, K ** -0.5).to(adt), _rand((nlen, r), dtype, 40 + i, 0.3).to(adt)) for i, (_, nlen, r, _) in enumerate(spec)]
    dy = _rand((T, N), dtype, 23)
    leaves = [x, w, b] + [t for pair in ab for t in pair]
    mine = [t.clone().requires_grad_(True) for t in leaves]
    adapters = [(n0, nlen, mine[3 + 2 * i], mine[4 + 2 * i], s) for i, (n0, nlen, r, s) in enumerate(spec)]
    y = ops.lora_linear(mine[0], mine[1], mine[2], adapters)
    y.backward(dy)
    ref = [t.double().clone().requires_grad_(True) for t in leaves]
    yr = ref[0] @ ref[1].t() + ref[2]
    cols = []
    o = 0
    for i, (n0, nlen, r, s) in enumerate(spec):
        cols += [yr[:, o:n0], yr[:, n0:n0 + nlen] + s * (ref[0] @ ref[3 + 2 * i].t()) @ ref[4 + 2 * i].t()]
        o = n0 + nlen
    yr = torch.cat(cols + [yr[:, o:]], 1)
    yr.backward(dy.double())
    lim = 4 * U[dtype] / 2                       # ref64_common.U is the doubled half-spacing
    rel = lambda a, r_: float((a.double() - r_).norm() / r_.norm())
    errs = {"y": rel(y, yr.detach())}
    for name, m_, r_ in zip(["x", "w", "b"] + [f"{ab_}{i}" for i in range(len(spec)) for ab_ in "AB"], mine, ref):
        assert m_.grad is not None and m_.grad.dtype == m_.dtype and m_.grad.shape == m_.shape, name
        errs["d" + name] = rel(m_.grad, r_.grad)
    print(f"lora_linear {layout} T={T}: {({k: round(v, 5) for k, v in errs.items()})} (bound {lim:.5f})")
    assert max(errs.values()) <= lim, errs
    untouched = torch.ones(N, dtype=torch.bool, device=DEV)
    for n0, nlen, _, _ in spec:
        untouched[n0:n0 + nlen] = False
    if untouched.any():                          # columns of a member without adapter: the base GEMM's bits
        assert torch.equal(y[:, untouched], torch.nn.functional.linear(x, w, b)[:, untouched])
    mine2 = [t.clone().requires_grad_(True) for t in leaves]
    y2 = ops.lora_linear(mine2[0], mine2[1], mine2[2], [(n0, nlen, mine2[3 + 2 * i], mine2[4 + 2 * i], s) for i, (n0, nlen, r, s) in enumerate(spec)])
    y2.backward(dy)
    assert torch.equal(y, y2) and all(torch.equal(a.grad, c.grad) for a, c in zip(mine, mine2))      # the same bits on every call


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_wgrad_dispatch_covers_both_forms(dtype):
    """ops._lora_wgrad on both sides of WGRAD_KERNEL_MAX_K: the kernel and the fp32-output GEMM both keep the sum in fp32, scale it there
    and round once to the output dtype - an fp32 result (fp32 adapters) meets the fp32 bound in either form."""
    M = ops.WGRAD_KERNEL_MAX_K
    assert ops._wgrad_by_kernel(1024) and ops._wgrad_by_kernel(4096) and ops._wgrad_by_kernel(M) and not ops._wgrad_by_kernel(M + 16)
    assert ops._down_by_kernel(1024, 32) and not ops._down_by_kernel(1024, 48) and not ops._down_by_kernel(4096, 16)
    seg = [(0, 6, 3.0), (6, 16, 0.3)]
    rs = np.ones(22, np.float32); rs[:6] = 3.0; rs[6:] = 0.3
    l, x = _rand((4099, 22), dtype, 50), _rand((4099, M + 16), dtype, 51)
    for xs, form in ((x, "GEMM"), (x[:, :4096].contiguous(), "kernel")):
        r, mag, n = ref64.wgrad_ref(l, xs, rs)
        for out_dtype in (torch.float32, dtype):
            g = ops._lora_wgrad(l, xs, out_dtype, seg)
            assert g.dtype == out_dtype and g.shape == (22, xs.shape[1])
            _check(g, r, mag, n, out_dtype, f"wgrad by {form} -> {out_dtype}")
            assert torch.equal(g, ops._lora_wgrad(l, xs, out_dtype, seg))
