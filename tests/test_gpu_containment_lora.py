"""Containment of the two LoRA kernels (dta_lora_down, dta_lora_wgrad): each entry is called through the C ABI on guarded arenas
(tests/arena.py) and must return 0, leave every guard byte of its output alone - the pitch gaps of an out [T, R] with ldo > R among
them -, write every output element (bit-identical payloads under the NaN and the -3.0 fill, finite under NaN), not depend on memory
past an input's extent (NaN against +inf around x [T, K] at a pitch above K, around l and m) and give, bit for bit, what the allocating
ops.* wrapper gives for the same inputs in the dense layout - whose values tests/test_gpu_lora_ops.py bounds against float64.

The pitches keep each operand on the load / store path of its dense layout (ldx = K + 8 and, for R = 16, ldo = 24 are multiples of 16
bytes like K and 16; ldo = 9 and 14 are not, like 1 and 6), and the path changes no arithmetic, so the comparison with the dense result
is bitwise.  Guards: 128 rows (the kernels' row tile) at the payload's pitch; one slab around `part`, which has exactly
dta_lora_wgrad_slabs(T, K) slabs.

Limits (tests/arena.py): a stray load whose value is discarded is not seen; a stray store further than the guard band is not caught;
no time is measured and no tolerance is used - every comparison is bitwise."""
import functools

import numpy as np
import pytest
import torch

import arena as A
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
TS, RS, KS = [1, 63, 257], [1, 6, 16], [16, 1040]


_in = functools.partial(A.in_arena, device=DEV)


def _randn(shape, dtype, seed, scale=1.0):
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(dtype)


def _rscale(R, mod):
    return (0.5 + np.arange(R) % mod).astype(np.float32) if R % 2 == 0 else None


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("T", TS)
def test_down(T, R, K, dtype):
    x, m = _randn((T, K), dtype, 1), _randn((R, K), dtype, 2, 0.2)
    rs = _rscale(R, 5)
    ldx, ldo = K + 8, R + 8
    label = f"lora_down T={T} R={R} K={K}"

    def run(fill, poison):
        a = {"x": _in("x", x, poison, strides=(ldx, 1), guard_rows=128), "m": _in("m", m, poison, guard_rows=R),
             "out": A.out_arena("out", (T, R), dtype, fill, strides=(ldo, 1), guard_rows=128, device=DEV)}
        A.launch("dta_lora_down", a["x"], ldx, a["m"], K, a["out"], ldo, None if rs is None else rs.ctypes.data, T, R, K, ops._DT[dtype])
        return a
    got = A.check_case(run, label)
    A.assert_same_bits(got["out"], ops.lora_down(x.to(DEV), m.to(DEV), rs), label + " out: the arena call against the ops wrapper")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("T", TS)
def test_wgrad(T, R, K, dtype):
    """`part` has exactly dta_lora_wgrad_slabs(T, K) slabs and starts as NaN or -3.0: every slab is written in full and none is read
    before that.  The slabs summed in order (ops.sum_slabs; a single slab as it is) are the wrapper's fp32 result."""
    l, x = _randn((T, R), dtype, 9), _randn((T, K), dtype, 10)
    rs = _rscale(R, 3)
    ldl, ldx = R + 8, K + 8
    S = lib().dta_lora_wgrad_slabs(T, K)
    label = f"lora_wgrad T={T} R={R} K={K} slabs={S}"

    def run(fill, poison):
        a = {"l": _in("l", l, poison, strides=(ldl, 1), guard_rows=128), "x": _in("x", x, poison, strides=(ldx, 1), guard_rows=128),
             "part": A.out_arena("part", (S, R, K), torch.float32, fill, guard_rows=1, device=DEV)}
        A.launch("dta_lora_wgrad", a["l"], ldl, a["x"], ldx, a["part"], None if rs is None else rs.ctypes.data, T, R, K, ops._DT[dtype])
        return a
    part = A.check_case(run, label)["part"]
    got = part[0] if S == 1 else ops.sum_slabs(part, torch.float32)
    A.assert_same_bits(got, ops.lora_wgrad(l.to(DEV), x.to(DEV), torch.float32, rs), label + " the arena's slabs against the ops wrapper")
