"""Containment of the two quantisation kernels (dta_quant_blockwise, dta_dequant_blockwise): each entry is called through the C ABI on
guarded arenas (tests/arena.py) and must return 0, leave every guard byte alone - the pitch gaps of a strided output among them -, write
every output element (bit-identical payloads under the two fills), not depend on memory past an input's extent (the pitch gaps of a
weight at ld_w > C; the bands around the codes and the scales) and give, bit for bit, what the allocating ops.* wrapper gives in the
dense layout - whose values tests/test_gpu_quant_kernels.py compares with the host mirror.

Every form: both formats, both orientations, bf16 / f16 / f32, the dense and the strided outputs (row-major at ld_out = C + 16 bytes;
transposed at a pitch that keeps the rows on 16 bytes and at one that does not), an input weight at a pitch above its row.  Shapes:
ragged row counts around the 64-row tile of the transposed form and the 16-row step of the row-major one.

The quantiser's codes are uint8 and arena fill A is the byte 0x7f, which `check_case` takes for "unwritten": the inputs are built so
that no code byte is 0x7f (nf4: the absmax element of every block is negative and no other element reaches the top level, so code 15
does not occur; fp8: 0x7f is a NaN encoding, which a finite input never yields).

Limits (tests/arena.py): a stray load whose value is discarded is not seen; a stray store further than the guard band is not caught;
no time is measured and no tolerance is used - every comparison is bitwise."""
import functools

import pytest
import torch

import arena as A
import quantcases as qc
from dynamictreeattn_amd import ops, quant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SHAPES = [s for s in qc.SHAPES if s[1] in (3, 5, 129, 130)]
_in = functools.partial(A.in_arena, device=DEV)


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else str(v)


def _weight_without_top_code(R, C, fmt, dtype, seed):
    B = quant.BLOCK[fmt]
    w = torch.randn(R, C, generator=torch.Generator().manual_seed(seed)).clamp(-3, 3)
    w = torch.where(w > 0, 0.5 * w, w).view(-1, B)
    w[:, 0] = -4.0
    return w.view(R, C).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("pitch", [0, 8], ids=["dense", "strided"])
@pytest.mark.parametrize("fmt,R,C", SHAPES, ids=_ids)
def test_quantise(fmt, R, C, pitch, dtype):
    w = _weight_without_top_code(R, C, fmt, dtype, R + C)
    nb, qcols = C // quant.BLOCK[fmt], (C // 2 if fmt == "nf4" else C)
    label = f"quant {fmt} [{R}, {C}] ld_w = C + {pitch} {dtype}"

    def run(fill, poison):
        a = {"w": _in("w", w, poison, strides=(C + pitch, 1), guard_rows=4),
             "q": A.out_arena("q", (R, qcols), torch.uint8, fill, guard_rows=4, device=DEV),
             "scales": A.out_arena("scales", (R, nb), torch.float32, fill, guard_rows=4, device=DEV)}
        A.launch("dta_quant_blockwise", a["w"], C + pitch, R, C, ops._DT[dtype], ops.QUANT_FMT[fmt], a["q"], a["scales"])
        return a
    got = A.check_case(run, label)
    q, s = ops.quant_blockwise(w.to(DEV), fmt)
    A.assert_matches(got, {"q": q, "scales": s}, label)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("form", ["rows", "rows_strided", "transposed", "transposed_strided16", "transposed_strided_odd"])
@pytest.mark.parametrize("fmt,R,C", SHAPES, ids=_ids)
def test_dequantise(fmt, R, C, form, dtype):
    q, s = quant.quantize_host(_weight_without_top_code(R, C, fmt, torch.float32, R + C), fmt)      # moderate values: finite in f16 too
    V = 16 // torch.empty(0, dtype=dtype).element_size()
    transposed = form.startswith("transposed")
    shape = (C, R) if transposed else (R, C)
    ld = shape[1] + {"rows": 0, "rows_strided": V, "transposed": 0, "transposed_strided16": 2 * V - shape[1] % V, "transposed_strided_odd": V + 3 - shape[1] % V}[form]
    label = f"dequant {fmt} [{R}, {C}] {form} ld_out = {ld} {dtype}"

    def run(fill, poison):
        a = {"q": _in("q", q, poison, hi=0x7E, guard_rows=4), "scales": _in("scales", s, poison, guard_rows=4),
             "out": A.out_arena("out", shape, dtype, fill, strides=(ld, 1), guard_rows=64, device=DEV)}
        A.launch("dta_dequant_blockwise", a["q"], a["scales"], R, C, ops.QUANT_FMT[fmt], a["out"], ld, ops._DT[dtype], int(transposed))
        return a
    got = A.check_case(run, label)
    want = torch.empty(shape, dtype=dtype, device=DEV)
    ops.dequant_blockwise(q.to(DEV), s.to(DEV), fmt, want, transposed)
    A.assert_matches(got, {"out": want}, label)
