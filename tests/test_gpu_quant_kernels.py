"""dta_quant_blockwise / dta_dequant_blockwise on the GPU, bit for bit against the host mirror (quant.quantize_host / dequantize_host; for
fp8 the mirror is ``(x.float() / scale).clamp(-448, 448).to(torch.float8_e4m3fn)``): codes and scales of the quantiser; the row-major and
the transposed expansion at bf16 / f16 / f32; an input at a pitch above its row; outputs written into the middle of a larger stacked
buffer whose other elements keep their fill.

Contents (tests/quantcases.py `content`), placed block by block from the first row on, as far as the shape has blocks: an all-zero
block; one element of the input type's largest finite value among tiny ones; a block whose absmax element is negative; nf4 - every one of
the 15 midpoints, and the next float above each, at absmax 1 (fp32 input: the midpoints are fp32 values); fp8 - every tie between two
neighbouring e4m3 values at scale 1; block absmax 2^-10 .. 2^-100.  The rest is random with a log-normal scale per row.  Scales in the
fp32 subnormal range are not tested."""
import pytest
import torch

import arena as A
import quantcases as qc
from dynamictreeattn_amd import ops, quant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _ids(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None


@pytest.mark.parametrize("in_dtype", OUT_DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt,R,C", qc.SHAPES, ids=qc.shape_id)
def test_quantise_codes_and_scales(fmt, R, C, in_dtype):
    w = qc.content(R, C, fmt, in_dtype, seed=R + C)
    q_ref, s_ref = quant.quantize_host(w, fmt)
    q, s = ops.quant_blockwise(w.to(DEV), fmt)
    A.assert_same_bits(s.cpu(), s_ref, f"{fmt} [{R}, {C}] {in_dtype} scales")
    A.assert_same_bits(q.cpu(), q_ref, f"{fmt} [{R}, {C}] {in_dtype} codes")
    # the same matrix as a window of a wider one (ld_w > C)
    wide = torch.full((R, C + 72), 7.0, dtype=in_dtype, device=DEV)
    wide[:, 8:8 + C] = w.to(DEV)
    q2, s2 = ops.quant_blockwise(wide[:, 8:8 + C], fmt)
    A.assert_same_bits(s2.cpu(), s_ref, f"{fmt} [{R}, {C}] {in_dtype} scales at ld_w = C + 72")
    A.assert_same_bits(q2.cpu(), q_ref, f"{fmt} [{R}, {C}] {in_dtype} codes at ld_w = C + 72")


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt,R,C", qc.SHAPES, ids=qc.shape_id)
def test_dequantise_row_major_and_transposed(fmt, R, C, out_dtype):
    q, s = qc.codes(R, C, fmt, seed=R + C)
    ref = quant.dequantize_host(q, s, fmt, out_dtype)
    qd, sd = q.to(DEV), s.to(DEV)
    out = torch.empty((R, C), dtype=out_dtype, device=DEV)
    ops.dequant_blockwise(qd, sd, fmt, out)
    A.assert_same_bits(out.cpu(), ref, f"{fmt} [{R}, {C}] {out_dtype} row-major")
    out_t = torch.empty((C, R), dtype=out_dtype, device=DEV)
    ops.dequant_blockwise(qd, sd, fmt, out_t, transposed=True)
    A.assert_same_bits(out_t.cpu(), ref.t().contiguous(), f"{fmt} [{R}, {C}] {out_dtype} transposed")


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=_ids)
@pytest.mark.parametrize("fmt,R,C", [s_ for s_ in qc.SHAPES if s_[1] in (3, 5, 129, 130, 257)], ids=qc.shape_id)
def test_dequantise_into_the_middle_of_a_stacked_operand(fmt, R, C, out_dtype):
    """Row-major at ld_out > C: rows [16, 16 + R) and columns [V, V + C) of a larger buffer.  Transposed: columns [16, 16 + R) of a
    [C, R + 40] buffer (rows that start on 16 bytes) and of a [C, R + 37] one (rows that do not).  Everything else keeps its fill."""
    q, s = qc.codes(R, C, fmt, seed=R + C)
    ref = quant.dequantize_host(q, s, fmt, out_dtype)
    qd, sd = q.to(DEV), s.to(DEV)
    V = 16 // torch.empty(0, dtype=out_dtype).element_size()
    fill = -3.0
    big = torch.full((R + 40, C + 2 * V), fill, dtype=out_dtype, device=DEV)
    ops.dequant_blockwise(qd, sd, fmt, big[16:16 + R, V:V + C])
    got = big.cpu()
    A.assert_same_bits(got[16:16 + R, V:V + C], ref, f"{fmt} [{R}, {C}] {out_dtype} row-major window")
    got[16:16 + R, V:V + C] = fill
    assert bool((got == fill).all()), "row-major: an element outside the window changed"
    for pad in (40, 37):
        big_t = torch.full((C, R + pad), fill, dtype=out_dtype, device=DEV)
        ops.dequant_blockwise(qd, sd, fmt, big_t[:, 16:16 + R], transposed=True)
        got = big_t.cpu()
        A.assert_same_bits(got[:, 16:16 + R].contiguous(), ref.t().contiguous(), f"{fmt} [{R}, {C}] {out_dtype} transposed window, pitch R + {pad}")
        got[:, 16:16 + R] = fill
        assert bool((got == fill).all()), f"transposed, pitch R + {pad}: an element outside the window changed"


def test_quantise_then_dequantise_on_the_device_equals_the_mirror_chain():
    """The two kernels in sequence, as quantize_base and the engine use them (QuantLinear.from_weight, QuantLinear.weight)."""
    for fmt in ("nf4", "fp8"):
        w = qc.content(257, 1024, fmt, torch.bfloat16, seed=11)
        lin = quant.QuantLinear.from_weight(w.to(DEV), None, fmt)
        q, s = quant.quantize_host(w, fmt)
        A.assert_same_bits(lin.weight.cpu(), quant.dequantize_host(q, s, fmt, torch.bfloat16), f"{fmt} QuantLinear.weight")
