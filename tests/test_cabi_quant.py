"""C ABI of the quantised frozen base (include/dta.h "Quantised frozen base"): both entries are exported, and bad arguments are
refused with the documented codes before any HIP call - the pattern of test_cabi.py::test_row_kernel_entries_refuse_bad_arguments_without_a_gpu
(a valid call without a GPU would return DTA_EPRIOR or DTA_ELAUNCH, never one of these)."""
import ctypes

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NF4, FP8 = 0, 1


def test_both_entries_are_exported():
    from dynamictreeattn_amd import _lib
    lib = _lib.lib()
    for name in ("dta_quant_blockwise", "dta_dequant_blockwise"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.dta_version() >= 270


def test_quant_entries_refuse_bad_arguments_without_a_gpu():
    from dynamictreeattn_amd import _lib
    lib = _lib.lib()
    raw = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(raw) + 63) & ~63

    def quant(w=p, ld=192, R=4, C=192, dtype=0, fmt=NF4, q=p, scales=p):
        return lib.dta_quant_blockwise(w, ld, R, C, dtype, fmt, q, scales, None)

    def dequant(q=p, scales=p, R=8, C=192, fmt=NF4, out=p, ld=192, dtype=0, transposed=0):
        return lib.dta_dequant_blockwise(q, scales, R, C, fmt, out, ld, dtype, transposed, None)

    # unknown fmt / dtype
    assert quant(fmt=2) == EUNSUPPORTED and quant(fmt=-1) == EUNSUPPORTED and quant(dtype=7) == EUNSUPPORTED
    assert dequant(fmt=2) == EUNSUPPORTED and dequant(dtype=3) == EUNSUPPORTED
    # C not a multiple of the block: 192 is three nf4 blocks and one and a half fp8 blocks
    assert quant(fmt=FP8) == EUNSUPPORTED and dequant(fmt=FP8) == EUNSUPPORTED
    assert quant(C=96, ld=96) == EUNSUPPORTED and dequant(C=96, ld=96) == EUNSUPPORTED
    assert quant(C=1 << 22, ld=1 << 22) == EUNSUPPORTED and dequant(C=1 << 22, ld=1 << 22) == EUNSUPPORTED
    # ld below the row
    assert quant(ld=191) == EINVAL
    assert dequant(ld=191) == EINVAL
    assert dequant(transposed=1, ld=7) == EINVAL                                  # transposed rows have R elements
    assert dequant(transposed=2) == EINVAL
    # sizes
    assert quant(R=0) == EINVAL and quant(C=0, ld=0) == EINVAL and dequant(R=-1) == EINVAL and dequant(C=0) == EINVAL
    # null pointers
    assert quant(w=None) == EINVAL and quant(q=None) == EINVAL and quant(scales=None) == EINVAL
    assert dequant(q=None) == EINVAL and dequant(scales=None) == EINVAL and dequant(out=None) == EINVAL
    # misaligned out (and the other 16-byte pointers); a row-major pitch off 16 bytes
    assert dequant(out=p + 2) == EALIGN and dequant(out=p + 8, transposed=1) == EALIGN
    assert dequant(q=p + 4) == EALIGN and dequant(scales=p + 4) == EALIGN
    assert dequant(ld=196) == EALIGN and dequant(ld=194, dtype=2) == EALIGN
    assert quant(q=p + 1) == EALIGN and quant(scales=p + 4) == EALIGN and quant(w=p + 1) == EALIGN
    # the order: EINVAL before EUNSUPPORTED before EALIGN
    assert dequant(ld=100, fmt=9, out=p + 2) == EINVAL and dequant(fmt=9, out=p + 2) == EUNSUPPORTED
    # 192 columns pass the nf4 block check: the same call is refused only for its pointer (refused calls only - nothing here may launch)
    assert dequant(C=192, fmt=NF4, out=p + 2) == EALIGN and quant(C=192, fmt=NF4, q=p + 1) == EALIGN
