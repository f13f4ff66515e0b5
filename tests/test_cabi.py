"""The C-ABI library loads without a GPU and exports every symbol include/dta.h declares; the row-kernel, MoE and LoRA entries refuse
bad arguments before any HIP call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported():
    import torch  # noqa: F401  - torch's own libamdhip64 must be resident first (as _lib.lib() arranges): ONE HIP runtime per process
    from dynamictreeattn_amd.build import build_native
    lib = ctypes.CDLL(build_native())
    header = open(os.path.join(ROOT, "include", "dta.h")).read()
    declared = set(re.findall(r"^int\s+(dta_\w+)\s*\(", header, flags=re.M))
    assert len(declared) >= 8
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.dta_version() >= 100
    from dynamictreeattn_amd import _lib
    assert set(_lib.EXPORTS) <= declared | {"dta_version"}
    _lib.lib()


def test_row_kernel_entries_refuse_bad_arguments_without_a_gpu():
    """Refused calls only: a refusal returns before any HIP call (a valid call without a GPU would return DTA_EPRIOR).  One 64-byte
    aligned host buffer stands for every pointer.  Order of the statuses in include/dta.h: DTA_EINVAL -1, DTA_EUNSUPPORTED -2, DTA_EALIGN -3."""
    from dynamictreeattn_amd import _lib
    lib = _lib.lib()
    raw = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(raw) + 63) & ~63
    nan, inf = float("nan"), float("inf")

    def lp_fwd(logits=p, stride=64, dtype=0, cap=0.0):       # R = 4, V = 64, temperature 1
        return lib.dta_logprob_entropy_fwd(logits, p, p, p, p, p, p, p, 4, 64, stride, 1.0, dtype, cap, None)

    def rms_fwd(x=p, H=64, off=0.0):
        return lib.dta_rmsnorm_fwd(x, p, p, p, p, p, 4, H, 1e-6, off, 0, None)

    assert lp_fwd(cap=nan) == -1 and lp_fwd(cap=inf) == -1
    assert lp_fwd(dtype=7) == -2
    assert lp_fwd(logits=p + 2) == -3 and lp_fwd(stride=12) == -3
    assert rms_fwd(off=nan) == -1
    assert rms_fwd(H=60) == -2
    assert lib.dta_rmsnorm_bwd(p, p, p, p, p, p, p, 4, 8200, 0.0, 0, None) == -2
    assert rms_fwd(x=p + 2) == -3
    for glu in (lib.dta_geglu_fwd, lib.dta_swiglu_fwd):
        assert glu(p, p, p, 4, 64, 56, 0, None) == -1        # ld < cols
    assert lib.dta_sum_slabs(p, 2, 64, 64, None, p, 7, None) == -2                                # out_dtype

    # MoE entries: the refusals of test_gpu_moe_ops.py::test_moe_return_codes
    assert lib.dta_moe_router_fwd(p, p, p, p, 4, 300, 2, 1, 0, None) == -2                        # E > 256
    assert lib.dta_moe_router_fwd(p, p, p, p, 4, 64, 17, 1, 0, None) == -2                        # k > 16
    assert lib.dta_moe_router_fwd(p, p, p, p, 4, 8, 9, 1, 0, None) == -1                          # k > E
    assert lib.dta_moe_router_fwd(None, p, p, p, 4, 8, 2, 1, 0, None) == -1
    assert lib.dta_moe_router_bwd(p, p, p, p, None, 4, 8, 2, 1, 0, None) == -1
    assert lib.dta_moe_router_fwd(p, p, p, p, 4, 8, 2, 1, 7, None) == -2                          # dtype
    assert lib.dta_moe_permute(p, 4, 2, 300, p, p, p, p, p, None) == -2
    assert lib.dta_moe_permute(p, 4, 2, 8, None, p, p, p, p, None) == -1
    assert lib.dta_moe_grouped_gemm(0, p, p, None, p, None, p, p, 8, 4, 40, 32, 0, None) == -2    # N % 16
    assert lib.dta_moe_grouped_gemm(0, p, p, None, p, None, p, p, 8, 4, 32, 24, 0, None) == -2    # K % 16
    assert lib.dta_moe_grouped_gemm(3, p, p, None, p, None, p, p, 8, 4, 32, 32, 0, None) == -1    # mode
    assert lib.dta_moe_grouped_gemm(0, None, p, None, p, None, p, p, 8, 4, 32, 32, 0, None) == -1  # fwd without x
    assert lib.dta_moe_grouped_gemm(0, p + 2, p, None, p, None, p, p, 8, 4, 32, 32, 0, None) == -3  # alignment
    assert lib.dta_moe_combine_fwd(p, p, None, p, 4, 2, 16, 0, None) == -1
    assert lib.dta_moe_combine_bwd(p, p, p, p, p, None, 4, 2, 16, 0, None) == -1
    assert lib.dta_moe_tile_bound(1000, 128) == -(-1000 // 128) + 128
    assert lib.dta_moe_permute_workspace(1000, 128) == 4 * 128

    # LoRA entries: the refusals of test_gpu_lora_ops.py::test_status_codes
    assert lib.dta_lora_down(p, 1024, p, 1024, p, 16, None, 64, 16, 1000, 0, None) == -2          # K % 16
    assert lib.dta_lora_down(p, 1024, p, 1024, p, 257, None, 64, 257, 1024, 0, None) == -2        # r > 256
    assert lib.dta_lora_down(p, 1024, p, 1024, p, 16, None, 64, 16, 1024, 2, None) == -2          # fp32
    assert lib.dta_lora_down(None, 1024, p, 1024, p, 16, None, 64, 16, 1024, 0, None) == -1
    assert lib.dta_lora_down(p, 1024, p, 1024, None, 16, None, 64, 16, 1024, 0, None) == -1
    assert lib.dta_lora_down(p, 512, p, 1024, p, 16, None, 64, 16, 1024, 0, None) == -1           # pitch < row

    def wg(l_, x_, part_, R=16, K=1024):
        return lib.dta_lora_wgrad(l_, 16, x_, 1024, part_, None, 64, R, K, 0, None)

    assert wg(None, p, p) == -1 and wg(p, None, p) == -1 and wg(p, p, None) == -1
    assert wg(p, p, p, K=1000) == -2
    assert lib.dta_lora_wgrad(p, 300, p, 1024, p, None, 64, 257, 1024, 0, None) == -2
    assert lib.dta_lora_wgrad_slabs(-1, 16) == -1


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dynamictreeattn_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn
