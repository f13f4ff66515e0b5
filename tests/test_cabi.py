"""The C-ABI library loads without a GPU and exports every symbol include/dta.h declares; the row-kernel entries refuse bad arguments
before any HIP call."""
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


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dynamictreeattn_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), fn
