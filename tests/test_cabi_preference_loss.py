"""dta_preference_loss refuses every bad argument include/dta.h lists, with the header's status codes, in the header's order and before
any HIP call: host buffers, no GPU (a valid call without a GPU would return DTA_EPRIOR or DTA_ELAUNCH, never one of the codes below)."""
import ctypes
import os
import re

import pytest

EINVAL, EALIGN = -1, -3
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRS = ("lp", "depth", "row_lo", "row_hi", "seq_ptr", "run_ptr", "run_row0", "run_depth0", "seq_leaf", "pair_c", "pair_r", "ref_lp", "ref_sum",
        "mask", "nhat", "u", "sft", "g", "dlp", "partial", "stats")
OPTIONAL = ("ref_lp", "ref_sum")


@pytest.fixture(scope="module")
def env():
    from dynamictreeattn_amd import _lib
    raw = ctypes.create_string_buffer(1 << 12)
    return _lib.lib(), (ctypes.addressof(raw) + 63) & ~63, raw


def _call(lib, p, T=4, S=2, M=1, R=1, P=1, kind=0, beta=0.1, eps=0.0, gamma=0.0, ln=0, free=0, sftc=0.0, scale=1.0, **ptrs):
    a = {n: ptrs.get(n, p) for n in PTRS}
    if "ref_sum" not in ptrs:
        a["ref_sum"] = None                     # the default call uses the per-token form of the reference
    return lib.dta_preference_loss(*(a[n] for n in PTRS), T, S, M, R, P, kind, beta, eps, gamma, ln, free, sftc, scale, None)


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "dta.h")).read()
    declared = set(re.findall(r"^int\s+(dta_\w+)\s*\(", header, flags=re.M))
    assert {"dta_preference_loss", "dta_preference_loss_blocks"} <= declared
    from dynamictreeattn_amd import _lib
    assert {"dta_preference_loss", "dta_preference_loss_blocks"} <= set(_lib.EXPORTS)
    assert _lib.lib().dta_version() >= 240
    decl = re.search(r"^int\s+dta_preference_loss\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    names = [re.split(r"[\s*]+", part.strip())[-1] for part in decl.split(",")]
    assert names[:21] == ["lp", "depth", "row_seq_lo", "row_seq_hi", "seq_ptr", "leaf_run_ptr", "run_row0", "run_depth0", "seq_leaf", "pair_c",
                          "pair_r", "ref_lp", "ref_sum", "mask", "nhat", "u", "sft", "g", "dlp", "partial", "stats"]
    assert names[21:] == ["T", "S", "M", "R", "P", "kind", "beta", "label_smoothing", "gamma", "length_normalize", "reference_free", "sft_coef",
                          "scale", "stream"]
    assert len(_lib._PROTOS["dta_preference_loss"][0]) == len(names)
    from dynamictreeattn_amd import losses
    assert losses.PREFERENCE_KINDS == ("sigmoid", "hinge", "ipo") and len(losses.PREFERENCE_STATS) == 8
    assert {"PreferenceLoss", "PREFERENCE_KINDS", "PREFERENCE_STATS"} <= set(losses.__all__)


def test_refusals(env):
    lib, p, _ = env
    f = lambda **kw: _call(lib, p, **kw)
    for name in PTRS:
        if name not in OPTIONAL:
            assert f(**{name: None}) == EINVAL, name
    for dim in ("T", "S", "M", "R", "P"):
        assert f(**{dim: 0}) == EINVAL and f(**{dim: -3}) == EINVAL, dim
    for bad in (-1, 3, 17):
        assert f(kind=bad) == EINVAL, bad
    for bad in (0.0, -0.1, NAN, INF, -INF):
        assert f(beta=bad) == EINVAL, bad
    for bad in (-0.1, 0.5, 0.7, NAN, INF):
        assert f(eps=bad) == EINVAL, bad
    assert f(eps=0.1, kind=1) == EINVAL and f(eps=0.1, kind=2) == EINVAL       # label smoothing goes with the sigmoid only
    assert f(gamma=NAN) == EINVAL and f(gamma=INF) == EINVAL and f(gamma=0.5, kind=2) == EINVAL
    assert f(sftc=-0.1) == EINVAL and f(sftc=NAN) == EINVAL and f(scale=NAN) == EINVAL and f(scale=INF) == EINVAL
    assert f(ref_lp=None, ref_sum=None) == EINVAL                               # a reference is needed and absent
    assert f(ref_lp=p, ref_sum=p) == EINVAL                                     # both forms given
    for name in PTRS:
        if name == "ref_sum":
            assert f(ref_lp=None, ref_sum=p + 4) == EALIGN and f(ref_lp=None, ref_sum=p + 8) == EALIGN
        else:
            assert f(**{name: p + 4}) == EALIGN and f(**{name: p + 8}) == EALIGN, name
    # the limits themselves and the legal forms are no refusal: what is left to refuse them is a misaligned pointer
    assert f(ref_lp=None, ref_sum=p, lp=p + 4) == EALIGN
    assert f(ref_lp=None, ref_sum=None, free=1, lp=p + 4) == EALIGN
    assert f(ref_lp=p + 4, ref_sum=p + 4, free=1, g=p + 8) == EALIGN             # reference_free: neither form is looked at
    assert f(eps=0.49, gamma=-2.0, ln=1, sftc=0.0, scale=-1.0, kind=0, beta=1e-6, T=1, S=1, M=1, R=1, P=1, u=p + 4) == EALIGN
    assert f(kind=1, gamma=3.0, dlp=p + 4) == EALIGN and f(kind=2, gamma=0.0, sftc=2.0, stats=p + 8) == EALIGN


def test_the_refusals_come_in_the_header_order(env):
    lib, p, _ = env
    assert _call(lib, p, T=0, lp=p + 4) == EINVAL
    assert _call(lib, p, P=0, pair_c=p + 4) == EINVAL
    assert _call(lib, p, pair_r=None, run_ptr=p + 8) == EINVAL
    assert _call(lib, p, kind=5, stats=p + 8) == EINVAL
    assert _call(lib, p, beta=0.0, mask=p + 4) == EINVAL
    assert _call(lib, p, ref_lp=None, ref_sum=None, g=p + 4) == EINVAL
    assert _call(lib, p, ref_lp=p, ref_sum=p, nhat=p + 8) == EINVAL


def test_the_workspace_rows_follow_the_pair_count(env):
    lib, _, _ = env
    q = lib.dta_preference_loss_blocks
    assert [q(1, 2, n) for n in (1, 256, 257, 1024 * 256, 1024 * 256 + 1, 1 << 30)] == [1, 1, 2, 1024, 1024, 1024]
    assert q(1 << 30, 1 << 30, 1050) == 5
    assert q(0, 2, 1) == EINVAL and q(1, 0, 1) == EINVAL and q(1, 2, 0) == EINVAL and q(-3, 5, 5) == EINVAL and q(5, 5, -1) == EINVAL
