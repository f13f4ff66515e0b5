"""dta_policy_loss refuses every bad argument include/dta.h lists, with the header's status codes, in the header's order and before
any HIP call: host buffers, no GPU (a valid call without a GPU would return DTA_EPRIOR or DTA_ELAUNCH, never one of the codes below).
The one entry serves every option of the objective, so the cases of a plain token-level call (no path tables, neutral options), of a
sequence-level ratio and of the off-policy / CISPO options are all asked of it."""
import ctypes
import os
import re

import pytest

EINVAL, EALIGN = -1, -3
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTRS = ("lp", "ent", "depth", "row_lo", "row_hi", "seq_ptr", "run_ptr", "run_row0", "run_depth0", "seq_leaf", "old", "ref", "rollout", "mask",
        "adv", "w", "c", "omega", "dlp", "dent", "partial", "stats")
PATH = ("run_ptr", "run_row0", "run_depth0", "seq_leaf")
OPTIONAL = ("old", "ref", "rollout") + PATH
REMOVED = ("dta_policy_loss_seq", "dta_policy_loss_seq_blocks", "dta_policy_loss_ex", "dta_policy_loss_ex_blocks")
# the three kinds of call the entry folds: their defaults, on top of the neutral options of _call
NO_TABLES = dict(M=0, R=0, **{name: None for name in PATH})
FLAVOURS = {"token": NO_TABLES, "token_with_tables": {}, "sequence": dict(ratio=1)}


@pytest.fixture(scope="module")
def env():
    from dynamictreeattn_amd import _lib
    raw = ctypes.create_string_buffer(1 << 12)
    return _lib.lib(), (ctypes.addressof(raw) + 63) & ~63, raw


def _call(lib, p, T=4, S=2, M=1, R=1, per_seq=0, cl=0.2, ch=0.2, dual=0.0, kc=0.0, est=2, ec=0.0, agg=0, scale=1.0, ratio=0, sur=0, level=0,
          mode=0, cap=2.0, floor=0.0, **ptrs):
    a = {n: ptrs.get(n, p) for n in PTRS}
    return lib.dta_policy_loss(*(a[n] for n in PTRS[:15]), per_seq, *(a[n] for n in PTRS[15:]), T, S, M, R, cl, ch, dual, kc, est, ec, agg,
                               scale, ratio, sur, level, mode, cap, floor, None)


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "dta.h")).read()
    declared = set(re.findall(r"^int\s+(dta_\w+)\s*\(", header, flags=re.M))
    assert {"dta_policy_loss", "dta_policy_loss_blocks"} <= declared
    from dynamictreeattn_amd import _lib
    assert {"dta_policy_loss", "dta_policy_loss_blocks"} <= set(_lib.EXPORTS)
    assert not set(REMOVED) & declared and not set(REMOVED) & set(_lib.EXPORTS)
    assert not any(name in header for name in REMOVED)
    assert _lib.lib().dta_version() >= 260
    from dynamictreeattn_amd import build
    assert "loss_kernels.hip" in build.SOURCES
    # the header's parameter list, in order, is the one the prototype table and this file's PTRS assume
    decl = re.search(r"^int\s+dta_policy_loss\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    names = [re.split(r"[\s*]+", part.strip())[-1] for part in decl.split(",")]
    assert names[:15] == ["lp", "ent", "depth", "row_seq_lo", "row_seq_hi", "seq_ptr", "leaf_run_ptr", "run_row0", "run_depth0", "seq_leaf",
                          "old_lp", "ref_lp", "rollout_lp", "mask", "adv"]
    assert names[15:] == ["adv_per_seq", "w", "c", "omega", "dlp", "dent", "partial", "stats", "T", "S", "M", "R", "clip_low", "clip_high",
                          "dual_clip", "kl_coef", "kl_estimator", "entropy_coef", "agg", "scale", "ratio_level", "surrogate", "is_level",
                          "is_mode", "is_cap", "is_floor", "stream"]
    protos = _lib._PROTOS["dta_policy_loss"][0]
    assert len(protos) == len(names)
    # ... and so are the types: the header's pointers, int32_t and float are the table's void pointers, c_int32 and c_float
    kinds = [ctypes.c_void_p if "*" in part else ctypes.c_float if "float" in part else ctypes.c_int32 for part in decl.split(",")]
    assert list(protos) == kinds
    blocks = re.search(r"^int\s+dta_policy_loss_blocks\s*\(([^;]*)\);", header, flags=re.M).group(1)
    assert [part.split()[-1] for part in blocks.split(",")] == ["T", "S"] and _lib._PROTOS["dta_policy_loss_blocks"][0] == [ctypes.c_int32] * 2


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_refusals(env, flavour):
    """what a plain token-level call, the same call with path tables and a call with a sequence-level ratio must all refuse"""
    lib, p, _ = env
    base = FLAVOURS[flavour]
    f = lambda **kw: _call(lib, p, **{**base, **kw})
    walks = flavour == "sequence"
    given = [name for name in PTRS if base.get(name, p) is not None]
    for name in given:
        if name not in OPTIONAL or (walks and name in PATH):
            assert f(**{name: None}) == EINVAL, name
    for dim in ("T", "S") + (("M", "R") if walks else ()):
        assert all(f(**{dim: bad}) == EINVAL for bad in (0, -1, -3, -5)), dim
    for bad in (-0.1, NAN, INF, -INF):
        assert f(cl=bad) == EINVAL and f(ch=bad) == EINVAL, bad
    for bad in (1.0, 0.5, -2.0, NAN, INF):
        assert f(dual=bad) == EINVAL, bad
    for bad in (-1, 3, 17):
        assert f(est=bad) == EINVAL, bad
    assert f(agg=2) == EINVAL and f(agg=-1) == EINVAL
    assert f(kc=NAN) == EINVAL and f(ec=INF) == EINVAL and f(scale=NAN) == EINVAL
    assert f(kc=0.1, ref=None) == EINVAL                                   # a KL term without reference log-probs
    for name in given:
        assert f(**{name: p + 4}) == EALIGN and f(**{name: p + 8}) == EALIGN, name
    # the optional pointers absent and the limits themselves are no refusal: what is left to refuse them is a misaligned pointer
    assert f(old=None, ref=None, rollout=None, lp=p + 4) == EALIGN
    edge = dict(cl=0.0, ch=0.0, dual=1.0000001, kc=0.1, est=0, agg=1, per_seq=1, T=1, S=1)
    assert f(**edge, dlp=p + 4) == EALIGN and f(**edge, c=p + 4) == EALIGN


def test_refusals_of_the_options(env):
    lib, p, _ = env
    f = lambda **kw: _call(lib, p, **kw)
    for bad in (-1, 2):
        assert f(ratio=bad) == EINVAL and f(sur=bad) == EINVAL and f(mode=bad) == EINVAL, bad
    assert f(level=-1) == EINVAL and f(level=4) == EINVAL
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert f(cap=bad) == EINVAL and f(level=1, cap=bad) == EINVAL, bad
    for bad in (-0.1, NAN, INF, 2.0, 3.0):
        assert f(level=1, mode=1, floor=bad) == EINVAL, bad
    assert f(level=1, mode=0, floor=0.5) == EINVAL and f(floor=0.5) == EINVAL                  # a floor goes with "mask" only
    assert f(sur=1, ratio=1) == EINVAL and f(sur=1, dual=3.0) == EINVAL                        # CISPO: no sequence ratio, no dual clip
    for level in (1, 2, 3):
        assert f(level=level, rollout=None) == EINVAL, level                                   # a weight without rollout log-probs
    # the path tables: required where a path is walked - a sequence ratio, a sequence-level weight without old_lp
    for name in PATH:
        assert f(ratio=1, **{name: None}) == EINVAL and f(level=2, old=None, **{name: None}) == EINVAL, name
        assert f(level=3, old=None, **{name: None}) == EINVAL, name
    for dim in ("M", "R"):
        assert f(ratio=1, **{dim: 0}) == EINVAL and f(level=2, old=None, **{dim: -1}) == EINVAL, dim
    # the optional pointers absent and the limits themselves are no refusal: what is left to refuse them is a misaligned pointer
    assert f(old=None, ref=None, rollout=None, lp=p + 4, **NO_TABLES) == EALIGN                # nothing walks a path: no tables
    assert f(level=1, old=None, lp=p + 4, **NO_TABLES) == EALIGN                               # a token weight from the row's own lp
    assert f(level=2, lp=p + 4, **NO_TABLES) == EALIGN and f(level=3, mode=1, floor=0.5, lp=p + 4, **NO_TABLES) == EALIGN
    assert f(sur=1, level=1, lp=p + 4, **NO_TABLES) == EALIGN
    assert f(cl=0.0, ch=0.0, dual=1.0000001, kc=0.1, est=0, agg=1, per_seq=1, T=1, S=1, ratio=1, level=3, mode=1, cap=1e-30, floor=0.0,
             omega=p + 4) == EALIGN


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_the_refusals_come_in_the_header_order(env, flavour):
    lib, p, _ = env
    f = lambda **kw: _call(lib, p, **{**FLAVOURS[flavour], **kw})
    assert f(T=0, lp=p + 4) == EINVAL
    assert f(dual=0.5, ent=p + 4) == EINVAL
    assert f(kc=0.1, ref=None, mask=p + 4) == EINVAL
    assert f(est=5, stats=p + 8) == EINVAL
    assert f(level=7, omega=p + 4) == EINVAL
    assert f(cap=0.0, adv=p + 4) == EINVAL and f(cap=0.0, rollout=p + 4) == EINVAL
    assert f(level=1, rollout=None, c=p + 8) == EINVAL
    assert f(sur=1, dual=3.0, dlp=p + 4) == EINVAL
    if flavour != "token":                                              # the path tables are given: a sequence ratio asks for them
        assert f(ratio=1, R=0, run_row0=p + 4) == EINVAL
        assert f(ratio=1, seq_leaf=None, run_ptr=p + 8) == EINVAL
        # the header: a missing path table or M <= 0 and a bad hyper-parameter are one DTA_EINVAL, whichever is looked at first
        assert f(ratio=1, M=0, dual=0.5) == EINVAL and f(ratio=1, seq_leaf=None, est=5) == EINVAL


def test_the_workspace_rows_follow_the_row_and_sequence_counts(env):
    lib, _, _ = env
    q = lib.dta_policy_loss_blocks
    for s in (1, 5, 2048, 2100):
        assert [q(t, s) - min(s, 2048) for t in (1, 256, 257, 1024 * 256, 1024 * 256 + 1, 1 << 30)] == [1, 1, 2, 1024, 1024, 1024]
    assert [q(t, 1) for t in (1, 256, 257, 1024 * 256, 1024 * 256 + 1, 1 << 30)] == [2, 2, 3, 1025, 1025, 1025]
    assert [q(1, s) for s in (1, 2, 2047, 2048, 2049, 1 << 30)] == [2, 3, 2048, 2049, 2049, 2049]
    assert q(257, 2100) == 2 + 2048
    assert q(0, 1) == EINVAL and q(1, 0) == EINVAL and q(-3, 5) == EINVAL and q(5, -1) == EINVAL and q(-3, 1) == EINVAL
