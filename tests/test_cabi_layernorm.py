"""dta_layernorm_fwd / _bwd refuse every bad argument include/dta.h lists, with the header's status codes, in the header's order and
before any HIP call: host buffers, no GPU (a valid call without a GPU would return DTA_EPRIOR or DTA_ELAUNCH, never one of the three
codes below)."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    from dynamictreeattn_amd import _lib
    raw = ctypes.create_string_buffer(1 << 16)
    return _lib.lib(), (ctypes.addressof(raw) + 63) & ~63, raw


def _fwd(lib, p, R=4, H=64, eps=1e-5, dtype=0, **ptrs):
    a = {n: ptrs.get(n, None if n in ("da", "db", "xo") else p) for n in ("x", "da", "db", "w", "xo", "y", "mean", "rstd")}
    return lib.dta_layernorm_fwd(a["x"], a["da"], a["db"], a["w"], a["xo"], a["y"], a["mean"], a["rstd"], R, H, eps, dtype, None)


def _bwd(lib, p, R=4, H=64, dtype=0, **ptrs):
    a = {n: ptrs.get(n, p) for n in ("x", "w", "dy", "dres", "mean", "rstd", "dx", "part")}
    return lib.dta_layernorm_bwd(a["x"], a["w"], a["dy"], a["dres"], a["mean"], a["rstd"], a["dx"], a["part"], R, H, dtype, None)


def test_forward_refusals(env):
    lib, p, _ = env
    f = lambda **kw: _fwd(lib, p, **kw)
    for name in ("x", "w", "y", "mean", "rstd"):
        assert f(**{name: None}) == EINVAL, name
    assert f(R=0) == EINVAL and f(R=-3) == EINVAL and f(H=0) == EINVAL and f(H=-8) == EINVAL
    assert f(db=p, xo=p) == EINVAL                                       # delta_b without delta_a
    assert f(da=p) == EINVAL and f(da=p, db=p) == EINVAL                 # a delta without x_out
    assert f(xo=p) == EINVAL                                             # x_out without a delta
    assert f(eps=NAN) == EINVAL
    for dt in (3, 7, -1):
        assert f(dtype=dt) == EUNSUPPORTED
    for H in (12, 4, 100, 8200, 8196, 16384):
        assert f(H=H) == EUNSUPPORTED, H
    for dt in (0, 1, 2):                                                 # the limits themselves are no refusal of these kinds
        assert f(H=8192, dtype=dt, x=p + 2) == EALIGN and f(H=8, dtype=dt, x=p + 2) == EALIGN
    for name in ("x", "w", "y"):
        assert f(**{name: p + 2}) == EALIGN and f(**{name: p + 8}) == EALIGN, name
    assert f(da=p + 4, xo=p) == EALIGN and f(da=p, xo=p + 6) == EALIGN and f(da=p, db=p + 8, xo=p) == EALIGN


def test_backward_refusals(env):
    lib, p, _ = env
    b = lambda **kw: _bwd(lib, p, **kw)
    for name in ("x", "w", "dy", "mean", "rstd", "dx"):
        assert b(**{name: None}) == EINVAL, name
    assert b(R=0) == EINVAL and b(H=0) == EINVAL and b(R=-1) == EINVAL
    for dt in (3, -2):
        assert b(dtype=dt) == EUNSUPPORTED
    for H in (12, 8200, 9000):
        assert b(H=H) == EUNSUPPORTED, H
    for name in ("x", "w", "dy", "dx", "dres"):
        assert b(**{name: p + 2}) == EALIGN, name
    # dres NULL and dw_partial NULL are valid forms: what is left to refuse them is the misaligned pointer behind them
    assert b(dres=None, x=p + 2) == EALIGN and b(part=None, dx=p + 4) == EALIGN


def test_the_refusals_come_in_the_header_order(env):
    """DTA_EINVAL (null / sizes / the delta forms / eps) before DTA_EUNSUPPORTED (dtype, H % 8, H > 8192) before DTA_EALIGN."""
    lib, p, _ = env
    assert _fwd(lib, p, R=0, H=12, x=p + 2) == EINVAL
    assert _fwd(lib, p, db=p, xo=p, dtype=7, w=p + 2) == EINVAL
    assert _fwd(lib, p, eps=NAN, H=8200) == EINVAL
    assert _fwd(lib, p, H=8200, x=p + 2) == EUNSUPPORTED
    assert _fwd(lib, p, dtype=7, y=p + 2) == EUNSUPPORTED
    assert _fwd(lib, p, H=12, da=p + 2, xo=p) == EUNSUPPORTED
    assert _bwd(lib, p, dx=None, H=12, x=p + 2) == EINVAL
    assert _bwd(lib, p, H=12, x=p + 2) == EUNSUPPORTED
    assert _bwd(lib, p, H=8200, dy=p + 2) == EUNSUPPORTED


def test_the_workspace_rows_follow_the_row_count(env):
    lib, _, _ = env
    assert [lib.dta_layernorm_bwd_blocks(r) for r in (1, 4, 5, 8192, 8193, 1 << 20)] == [1, 1, 2, 2048, 2048, 2048]
