"""dta_rope_partial_fwd / _bwd refuse every bad argument include/dta.h lists, with the header's status codes and before any HIP call:
host buffers, no GPU (a valid call without a GPU would return DTA_EPRIOR or DTA_ELAUNCH, never one of the three codes below)."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def env():
    from dynamictreeattn_amd import _lib
    raw = ctypes.create_string_buffer(1 << 16)
    return _lib.lib(), (ctypes.addressof(raw) + 63) & ~63, raw


def _fwd(lib, p, x=None, cs=None, y=None, T=4, NH=3, D=128, rot=96, pairing=0, st=3 * 128, dtype=0):
    a = {"x": p if x is None else x, "cs": p if cs is None else cs, "y": p if y is None else y}
    return lib.dta_rope_partial_fwd(a["x"], a["cs"], a["y"], T, NH, D, rot, pairing, st, dtype, None)


def _bwd(lib, p, cs=None, dy=None, dx=None, T=4, NH=3, D=128, rot=96, pairing=0, st_t=3 * 128, st_h=128, dx_st=3 * 128, dtype=0):
    a = {"cs": p if cs is None else cs, "dy": p if dy is None else dy, "dx": p if dx is None else dx}
    return lib.dta_rope_partial_bwd(a["cs"], a["dy"], a["dx"], T, NH, D, rot, pairing, st_t, st_h, dx_st, dtype, None)


def test_forward_refusals(env):
    lib, p, _ = env
    f = lambda **kw: _fwd(lib, p, **kw)
    assert lib.dta_rope_partial_fwd(None, p, p, 4, 3, 128, 96, 0, 384, 0, None) == EINVAL
    assert lib.dta_rope_partial_fwd(p, None, p, 4, 3, 128, 96, 0, 384, 0, None) == EINVAL
    assert lib.dta_rope_partial_fwd(p, p, None, 4, 3, 128, 96, 0, 384, 0, None) == EINVAL
    assert f(T=0) == EINVAL and f(T=-1) == EINVAL and f(NH=0) == EINVAL
    assert f(rot=0) == EINVAL and f(rot=-16) == EINVAL
    assert f(pairing=2) == EINVAL and f(pairing=-1) == EINVAL
    for dt in (3, 7, -1):
        assert f(dtype=dt) == EUNSUPPORTED
    for D in (32, 96, 256, 0):
        assert f(D=D, rot=32, st=3 * max(D, 8)) == EUNSUPPORTED, D
    assert f(rot=144) == EUNSUPPORTED and f(D=64, rot=80, st=192) == EUNSUPPORTED                  # R > D
    for rot in (8, 24, 40, 104, 120):                                                              # half-split: R % 16
        assert f(rot=rot) == EUNSUPPORTED, rot
    for rot in (4, 12, 60, 100):                                                                   # interleaved: R % 8
        assert f(rot=rot, pairing=1) == EUNSUPPORTED, rot
    assert f(x=p + 2) == EALIGN and f(y=p + 8) == EALIGN and f(cs=p + 4) == EALIGN
    assert f(st=3 * 128 + 4) == EALIGN
    assert f(st=-8) == EINVAL


def test_backward_refusals(env):
    lib, p, _ = env
    b = lambda **kw: _bwd(lib, p, **kw)
    assert lib.dta_rope_partial_bwd(None, p, p, 4, 3, 128, 96, 0, 384, 128, 384, 0, None) == EINVAL
    assert lib.dta_rope_partial_bwd(p, None, p, 4, 3, 128, 96, 0, 384, 128, 384, 0, None) == EINVAL
    assert lib.dta_rope_partial_bwd(p, p, None, 4, 3, 128, 96, 0, 384, 128, 384, 0, None) == EINVAL
    assert b(T=0) == EINVAL and b(NH=-2) == EINVAL and b(rot=0) == EINVAL and b(pairing=3) == EINVAL
    assert b(dtype=5) == EUNSUPPORTED
    assert b(D=96, rot=48, st_h=96, st_t=288, dx_st=288) == EUNSUPPORTED
    assert b(rot=136) == EUNSUPPORTED and b(rot=88) == EUNSUPPORTED and b(rot=92, pairing=1) == EUNSUPPORTED
    assert b(dy=p + 2) == EALIGN and b(dx=p + 6) == EALIGN and b(cs=p + 8) == EALIGN
    assert b(st_t=388) == EALIGN and b(st_h=132) == EALIGN and b(dx_st=390) == EALIGN
    assert b(dx_st=2 * 128) == EINVAL                                                              # dx token stride below NH * D
    assert b(st_h=64) == EINVAL                                                                    # dy head stride below D
    assert b(st_t=-384) == EINVAL


def test_the_refusals_come_in_the_header_order(env):
    """DTA_EINVAL (null / sizes / pairing) before DTA_EUNSUPPORTED (dtype, head_dim, R) before DTA_EALIGN before the stride DTA_EINVAL."""
    lib, p, _ = env
    assert _fwd(lib, p, T=0, dtype=7, x=p + 2) == EINVAL
    assert _fwd(lib, p, dtype=7, x=p + 2) == EUNSUPPORTED
    assert _fwd(lib, p, rot=24, x=p + 2) == EUNSUPPORTED
    assert _bwd(lib, p, dy=p + 2, dx_st=128) == EALIGN
