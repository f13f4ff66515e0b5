"""Containment of the LayerNorm kernels: dta_layernorm_fwd and dta_layernorm_bwd are called through the C ABI on the guarded arenas of
tests/arena.py - at the edges of H (8, a ragged last vector group, 8184, 8192) and R (1, a partial last workgroup), with every optional
pointer given and NULL - and must return 0, leave every guard byte of their outputs and workspaces alone, write every output element,
not depend on memory past an input's extent, and give, bit for bit, what the allocating ops.* wrapper gives for the same inputs (whose
values tests/test_gpu_layernorm.py bounds against float64).  Guards are at least one workgroup's rows (4).  Limits as in tests/arena.py."""
import functools

import pytest
import torch

import arena as A
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
EPS = 1e-5

_in, _out, _same = functools.partial(A.in_arena, device=DEV), functools.partial(A.out_arena, device=DEV), A.assert_matches


def _randn(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _fwd_run(x, da, db, w, disown=None):
    R, H = x.shape

    def run(fill, poison):
        a = {"x": _in("x", x, poison, guard_rows=4), "w": _in("w", w, poison, guard_rows=H)}
        for n, d in (("delta_a", da), ("delta_b", db)):
            if d is not None:
                a[n] = _in(n, d, poison, guard_rows=4)
        if da is not None:
            a["x_out"] = _out("x_out", (R, H), x.dtype, fill, guard_rows=4)
        a["y"] = _out("y", (R, H), x.dtype, fill, guard_rows=4)
        a["mean"] = _out("mean", (R,), F32, fill, guard_rows=64)
        a["rstd"] = _out("rstd", (R,), F32, fill, guard_rows=64)
        if disown:
            a[disown].disown_last_row()
        A.launch("dta_layernorm_fwd", a["x"], a.get("delta_a"), a.get("delta_b"), a["w"], a.get("x_out"), a["y"], a["mean"], a["rstd"], R, H, EPS,
                 ops._DT[x.dtype])
        return a
    return run


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 120, 8184, 8192])
@pytest.mark.parametrize("R", [1, 37])
def test_layernorm_fwd(R, H, dtype):
    x, d1, d2, w = _randn((R, H), dtype, R + H), _randn((R, H), dtype, H + 1), _randn((R, H), dtype, H + 3), _randn((H,), dtype, H + 2)
    for da, db in ((None, None), (d1, None), (d1, d2)):
        label = f"layernorm_fwd R={R} H={H} deltas={(da is not None) + (db is not None)}"
        got = A.check_case(_fwd_run(x, da, db, w), label)
        xa, wa = x.to(DEV).requires_grad_(True), w.to(DEV)
        xo, y = ops.add_layer_norm(xa, None if da is None else da.to(DEV), None if db is None else db.to(DEV), wa, EPS)
        saved = y.grad_fn.saved_tensors
        want = {"y": y.detach(), "mean": saved[2], "rstd": saved[3]}
        if da is not None:
            want["x_out"] = xo.detach()
        _same(got, want, label)


def test_teeth_layernorm_fwd_last_row_told_to_be_a_guard():
    """The entry is called correctly on a [37, 120] output; the helper is told that the extent ends one row earlier.  The kernel's
    stores to row 36 must then be reported: the comparison sees real device stores.  Nothing out of bounds is executed."""
    x, w = _randn((37, 120), BF, 1), _randn((120,), BF, 2)
    with pytest.raises(AssertionError, match="y: 120 guard element.* behind the payload"):
        A.check_case(_fwd_run(x, None, None, w, disown="y"), "teeth")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 120, 8184, 8192])
@pytest.mark.parametrize("R", [1, 37])
def test_layernorm_bwd(R, H, dtype):
    """dw_partial has exactly dta_layernorm_bwd_blocks(R) rows, every one written in full; dw_partial NULL gives the same dx."""
    x, w, dy, dres = (_randn(s, dtype, H + i) for i, s in enumerate(((R, H), (H,), (R, H), (R, H))))
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    xo, y = ops.add_layer_norm(xd, torch.zeros_like(xd), None, wd, EPS)          # (x + 0: the statistics of x)
    mean, rstd = (t.cpu() for t in y.grad_fn.saved_tensors[2:4])
    blocks = lib().dta_layernorm_bwd_blocks(R)
    for with_dres in (True, False):
        for frozen in (False, True):
            label = f"layernorm_bwd R={R} H={H} dres={with_dres} frozen={frozen}"

            def run(fill, poison):
                a = {n: _in(n, t, poison, guard_rows=g) for n, t, g in (("x", x, 4), ("w", w, H), ("dy", dy, 4), ("mean", mean, 64), ("rstd", rstd, 64))}
                if with_dres:
                    a["dres"] = _in("dres", dres, poison, guard_rows=4)
                a["dx"] = _out("dx", (R, H), dtype, fill, guard_rows=4)
                if not frozen:
                    a["dw_partial"] = _out("dw_partial", (blocks, H), F32, fill, guard_rows=1)
                A.launch("dta_layernorm_bwd", a["x"], a["w"], a["dy"], a.get("dres"), a["mean"], a["rstd"], a["dx"], a.get("dw_partial"), R, H,
                         ops._DT[dtype])
                return a
            got = A.check_case(run, label)
            if with_dres:
                dx, dw = torch.autograd.grad([xo, y], [xd, wd], [dres.to(DEV), dy.to(DEV)], retain_graph=True)
                _same(got, {"dx": dx}, label)
            if not frozen:
                if with_dres:
                    A.assert_same_bits(ops.sum_slabs(got["dw_partial"], dtype), dw, label + " dw: the arena's partials against the ops wrapper")
                keep = got["dx"]
            else:
                A.assert_same_bits(got["dx"], keep, label + " dx: dw_partial NULL against given")
