"""Containment of the row kernels (rmsnorm, rmsnorm-add, q/k norm + RoPE, SwiGLU / GeGLU, transpose, sum_slabs): every entry is called
through the C ABI on guarded arenas (tests/arena.py) and must return 0, leave every guard byte of its outputs and workspaces alone,
write every output element (bit-identical payloads under the NaN and the -3.0 fill, finite under NaN), not depend on memory past an
input's extent (bit-identical under NaN and +inf poison around the inputs) and give, bit for bit, what the allocating ops.* wrapper
gives for the same inputs - whose values tests/test_gpu_rowops_bounds.py and test_gpu_rowops_gemma.py bound against float64.

Guards are at least one workgroup's rows: 4 rows for the RMSNorm kernels, 32 (token, head) units for the q/k kernels, 64 rows for the
transpose, 2048 elements for the GLUs, 4096 for sum_slabs.

Limits (tests/arena.py): a stray load whose value is discarded is not seen; a stray store further than the guard band is not caught;
no time is measured and no tolerance is used - every comparison is bitwise."""
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
EPS = 1e-6


_in, _out, _same = functools.partial(A.in_arena, device=DEV), functools.partial(A.out_arena, device=DEV), A.assert_matches


def _randn(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# ------------------------------------------------------------------------------------------------ RMSNorm
def _rms_fwd_run(x, delta, w, off, disown=None):
    R, H = x.shape

    def run(fill, poison):
        a = {"x": _in("x", x, poison, guard_rows=4), "w": _in("w", w, poison, guard_rows=H)}
        if delta is not None:
            a["delta"] = _in("delta", delta, poison, guard_rows=4)
            a["x_out"] = _out("x_out", (R, H), x.dtype, fill, guard_rows=4)
        a["y"] = _out("y", (R, H), x.dtype, fill, guard_rows=4)
        a["rstd"] = _out("rstd", (R,), F32, fill, guard_rows=64)
        if disown:
            a[disown].disown_last_row()
        A.launch("dta_rmsnorm_fwd", a["x"], a.get("delta"), a["w"], a.get("x_out"), a["y"], a["rstd"], R, H, EPS, off, ops._DT[x.dtype])
        return a
    return run


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 72, 2056, 8200])
@pytest.mark.parametrize("R", [1, 37])
def test_rmsnorm_fwd(R, H, dtype):
    x, d, w = _randn((R, H), dtype, R + H), _randn((R, H), dtype, H + 1), _randn((H,), dtype, H + 2)
    for delta in (None, d):
        for off in (0.0, 1.0):
            label = f"rmsnorm_fwd R={R} H={H} delta={delta is not None} w_offset={off}"
            got = A.check_case(_rms_fwd_run(x, delta, w, off), label)
            xa, wa = x.to(DEV).requires_grad_(True), w.to(DEV)
            xo, y = ops.add_rms_norm(xa, None if delta is None else delta.to(DEV), wa, EPS, off)
            want = {"y": y.detach(), "rstd": y.grad_fn.saved_tensors[2]}
            if delta is not None:
                want["x_out"] = xo.detach()
            _same(got, want, label)


def test_teeth_rmsnorm_fwd_last_row_told_to_be_a_guard():
    """The entry is called correctly on a [37, 72] output; the helper is told that the extent ends one row earlier.  The kernel's
    stores to row 36 must then be reported: the comparison sees real device stores.  Nothing out of bounds is executed."""
    x, w = _randn((37, 72), BF, 1), _randn((72,), BF, 2)
    with pytest.raises(AssertionError, match="y: 72 guard element.* behind the payload"):
        A.check_case(_rms_fwd_run(x, None, w, 0.0, disown="y"), "teeth")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 72, 2056, 8192])
@pytest.mark.parametrize("R", [1, 37])
def test_rmsnorm_bwd(R, H, dtype):
    """dw_partial has exactly dta_rmsnorm_bwd_blocks(R) rows, every one written in full; dw_partial NULL gives the same dx."""
    x, w, dy, dres = (_randn(s, dtype, H + i) for i, s in enumerate(((R, H), (H,), (R, H), (R, H))))
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    xo, y = ops._RMSNorm.apply(xd, torch.zeros_like(xd), wd, EPS, 0.0)
    rstd = y.grad_fn.saved_tensors[2].cpu()
    blocks = lib().dta_rmsnorm_bwd_blocks(R)
    for with_dres in (True, False):
        for frozen in (False, True):
            label = f"rmsnorm_bwd R={R} H={H} dres={with_dres} frozen={frozen}"

            def run(fill, poison):
                a = {n: _in(n, t, poison, guard_rows=g) for n, t, g in (("x", x, 4), ("w", w, H), ("dy", dy, 4), ("rstd", rstd, 64))}
                if with_dres:
                    a["dres"] = _in("dres", dres, poison, guard_rows=4)
                a["dx"] = _out("dx", (R, H), dtype, fill, guard_rows=4)
                if not frozen:
                    a["dw_partial"] = _out("dw_partial", (blocks, H), F32, fill, guard_rows=1)
                A.launch("dta_rmsnorm_bwd", a["x"], a["w"], a["dy"], a.get("dres"), a["rstd"], a["dx"], a.get("dw_partial"), R, H, 0.0, ops._DT[dtype])
                return a
            got = A.check_case(run, label)
            g_res = dres.to(DEV) if with_dres else torch.zeros(R, H, dtype=dtype, device=DEV)
            dx, dw = torch.autograd.grad([xo, y], [xd, wd], [g_res, dy.to(DEV)], retain_graph=True)
            if with_dres:                       # the wrapper always hands the kernel a dres (zeros when no gradient arrives on the stream)
                _same(got, {"dx": dx}, label)
            else:
                A.assert_same_bits(got["dx"], dx, label + " dx: dres NULL against a dres of zeros through the ops wrapper")
            if not frozen:
                A.assert_same_bits(ops.sum_slabs(got["dw_partial"], dtype), dw, label + " dw: the arena's partials against the ops wrapper")
                keep = got["dx"]
            else:
                A.assert_same_bits(got["dx"], keep, label + " dx: dw_partial NULL against given")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 72, 2056, 8200])
@pytest.mark.parametrize("R", [1, 37])
def test_rmsnorm_add_fwd(R, H, dtype):
    y, res, w = _randn((R, H), dtype, R + H), _randn((R, H), dtype, H + 1), _randn((H,), dtype, H + 2)
    ya = y.to(DEV).requires_grad_(True)
    o = ops.rms_norm_add(res.to(DEV), ya, w.to(DEV), EPS)
    want = {"out": o.detach(), "rstd": o.grad_fn.saved_tensors[2]}
    for want_yn in (True, False):
        label = f"rmsnorm_add_fwd R={R} H={H} yn={want_yn}"

        def run(fill, poison):
            a = {"y": _in("y", y, poison, guard_rows=4), "res": _in("res", res, poison, guard_rows=4), "w": _in("w", w, poison, guard_rows=H),
                 "out": _out("out", (R, H), dtype, fill, guard_rows=4), "rstd": _out("rstd", (R,), F32, fill, guard_rows=64)}
            if want_yn:
                a["yn"] = _out("yn", (R, H), dtype, fill, guard_rows=4)
            A.launch("dta_rmsnorm_add_fwd", a["y"], a["w"], a["res"], a["out"], a.get("yn"), a["rstd"], R, H, EPS, ops._DT[dtype])
            return a
        _same(A.check_case(run, label), want, label)


# ------------------------------------------------------------------------------------------------ q/k head norm + RoPE
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("NH", [1, 3])
def test_qk_norm_rope(NH, D, dtype):
    """x read in place from a fused [T, NH+2, D] buffer (the two spare heads of every token are poison); dy with token and head strides
    above the minimum; dx out of place at a token stride above NH*D, and in place over dy; partials of exactly
    dta_qk_norm_rope_bwd_blocks(T*NH) rows; with the head-norm weight and without (RoPE only)."""
    T, H3 = 33, NH + 2
    xs, w, dy = _randn((T, NH, D), dtype, NH + D), _randn((D,), dtype, 3), _randn((T, NH, D), dtype, 4)
    depth = torch.randint(0, 4096, (T,), generator=torch.Generator().manual_seed(5)).to(DEV)
    cs = ops.rope_cos_sin(depth, D, 1e4).cpu()
    fused = (H3 * D, D, 1)
    units = 32                                  # (token, head) units of one workgroup at most: the guard rows, in tokens
    blocks = lib().dta_qk_norm_rope_bwd_blocks(T * NH)
    for has_w in (True, False):
        label = f"qk_norm_rope T={T} NH={NH} D={D} w={has_w}"

        def fwd(fill, poison):
            a = {"x": _in("x", xs, poison, strides=fused, guard_rows=units), "cos_sin": _in("cos_sin", cs, poison, guard_rows=units),
                 "y": _out("y", (T, NH, D), dtype, fill, guard_rows=units)}
            if has_w:
                a["w"] = _in("w", w, poison, guard_rows=D)
                a["rstd"] = _out("rstd", (T * NH,), F32, fill, guard_rows=64)
            A.launch("dta_qk_norm_rope_fwd", a["x"], a.get("w"), a["cos_sin"], a["y"], a.get("rstd"), T, NH, D, fused[0], EPS, ops._DT[dtype])
            return a
        got = A.check_case(fwd, label + " fwd")
        xd = torch.zeros(T, H3, D, dtype=dtype, device=DEV)
        xd[:, :NH] = xs.to(DEV)
        wd = w.to(DEV) if has_w else None
        y, rstd = ops._qk_norm_rope_fwd(xd[:, :NH], wd, cs.to(DEV), EPS)
        _same(got, {"y": y, "rstd": rstd} if has_w else {"y": y}, label + " fwd")
        dxw = torch.empty(T, NH, D, dtype=dtype, device=DEV)
        dww = ops._qk_norm_rope_bwd(xd[:, :NH], wd, cs.to(DEV), dy.to(DEV), rstd, dxw, True)
        rstd_h = rstd.cpu() if has_w else None
        for in_place in (False, True):
            for frozen in ((False, True) if has_w else (True,)):
                lb = f"{label} bwd in_place={in_place} frozen={frozen}"

                def bwd(fill, poison):
                    a = {"cos_sin": _in("cos_sin", cs, poison, guard_rows=units)}
                    if has_w:
                        a.update(x=_in("x", xs, poison, strides=fused, guard_rows=units), w=_in("w", w, poison, guard_rows=D),
                                 rstd=_in("rstd", rstd_h, poison, guard_rows=64))
                    if in_place:               # dx is dy: one buffer at the fused pitch, its initial content the incoming gradient
                        a["dx"] = _out("dx", (T, NH, D), dtype, fill, data=dy, strides=fused, guard_rows=units)
                        dyp, dys = a["dx"], fused
                    else:
                        dys = ((NH + 1) * (D + 8), D + 8, 1)
                        a["dy"] = dyp = _in("dy", dy, poison, strides=dys, guard_rows=units)
                        a["dx"] = _out("dx", (T, NH, D), dtype, fill, strides=fused, guard_rows=units)
                    if has_w and not frozen:
                        a["dw_partial"] = _out("dw_partial", (blocks, D), F32, fill, guard_rows=16)
                    A.launch("dta_qk_norm_rope_bwd", a.get("x"), a.get("w"), a["cos_sin"], dyp, a.get("rstd"), a["dx"], a.get("dw_partial"),
                             T, NH, D, fused[0], dys[0], dys[1], fused[0], ops._DT[dtype])
                    return a
                got = A.check_case(bwd, lb)
                _same(got, {"dx": dxw}, lb)
                if "dw_partial" in got:
                    A.assert_same_bits(ops.sum_slabs(got["dw_partial"], dtype), dww, lb + " dw: the arena's partials against the ops wrapper")


# ------------------------------------------------------------------------------------------------ SwiGLU / GeGLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [8, 72])
@pytest.mark.parametrize("kernel", ["swiglu", "geglu"])
def test_glu(kernel, cols, dtype):
    """gate | up are the halves of one fused [3, 2*cols] buffer (ld = 2*cols); the gradients go to one fused buffer (ld_grad = 2*cols)
    and to two dense ones (ld_grad = cols)."""
    rows = 3
    gu, dy = _randn((rows, 2 * cols), dtype, cols), _randn((rows, cols), dtype, cols + 1)
    g = -(-2048 // cols)                       # one workgroup takes 256 x 8 elements: that many rows of guard
    esz = gu.element_size()
    gud = gu.to(DEV).requires_grad_(True)
    y = getattr(ops, kernel + "_fused")(gud)
    (dgu,) = torch.autograd.grad(y, [gud], dy.to(DEV))
    label = f"{kernel} cols={cols}"

    def fwd(fill, poison):
        a = {"gu": _in("gu", gu, poison, guard_rows=g), "y": _out("y", (rows, cols), dtype, fill, guard_rows=g)}
        A.launch(f"dta_{kernel}_fwd", a["gu"].ptr(), a["gu"].ptr() + cols * esz, a["y"], rows, cols, 2 * cols, ops._DT[dtype])
        return a
    _same(A.check_case(fwd, label + " fwd"), {"y": y.detach()}, label + " fwd")
    for fused_grad in (True, False):
        lb = f"{label} bwd ld_grad={'2*cols' if fused_grad else 'cols'}"

        def bwd(fill, poison):
            a = {"gu": _in("gu", gu, poison, guard_rows=g), "dy": _in("dy", dy, poison, guard_rows=g)}
            if fused_grad:
                a["dgu"] = _out("dgu", (rows, 2 * cols), dtype, fill, guard_rows=g)
                dg, du, ldg = a["dgu"].ptr(), a["dgu"].ptr() + cols * esz, 2 * cols
            else:
                a["dgate"], a["dup"] = (_out(n, (rows, cols), dtype, fill, guard_rows=g) for n in ("dgate", "dup"))
                dg, du, ldg = a["dgate"], a["dup"], cols
            A.launch(f"dta_{kernel}_bwd", a["gu"].ptr(), a["gu"].ptr() + cols * esz, a["dy"], dg, du, rows, cols, 2 * cols, ldg, ops._DT[dtype])
            return a
        got = A.check_case(bwd, lb)
        _same(got, {"dgu": dgu} if fused_grad else {"dgate": dgu[:, :cols].contiguous(), "dup": dgu[:, cols:].contiguous()}, lb)


# ------------------------------------------------------------------------------------------------ transpose, sum_slabs
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("rows,cols", [(8, 8), (200, 72)])
def test_transpose(rows, cols, dtype):
    """ld_in and ld_out 8 elements above the minimum, at 2-byte and 4-byte elements: the pitch gaps are guards on both sides."""
    x = _randn((rows, cols), dtype, rows)
    ld_in, ld_out = cols + 8, rows + 8
    label = f"transpose {rows}x{cols} {dtype}"

    def run(fill, poison):
        a = {"in": _in("in", x, poison, strides=(ld_in, 1), guard_rows=64), "out": _out("out", (cols, rows), dtype, fill, strides=(ld_out, 1), guard_rows=64)}
        A.launch("dta_transpose", a["in"], a["out"], rows, cols, ld_in, ld_out, x.element_size())
        return a
    got = A.check_case(run, label)
    _same(got, {"out": ops.transpose_2d(x.to(DEV))}, label)
    assert torch.equal(got["out"].cpu(), x.t())


@pytest.mark.parametrize("out_dtype", DTYPES)
@pytest.mark.parametrize("n,slabs,stride", [(8, 1, 16), (1028, 16, 1040), (1029, 17, 1031)])
def test_sum_slabs(n, slabs, stride, out_dtype):
    """slab_stride above n (the gap behind every slab is poison), with and without `extra`.  (8, 1) and (1028, 16) take the vector form
    at the pitched stride as at the dense one, (1029, 17) the scalar form both times: the dense result of ops.sum_slabs is the same
    sum in the same order, so the comparison is bitwise."""
    part, extra = _randn((slabs, n), F32, n), _randn((n,), F32, n + 1)
    for with_extra in (False, True):
        label = f"sum_slabs n={n} slabs={slabs} extra={with_extra} {out_dtype}"

        def run(fill, poison):
            a = {"part": _in("part", part, poison, strides=(stride, 1), guard_rows=4), "out": _out("out", (n,), out_dtype, fill, guard_rows=4096)}
            if with_extra:
                a["extra"] = _in("extra", extra, poison, guard_rows=4096)
            A.launch("dta_sum_slabs", a["part"], slabs, n, stride, a.get("extra"), a["out"], ops._DT[out_dtype])
            return a
        _same(A.check_case(run, label), {"out": ops.sum_slabs(part.to(DEV), out_dtype, extra.to(DEV) if with_extra else None)}, label)
