"""tests/arena.py on the CPU: a correct stand-in "kernel" passes every check of the helper, and each of seven deliberate defects is
reported with a message that names the buffer.  The stand-in works on raw (flat storage, offset, pitch) triples the way a kernel works
on a pointer, so that a defect can reach past the extent it was given - inside the arena, as on the device.

The operation: out[r] = 2 * x[idx[r]] + 1 over R rows of W elements, through a workspace row ws[r] = 2 * x[idx[r]]; x has N rows, idx
is an int32 table of R entries; x and out are pitched."""
import pytest
import torch

import arena as A

R, W, N, PITCH = 5, 8, 7, 12


def _raw(a):
    return a.flat, a.front, a.view.stride(0)


def _kernel(x, idx, ws, out, defect=None):
    (xf, x0, xp), (tf, t0, _), (wf, w0, wp), (of, o0, op) = _raw(x), _raw(idx), _raw(ws), _raw(out)
    for r in range(R):
        src = int(tf[t0 + r])
        wf[w0 + r * wp:w0 + r * wp + W] = 2 * xf[x0 + src * xp:x0 + src * xp + W]
    for r in range(R):
        row = wf[w0 + r * wp:w0 + r * wp + W] + 1
        if defect == "unwritten workspace row" and r == R - 1:
            row = row + wf[w0 + R * wp:w0 + R * wp + W]                     # a slab nobody wrote
        if defect == "masked load past the input" and r == R - 1:
            row = row + 0.0 * xf[x0 + N * xp:x0 + N * xp + W]              # row N of x, times zero
        if defect == "index read too far" and r == R - 1:
            row = row + xf[x0 + int(tf[t0 + R]) * xp:x0 + int(tf[t0 + R]) * xp + W]
        of[o0 + r * op:o0 + r * op + W] = row
    if defect == "store past the tail":
        of[o0 + (R - 1) * op + W] = 1.0
    if defect == "store into a pitch gap":
        of[o0 + W] = 1.0
    if defect == "store in front":
        of[o0 - 1] = 1.0
    if defect == "element unwritten":
        of[o0 + 2 * op + 3] = out.guard_fill


def _run(defect, dtype, unwritten_ws_rows=0):
    x = torch.randn(N, W, generator=torch.Generator().manual_seed(1)).to(dtype)
    idx = torch.randint(0, N, (R,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)

    def run(fill, poison):
        xa = A.in_arena("x", x, poison, strides=(PITCH, 1), guard_rows=2)
        ia = A.in_arena("idx", idx, poison, hi=N - 1)
        ws = A.out_arena("ws", (R + unwritten_ws_rows, W), dtype, fill, guard_rows=2)
        out = A.out_arena("out", (R, W), dtype, fill, strides=(PITCH, 1), guard_rows=2)
        _kernel(xa, ia, ws, out, defect)
        xa.assert_guards_intact("stand-in"); ia.assert_guards_intact("stand-in")
        return {"ws": ws, "out": out}
    return A.check_case(run, "stand-in", scratch=("ws",) if unwritten_ws_rows else ())["out"], x, idx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_a_correct_stand_in_passes(dtype):
    out, x, idx = _run(None, dtype)
    assert torch.equal(out, 2 * x[idx.long()] + 1)


DEFECTS = [("store past the tail", "stand-in .* out: 1 guard element.* changed behind the payload", 0),
           ("store into a pitch gap", "stand-in .* out: 1 guard element.* changed in a pitch gap", 0),
           ("store in front", "stand-in .* out: 1 guard element.* changed in front of the payload", 0),
           ("element unwritten", "stand-in out: 1 of 40 elements", 0),
           ("unwritten workspace row", "stand-in out: 8 of 40 elements are not finite", 1),
           ("masked load past the input", "stand-in out: 8 of 40 elements are not finite", 0),
           ("index read too far", "stand-in out: input poison NaN/0 against \\+inf/max", 0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("defect,message,ws_rows", DEFECTS)
def test_deliberate_defects_are_reported_by_buffer(defect, message, ws_rows, dtype):
    with pytest.raises(AssertionError, match=message):
        _run(defect, dtype, ws_rows)


def test_an_unwritten_element_under_a_finite_fill_is_a_difference_between_the_fills():
    """Fill B alone does not show an unwritten element; the pair of runs does."""
    a, b = A.out_arena("o", (4,), torch.float32, "A"), A.out_arena("o", (4,), torch.float32, "B")
    for t in (a, b):
        t.view[:3] = 1.0
    with pytest.raises(AssertionError, match="fill A against fill B"):
        A.assert_same_bits(a.payload(), b.payload(), "o: fill A against fill B")


def test_a_nan_over_a_nan_guard_is_seen():
    """The guard comparison is bytewise: another NaN's bits over the fill's NaN are a change."""
    a = A.out_arena("o", (4,), torch.float32, "A")
    a.flat.view(torch.int32)[a.front + 4] = 0x7FC00001
    assert bool(torch.isnan(a.flat).all())
    with pytest.raises(AssertionError, match="o: 1 guard element.* behind the payload"):
        a.assert_guards_intact()


def test_integer_arenas_and_a_disowned_row():
    a = A.out_arena("tiles", (6,), torch.int32, "A")
    assert int(a.flat[0]) == 0x7F7F7F7F and a.ptr() % A.ALIGN == 0
    b = A.out_arena("tiles", (6,), torch.int32, "B")
    assert int(b.flat[0]) == 0x01010101
    i = A.in_arena("ids", torch.arange(6, dtype=torch.int64), 1, hi=5)
    assert int(i.flat[0]) == 5 and int(i.flat[-1]) == 5 and torch.equal(i.view, torch.arange(6))
    o = A.out_arena("y", (3, 4), torch.float32, "A")
    o.disown_last_row()
    o.view.copy_(torch.ones(3, 4))                                         # a correct store to what the helper was told is a guard
    with pytest.raises(AssertionError, match="y: 4 guard element.* behind the payload"):
        o.assert_guards_intact()
