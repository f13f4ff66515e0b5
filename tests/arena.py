"""Guarded arenas: test-owned buffers that show whether a kernel stayed inside the extent it was given.

An arena is ONE flat allocation: a guard band, the payload at a 256-byte-aligned offset (so a kernel takes the code path it takes on a
plain tensor), a guard band behind it.  A payload with a row pitch above its row, or a head stride above head_dim, has its pitch gaps
as guards too: every element of the allocation that the payload view does not cover is a guard.  The bands are sized by the caller to
at least one full tile of the kernel's rows at the payload's pitch, so a stray store of a broken kernel lands inside the allocation,
is seen there, and never reaches memory the test does not own.

* Output / workspace arenas (`out_arena`): payload and guards start as one fill.  Fill "A" is NaN (floats) / 0x7f7f7f7f (ints), fill
  "B" is -3.0 / 0x01010101.  `assert_guards_intact` compares every guard BYTE with what it held before the call (an integer view, not
  isnan: a NaN overwritten by another NaN is seen).  A case runs under both fills; `check_case` wants the payloads bit-identical
  across the runs and, under A, finite: every element was written and nothing was read before it was written.
* Accumulating outputs (`out_arena(..., data=...)`): the payload's initial content is an input; only the guards take the fill.
* Input arenas (`in_arena`): the declared extent holds the data, the guards a poison that differs between two runs - NaN / +inf for
  floats (a masked 0 * v of a stray load gives NaN, or a difference between the runs), and for index tables 0 / the largest VALID index
  of that table: a stray index read must change the result, never the address space, so no guard value may point outside an allocation.

Limits of the method.  A stray load whose value is discarded leaves no trace and is not detected; one that enters arithmetic is, even
under a zero factor.  The guards bound how far a stray store can go and still be caught: one tile of rows.  Nothing here measures time,
and there are no tolerances: every comparison is bitwise (or a caller reuses an existing float64 bound).

Importing this module needs no GPU; tests/test_arena.py runs it on CPU arenas against stand-in kernels with deliberate defects."""
import math

import torch

ALIGN = 256                                   # bytes: the payload's offset in the allocation
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_FILL_INT = {"A": 0x7F, "B": 0x01}            # the byte repeated over the element: 0x7f7f7f7f / 0x01010101 for int32
_FILL_FLOAT = {"A": float("nan"), "B": -3.0}
_POISON_FLOAT = (float("nan"), float("inf"))


def fill_value(dtype, fill):
    """The element an output arena starts with under fill "A" / "B"."""
    if dtype.is_floating_point:
        return _FILL_FLOAT[fill]
    return int.from_bytes(bytes([_FILL_INT[fill]]) * torch.empty(0, dtype=dtype).element_size(), "little")


def _bits(t):
    """The elements of a (possibly strided) tensor as integers of the same size."""
    return t.view(_INT_VIEW[t.element_size()])


class Arena:
    """`view`: the payload, a strided window of shape `shape` / `strides` (elements; default dense) into the flat allocation `flat`.
    guard_rows: rows of the outermost dimension, at its stride, in front of and behind the payload."""

    def __init__(self, label, shape, dtype, guard_fill, *, data=None, strides=None, guard_rows=1, device="cpu"):
        shape = tuple(int(s) for s in shape)
        if strides is None:
            strides = tuple(math.prod(shape[i + 1:]) for i in range(len(shape)))
        strides = tuple(int(s) for s in strides)
        esz = torch.empty(0, dtype=dtype).element_size()
        extent = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if math.prod(shape) else 0
        band = max(int(guard_rows), 1) * max(strides[0] if shape else 1, 1)
        per = ALIGN // esz
        front = (band + per - 1) // per * per                   # whole 256-byte units: the payload keeps the allocation's alignment
        self.flat = torch.full((front + extent + band + per,), guard_fill, dtype=dtype, device=device)
        front += (-self.flat.data_ptr() % ALIGN) // esz         # a host allocation may start off 256 bytes: the slack joins the front band
        self.label, self.dtype, self.front, self.extent, self.guard_fill, self.is_input = label, dtype, front, extent, guard_fill, False
        self.view = self.flat.as_strided(shape, strides, front)
        self.owned = torch.zeros(self.flat.numel(), dtype=torch.bool, device=device)
        self.owned.as_strided(shape, strides, front).fill_(True)
        if data is not None:
            self.view.copy_(data.to(device=device, dtype=dtype))
        self._before = _bits(self.flat).clone()

    def ptr(self):
        return self.view.data_ptr()

    def disown_last_row(self):
        """Declare the extent one row (of the outermost dimension) shorter than the view a kernel is handed: that row counts as guard.
        For the teeth checks - a correct kernel's stores to it must then be reported."""
        self.owned.as_strided(self.view.shape, self.view.stride(), self.front)[-1].fill_(False)
        self.extent -= self.view.stride(0)

    def assert_guards_intact(self, label=""):
        """Every guard byte - front band, back band, pitch gaps - still holds what it held when the arena was built."""
        bad = (_bits(self.flat) != self._before) & ~self.owned
        n = int(bad.sum())
        if n:
            at = torch.nonzero(bad).flatten()
            first, last = int(at[0]) - self.front, int(at[-1]) - self.front
            where = "in front of the payload" if last < 0 else ("behind the payload" if first >= self.extent else
                                                                 "in a pitch gap or a band (offsets relative to the payload start)")
            raise AssertionError(f"{label} {self.label}: {n} guard element(s) changed {where}; first at element {first}, last at {last} "
                                 f"of an extent of {self.extent}")

    def payload(self):
        """A dense copy of the payload."""
        return self.view.clone()


def out_arena(label, shape, dtype, fill, *, data=None, strides=None, guard_rows=1, device="cpu"):
    """An output or workspace arena under fill "A" / "B".  data: the initial payload of an accumulating output (guards alone take the fill)."""
    return Arena(label, shape, dtype, fill_value(dtype, fill), data=data, strides=strides, guard_rows=guard_rows, device=device)


def in_arena(label, data, run, *, hi=None, strides=None, guard_rows=1, device="cpu"):
    """An input arena holding `data`; run 0 / 1 picks the guards' poison.  Floats: NaN / +inf.  Index tables: 0 / `hi`, the largest value
    that is valid wherever the kernel would use an entry of this table (required for integer data)."""
    if data.dtype.is_floating_point:
        poison = _POISON_FLOAT[run]
    else:
        assert hi is not None, f"{label}: an index table needs its largest valid value for the guards"
        poison = (0, int(hi))[run]
    a = Arena(label, data.shape, data.dtype, poison, data=data, strides=strides, guard_rows=guard_rows, device=device)
    a.is_input = True
    return a


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    diff = _bits(a.contiguous()) != _bits(b.contiguous())
    n = int(diff.sum())
    if n:
        i = tuple(int(v) for v in torch.nonzero(diff)[0])
        raise AssertionError(f"{what}: {n} of {diff.numel()} elements differ in their bits; first at {i}: {a[i].item()!r} against {b[i].item()!r}")


def assert_matches(got, want, label, other="the ops wrapper"):
    """Every tensor of `want` bit-equal to the payload of that name in `got` (check_case's result): the arena call against `other`."""
    for name, t in want.items():
        assert_same_bits(got[name], t.reshape(got[name].shape), f"{label} {name}: the arena call against {other}")


def assert_written(t, fill, what):
    """No element of a payload that ran under `fill` may still look unwritten: floats finite (fill A is NaN, and a NaN read before the
    write spreads), integers different from the fill."""
    bad = ~torch.isfinite(t) if t.dtype.is_floating_point else (t == fill_value(t.dtype, fill))
    n = int(bad.sum())
    if n:
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements are {'not finite' if t.dtype.is_floating_point else 'the fill'} under "
                             f"fill {fill} (first at {i}): left unwritten, or computed from memory the call did not define")


def check_case(run, label, scratch=()):
    """run(fill, poison_run) makes the arenas, calls the entry ONCE (asserting its return code) and returns {name: Arena} of every
    output and workspace - and of the inputs (in_arena), whose guards and payload must come back unchanged.  Three calls: (A, poison 0),
    (B, poison 0), (A, poison 1).  Asserts, naming the buffer: every guard intact in every run; payloads bit-identical under fills A and B
    and written (finite) under A; payloads bit-identical under the two input poisons.  `scratch`: names of workspaces whose final content is not a result - their guards are checked, their payload is not.
    Returns {name: payload} of the (A, 0) run."""
    res = {}
    for fill, poison in (("A", 0), ("B", 0), ("A", 1)):
        arenas = run(fill, poison)
        for name, a in arenas.items():
            a.assert_guards_intact(f"{label} [fill {fill}, poison {poison}]")
            if a.is_input:
                assert bool((_bits(a.flat) == a._before).all()), f"{label} {a.label}: an input was written"
        res[fill, poison] = {name: a.payload() for name, a in arenas.items() if name not in scratch and not a.is_input}
    base = res["A", 0]
    for name, t in base.items():
        assert_written(t, "A", f"{label} {name}")
        assert_same_bits(t, res["B", 0][name], f"{label} {name}: fill A against fill B (an element left unwritten, or read before it was written)")
        assert_same_bits(t, res["A", 1][name], f"{label} {name}: input poison NaN/0 against +inf/max (the result depends on memory past an input's extent)")
    return base


def launch(name, *args):
    """One C-ABI call (include/dta.h) on the current stream; an Arena or a tensor stands for its payload's address.  The return code
    must be 0."""
    from dynamictreeattn_amd._lib import lib
    argv = [a.ptr() if isinstance(a, Arena) else a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(lib(), name)(*argv, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"{name} returned {rc}"
