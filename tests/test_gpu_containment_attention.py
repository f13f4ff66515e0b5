"""Containment of the tree-attention kernels (dta_tree_attn_fwd / dta_tree_attn_bwd: the MFMA kernels in bf16 / f16, the fp32 kernels),
called through the C ABI on guarded arenas (tests/arena.py) in the layouts the product uses:

* packed tries - q, k and v read in place from ONE fused [T, Hq+2Hkv+1, D] arena whose spare head slot is poison; out, and dq | dk | dv
  side by side, written into such fused arenas whose spare slot is a guard (_TreeAttention.backward's buffer);
* the stack form - K / V are the first start+B rows of a taller stack arena whose remaining rows are poison (_StackAttention's
  kst[:end]); dk / dv accumulate into the first start+B rows of such a stack, whose rows from Tk on must keep their bits;
* lse and delta [Hq, Tq] arenas; under forced splits a dkv_ws arena of exactly n_slabs slabs; every plan table (subtree_end, run_ptr,
  runs, ktile_qend, win_lo, dkv_units, dkv_splits) an index arena whose guards hold 0 / the table's largest valid value.

Each case must return 0, leave every guard byte of its outputs and workspaces alone, give bit-identical payloads under the NaN and the
-3.0 fill (finite under NaN: every element written, none read first; for accumulate 1 / 2 the random initial dk / dv are an input and
the guards alone take the fill), bit-identical payloads under NaN and +inf poison around the inputs, and - in the dense layout - the
bits ops.attn_fwd_raw / ops.attn_bwd_raw return for the same inputs, whose values the attention suites bound against float64.  The
backward runs as which = 3 and as 1, then 2|8, then 4; with the plan's units and with every key tile forced into split units
(packing.plan_dkv_units(..., n_cu=1 << 20, min_tiles=1); the fp32 path takes no units, as in ops.attn_bwd_raw); accumulate 0, 1, 2.
dkv_ws is scratch: its guards are checked and its content is not a result (rows of a slab past Tk are never read).

Guards: 128 rows (DTA_QTILE = DTA_KTILE) at the payload's pitch; 128 floats around lse / delta; one slab around dkv_ws.
Limits (tests/arena.py): a stray load whose value is discarded is not seen; a stray store further than the guard band is not caught;
no time is measured and no tolerance is used - every comparison is bitwise."""
import dataclasses

import numpy as np
import pytest
import torch

import arena as A
import test_gpu_attention_window as W
from dynamictreeattn_amd import ops, packing

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
FORMS = {"plain": (0, 0.0), "window": (64, 0.0), "softcap": (0, 5.0), "window_softcap": (64, 5.0)}      # each its own instantiation
TILE = 128


def _fork(T):
    """A prefix of T // 3 tokens and two branches, T packed tokens in all (the other suites' _prefix_trie packs 449 whatever its
    prefix; these cases need 63, 129 and 191)."""
    P = T // 3
    a = (T - P) // 2
    pre = list(range(1000, 1000 + P))
    return [pre + [1] + [5] * (a - 1), pre + [2] + [6] * (T - P - a - 1)]


def _host(t):
    return None if t is None else t.cpu()


class _Case:
    """One attention problem: dense host tensors, the plan tables on the host, and the arenas of one run."""

    def __init__(self, label, q, k, v, do, meta, Hkv, cap, stack):
        self.label, self.meta, self.cap, self.stack = label, meta, cap, stack
        self.q, self.k, self.v, self.do = (_host(t) for t in (q, k, v, do))
        (self.Tq, self.Hq, self.D), self.Tk, self.Hkv, self.dtype = q.shape, k.shape[0], Hkv, q.dtype
        self.scale = self.D ** -0.5
        nkt = -(-self.Tk // TILE)
        end = meta.q_offset + self.Tq
        nruns = 0 if meta.runs is None else meta.runs.shape[0]
        units = None if self.dtype == F32 else meta.dkv_units               # the fp32 kernels take no units
        self.splits = None if units is None else meta.dkv_splits
        self.n_slabs = meta.n_slabs if self.splits is not None else 0
        # (host table, largest value that is valid wherever an entry of the table is used)
        self.tables = {"subtree_end": (_host(meta.subtree_end), end), "run_ptr": (_host(meta.run_ptr), nruns), "runs": (_host(meta.runs), self.Tk),
                       "ktile_qend": (_host(meta.ktile_qend), end), "win_lo": (_host(meta.win_lo) if meta.window > 0 else None, self.Tk - 1),
                       "dkv_units": (_host(units), max(0, min(nkt, self.n_slabs) - 1)),
                       "dkv_splits": (_host(self.splits), min(nkt - 1, self.n_slabs // 2))}

    def inputs(self, poison, bwd):
        Hq, Hkv, D = self.Hq, self.Hkv, self.D
        a = {n: A.in_arena(n, t, poison, hi=hi, guard_rows=64, device=DEV) for n, (t, hi) in self.tables.items()
             if t is not None and (bwd or n not in ("ktile_qend", "dkv_units", "dkv_splits"))}
        if self.stack:
            a["q"] = A.in_arena("q", self.q, poison, strides=((Hq + 1) * D, D, 1), guard_rows=TILE, device=DEV)
            a["kv"] = A.in_arena("kv", torch.cat([self.k, self.v], 1), poison, strides=((2 * Hkv + 1) * D, D, 1), guard_rows=TILE, device=DEV)
            self.ptrs = (a["q"].ptr(), a["kv"].ptr(), a["kv"].ptr() + Hkv * D * self.q.element_size())
            self.strides = ((Hq + 1) * D, D) + ((2 * Hkv + 1) * D, D) * 2
        else:
            H4 = Hq + 2 * Hkv + 1
            a["qkv"] = A.in_arena("qkv", torch.cat([self.q, self.k, self.v], 1), poison, strides=(H4 * D, D, 1), guard_rows=TILE, device=DEV)
            p, e = a["qkv"].ptr(), D * self.q.element_size()
            self.ptrs = (p, p + Hq * e, p + (Hq + Hkv) * e)
            self.strides = (H4 * D, D) * 3
        return a

    def tail(self, a):
        return (a.get("win_lo"), int(self.meta.window), float(self.cap))

    def fwd(self, disown=None):
        Tq, Hq, D = self.Tq, self.Hq, self.D

        def run(fill, poison):
            a = self.inputs(poison, False)
            a["out"] = A.out_arena("out", (Tq, Hq, D), self.dtype, fill, strides=((Hq + 1) * D, D, 1), guard_rows=TILE, device=DEV)
            a["lse"] = A.out_arena("lse", (Hq, Tq), F32, fill, guard_rows=-(-TILE // Tq), device=DEV)
            if disown:
                a[disown].disown_last_row()
            A.launch("dta_tree_attn_fwd", *self.ptrs, a["out"], a["lse"], a.get("subtree_end"), a.get("run_ptr"), a.get("runs"),
                     Tq, self.Tk, self.meta.q_offset, Hq, self.Hkv, D, *self.strides, (Hq + 1) * D, D, self.scale, ops._DT[self.dtype], *self.tail(a))
            return a
        return run

    def bwd(self, out, lse, accumulate, whiches, base):
        """base: the initial (dk | dv) [Tk, 2*Hkv, D] of an accumulating call (host), else None."""
        Tq, Tk, Hq, Hkv, D, dt = self.Tq, self.Tk, self.Hq, self.Hkv, self.D, self.dtype
        out, lse = _host(out), _host(lse)
        fused = not self.stack and accumulate == 0 and Tq == Tk

        def run(fill, poison):
            a = self.inputs(poison, True)
            for n, t in (("out", out), ("dout", self.do)):
                a[n] = A.in_arena(n, t, poison, strides=((Hq + 1) * D, D, 1), guard_rows=TILE, device=DEV)
            a["lse"] = A.in_arena("lse", lse, poison, guard_rows=-(-TILE // Tq), device=DEV)
            a["delta"] = A.out_arena("delta", (Hq, Tq), F32, fill, guard_rows=-(-TILE // Tq), device=DEV)
            e = D * (4 if accumulate == 2 else self.q.element_size())
            if fused:
                H4 = Hq + 2 * Hkv + 1
                a["dqkv"] = A.out_arena("dqkv", (Tq, H4 - 1, D), dt, fill, strides=(H4 * D, D, 1), guard_rows=TILE, device=DEV)
                p = a["dqkv"].ptr()
                grads, gst = (p, p + Hq * e, p + (Hq + Hkv) * e), (H4 * D, D) * 2
            else:
                a["dq"] = A.out_arena("dq", (Tq, Hq, D), dt, fill, strides=((Hq + 1) * D, D, 1), guard_rows=TILE, device=DEV)
                a["dkv"] = A.out_arena("dkv", (Tk, 2 * Hkv, D), F32 if accumulate == 2 else dt, fill, data=base, strides=((2 * Hkv + 1) * D, D, 1),
                                       guard_rows=TILE, device=DEV)
                p = a["dkv"].ptr()
                grads, gst = (a["dq"].ptr(), p, p + Hkv * e), ((Hq + 1) * D, D, (2 * Hkv + 1) * D, D)
            if self.n_slabs:
                a["dkv_ws"] = A.out_arena("dkv_ws", (self.n_slabs, Hkv, 2, TILE, D), F32, fill, guard_rows=1, device=DEV)
            units, splits = a.get("dkv_units"), a.get("dkv_splits")
            for which in whiches:
                A.launch("dta_tree_attn_bwd", *self.ptrs, a["out"], a["dout"], a["lse"], a["delta"], *grads, a.get("subtree_end"), a.get("run_ptr"),
                         a.get("runs"), a.get("ktile_qend"), Tq, Tk, self.meta.q_offset, Hq, Hkv, D, *self.strides, (Hq + 1) * D, D, *gst,
                         self.scale, ops._DT[dt], accumulate, which, units, 0 if units is None else units.view.shape[0],
                         splits, 0 if splits is None else splits.view.shape[0], a.get("dkv_ws"), *self.tail(a))
            return a
        return run

    def check(self, splits_forced):
        """Forward, then the backward in both launch forms and the three accumulate modes; every payload against the ops wrappers."""
        lb = self.label + (" forced splits" if splits_forced else "")
        dev = lambda t: t.to(DEV)
        q, k, v, do = (dev(t) for t in (self.q, self.k, self.v, self.do))
        out, lse, _, _ = ops.attn_fwd_raw(q, k, v, self.meta, self.scale, self.cap)
        if not splits_forced:
            got = A.check_case(self.fwd(), lb + " fwd")
            for n, w in (("out", out), ("lse", lse)):
                A.assert_same_bits(got[n], w, f"{lb} fwd {n}: the arena call against ops.attn_fwd_raw")
        g = torch.Generator().manual_seed(self.Tk)
        for acc in (0, 1, 2):
            base = None if acc == 0 else torch.randn(self.Tk, 2 * self.Hkv, self.D, generator=g).to(F32 if acc == 2 else self.dtype)
            dkv = None if acc == 0 else dev(base).clone()
            want = ops.attn_bwd_raw(q, k, v, out, do, lse, self.meta, self.scale, dk=None if acc == 0 else dkv[:, :self.Hkv],
                                    dv=None if acc == 0 else dkv[:, self.Hkv:], accumulate=acc, softcap=self.cap)
            for whiches in ((3,), (1, 2 | 8, 4)):
                l2 = f"{lb} bwd accumulate={acc} which={whiches}"
                got = A.check_case(self.bwd(out, lse, acc, whiches, base), l2, scratch=("dkv_ws",))
                if "dqkv" in got:
                    res = (got["dqkv"][:, :self.Hq], got["dqkv"][:, self.Hq:self.Hq + self.Hkv], got["dqkv"][:, self.Hq + self.Hkv:])
                else:
                    res = (got["dq"], got["dkv"][:, :self.Hkv], got["dkv"][:, self.Hkv:])
                for n, r, w in zip(("dq", "dk", "dv"), res, want):
                    A.assert_same_bits(r.contiguous(), w.contiguous(), f"{l2} {n}: the arena call against ops.attn_bwd_raw")


def _forced(meta, Tk, Tq, Hkv):
    """`meta` with every key tile cut into units of one 64-row query tile."""
    nkt = -(-Tk // TILE)
    kq = meta.ktile_qend.cpu().numpy() if meta.ktile_qend is not None else np.full(nkt, meta.q_offset + Tq, np.int32)
    units, splits, n_slabs = packing.plan_dkv_units(kq, Tk, Tq, meta.q_offset, Hkv, n_cu=1 << 20, min_tiles=1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV)
    return dataclasses.replace(meta, dkv_units=up(units), dkv_splits=up(splits) if splits.shape[0] else None, n_slabs=n_slabs)


def _packed_case(seqs, kind, Hq, Hkv, D, dtype, form):
    Wn, cap = FORMS[form]
    plan = W._trie(seqs)
    full, win, *_ = W._metas(plan, Wn if Wn > 0 else 1 << 20, Hkv)
    meta = win if Wn > 0 else full
    q, k, v, do = W._inputs(plan.T, plan.T, Hq, Hkv, D, dtype, seed=plan.T)
    return [_Case(f"packed {kind} T={plan.T} {Hq}/{Hkv} D={D} {form}", q, k, v, do, m, Hkv, cap, False) for m in (meta, _forced(meta, plan.T, plan.T, Hkv))]


@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(3, 1), (4, 2)])
@pytest.mark.parametrize("form", list(FORMS))
def test_packed(form, Hq, Hkv, D, dtype):
    """Chains and forked tries of 1, 63, 129 and 191 packed tokens (one row; a ragged first tile; one row and 63 rows into the second)."""
    slabs = 0
    for T in (1, 63, 129, 191):
        for kind, seqs in (("chain", W._chain(T)),) + ((("fork", _fork(T)),) if T > 1 else ()):
            plain, forced = _packed_case(seqs, kind, Hq, Hkv, D, dtype, form)
            plain.check(False)
            forced.check(True)
            slabs += forced.n_slabs
    assert slabs > 0 or dtype == F32, "no case reached the split dK/dV sweep and its workspace"


@pytest.mark.parametrize("dtype", [BF, F16, F32])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Hq,Hkv", [(3, 1), (4, 2)])
@pytest.mark.parametrize("form", list(FORMS))
def test_stack(form, Hq, Hkv, D, dtype):
    """B new rows at stack positions [start, start+B) over the first start+B rows of a taller K / V stack; dk / dv accumulate into the
    first start+B rows of the gradient stacks."""
    Wn, cap = FORMS[form]
    for start, B in ((0, 1), (100, 37), (120, 64)):
        q, k, v, do = W._inputs(B, start + B, Hq, Hkv, D, dtype, seed=start + B)
        meta = ops.stack_meta(start, Wn)
        for m, forced in ((meta, False), (_forced(meta, start + B, B, Hkv), True)):
            _Case(f"stack start={start} B={B} {Hq}/{Hkv} D={D} {form}", q, k, v, do, m, Hkv, cap, True).check(forced)


def test_teeth_forward_last_row_told_to_be_a_guard():
    """The forward is called correctly on a 129-row output; the helper is told that the extent ends one row earlier.  The kernel's stores
    to row 128 (the one row of the second query tile) must then be reported: the comparison sees real device stores.  Nothing out of
    bounds is executed."""
    case = _packed_case(W._chain(129), "chain", 4, 2, 128, BF, "plain")[0]
    with pytest.raises(AssertionError, match=r"out: 512 guard element\(s\) changed behind the payload"):
        A.check_case(case.fwd(disown="out"), "teeth")
