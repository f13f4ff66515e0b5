"""The four trie kernels (dta_lcp_adjacent, dta_leafize, dta_preorder_meta, dta_window_lo) called directly through the C ABI on guarded
arenas (tests/arena.py) - the entry-level tests they did not have; elsewhere they run only through TokenTrie / _PackedTrie.  They are
integer kernels: the expected values are numpy restatements written here, hostmirror.expand_plan_host and packing.window_lo_host, and
every comparison is exact.  Each case must return 0, leave every guard byte of its outputs alone, give the same integers under the
0x7f7f7f7f and the 0x01010101 fill (every element written, none read first) and under the two input poisons.  The guards of an index
table hold values that are in range for that table (0 in one run, its largest valid value in the other): a stray index read must change
the result, never the address space.  dta_window_lo is also compared with ops.window_lo_device; the other three have no allocating
wrapper outside the trie classes.

dta_leafize writes M leaf positions and M - 1 leaf LCPs into buffers the caller sizes for S and S - 1: the entries past M and M - 1 are
part of the allocation but not of the result, and the kernel leaves them alone - asserted here as "still the fill".

Guards: one workgroup's elements (256 for the per-token kernels, 1024 for the leafization, 64 around the per-pair outputs).
Limits (tests/arena.py): a stray load whose value is discarded is not seen; a stray store further than the guard band is not caught;
no time is measured."""
import numpy as np
import pytest
import torch

import arena as A
import hostmirror
from dynamictreeattn_amd import ops, packing

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64 = torch.int32, torch.int64


def _in(name, data, poison, hi, **kw):
    return A.in_arena(name, torch.as_tensor(np.ascontiguousarray(data)), poison, hi=hi, device=DEV, **kw)


def _out(name, shape, dtype, fill, **kw):
    return A.out_arena(name, shape, dtype, fill, device=DEV, **kw)


def _expect(got, want, label):
    for name, w in want.items():
        A.assert_same_bits(got[name].cpu(), torch.as_tensor(np.ascontiguousarray(w)).to(got[name].dtype), f"{label} {name}: the kernel against the host restatement")


# ------------------------------------------------------------------------------------------------ adjacent LCP
POSITIONS = [0, 255, 256, 1023, 1024, 1025, "n"]          # first mismatch of a pair; "n": one sequence is a prefix of the other
LEN = 1100


def _sequences(S, shift, unsorted_pair):
    """S sequences in which pair i first differs at POSITIONS[(i + shift) % 7], ascending there except in `unsorted_pair`."""
    rng = np.random.default_rng(S + shift)
    seqs, want = [rng.integers(10, 1 << 40, LEN)], []
    for i in range(S - 1):
        prev, p = seqs[-1], POSITIONS[(i + shift) % 7]
        if p == "n":
            nxt = np.concatenate([prev, [5]])                  # the pair that follows cuts back to LEN tokens
            want.append(len(prev))
        else:
            nxt = np.concatenate([prev[:p], [prev[p] + (-1 if i == unsorted_pair else 1)], rng.integers(10, 1 << 40, LEN - p - 1)])
            want.append(p)
        seqs.append(nxt)
    return seqs, want


@pytest.mark.parametrize("S,shift", [(2, s) for s in range(7)] + [(3, s) for s in range(7)] + [(300, 0)])
def test_lcp_adjacent(S, shift):
    """out_lcp holds exactly S - 1 ints; out_unsorted is added to (the caller zeroes it) and counts the one descending pair."""
    bad_pair = 0 if POSITIONS[shift % 7] != "n" else 1 if S > 2 else None
    seqs, want = _sequences(S, shift, bad_pair)
    lens = np.array([len(s) for s in seqs], np.int32)
    starts = (np.cumsum(lens) - lens).astype(np.int64)
    tokens = np.concatenate(seqs).astype(np.int64)
    label = f"lcp_adjacent S={S} shift={shift}"

    def run(fill, poison):
        a = {"tokens": _in("tokens", tokens, poison, 1 << 40, guard_rows=2048), "starts": _in("starts", starts, poison, int(starts.max()), guard_rows=64),
             "lens": _in("lens", lens, poison, int(lens.min()), guard_rows=64), "out_lcp": _out("out_lcp", (S - 1,), I32, fill, guard_rows=64),
             "out_unsorted": _out("out_unsorted", (1,), I32, fill, data=torch.zeros(1, dtype=I32), guard_rows=64)}
        A.launch("dta_lcp_adjacent", a["tokens"], a["starts"], a["lens"], S, a["out_lcp"], a["out_unsorted"])
        return a
    got = A.check_case(run, label)
    assert want == [next((j for j in range(min(len(x), len(y))) if x[j] != y[j]), min(len(x), len(y))) for x, y in zip(seqs[:-1], seqs[1:])]
    _expect(got, {"out_lcp": np.array(want, np.int32), "out_unsorted": np.array([0 if bad_pair is None else 1], np.int32)}, label)


# ------------------------------------------------------------------------------------------------ leafization
def _keep_pattern(S, kind):
    if kind == "all":
        keep = np.ones(S, bool)
    elif kind == "last_only":
        keep = np.zeros(S, bool)
    else:                                       # alternating runs of 63, 64 and 65 kept / folded sequences
        keep, i, j = np.zeros(S, bool), 0, 0
        while i < S:
            n = (63, 64, 65)[j % 3]
            keep[i:i + n] = j % 2 == 0
            i, j = i + n, j + 1
    keep[S - 1] = True
    return keep


@pytest.mark.parametrize("kind", ["all", "last_only", "runs"])
@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 2049])
def test_leafize(S, kind):
    """The caller sizes out_leaf_pos for S and out_leaf_lcp for S - 1 entries; the kernel writes M and M - 1 of them and leaves the
    rest alone (they still hold the fill).  out_seq_leaf [S] and out_M are written in full."""
    keep = _keep_pattern(S, kind)
    lens = np.full(S, 10, np.int32)
    lcp = np.where(keep[:-1], 5, 10).astype(np.int32)           # kept: lcp < min(len, len'); folded onto the next: lcp == len
    pos = np.flatnonzero(keep).astype(np.int32)
    M = len(pos)
    want = {"out_leaf_pos": pos, "out_leaf_lcp": lcp[pos[:-1]], "out_seq_leaf": (np.cumsum(keep) - keep).astype(np.int32), "out_M": np.array([M], np.int32)}
    label = f"leafize S={S} {kind}"
    for fill, poison in (("A", 0), ("B", 0), ("A", 1)):
        a = {"lens": _in("lens", lens, poison, 10, guard_rows=1024), "out_leaf_pos": _out("out_leaf_pos", (S,), I32, fill, guard_rows=1024),
             "out_leaf_lcp": _out("out_leaf_lcp", (max(S - 1, 1),), I32, fill, guard_rows=1024),
             "out_seq_leaf": _out("out_seq_leaf", (S,), I32, fill, guard_rows=1024), "out_M": _out("out_M", (1,), I32, fill, guard_rows=64)}
        if S > 1:
            a["lcp"] = _in("lcp", lcp, poison, 10, guard_rows=1024)
        A.launch("dta_leafize", a["lens"], a.get("lcp"), S, a["out_leaf_pos"], a["out_leaf_lcp"], a["out_seq_leaf"], a["out_M"])
        for t in a.values():
            t.assert_guards_intact(f"{label} [fill {fill}, poison {poison}]")
        got = {n: t.payload().cpu() for n, t in a.items() if not t.is_input}
        lb = f"{label} [fill {fill}, poison {poison}]"
        for n, w in want.items():
            A.assert_same_bits(got[n][:len(w)], torch.from_numpy(np.ascontiguousarray(w)), f"{lb} {n}: the kernel against the host restatement")
        for n, used in (("out_leaf_pos", M), ("out_leaf_lcp", M - 1)):
            assert bool((got[n][used:] == A.fill_value(I32, fill)).all()), f"{lb} {n}: an entry past the result was written"


# ------------------------------------------------------------------------------------------------ pre-order metadata, window lower bounds
def _plan_case(lens, lcps):
    """(plan, tokens int64, leaf_tok_off int64) of leaves with the given lengths and adjacent LCPs: leaf i repeats leaf i-1 up to its
    LCP and goes on with tokens of its own."""
    plan = packing.plan_segments(lens, lcps)
    seqs, nxt = [], 1000
    for i, n in enumerate(lens):
        c = lcps[i - 1] if i else 0
        seqs.append(np.concatenate([seqs[-1][:c] if i else np.zeros(0, np.int64), np.arange(nxt, nxt + n - c, dtype=np.int64)]))
        nxt += n - c
    ln = np.array(lens, np.int64)
    return plan, np.concatenate(seqs), (np.cumsum(ln) - ln)


BIG = 2048 * 256 + 300                                                # the 2048-workgroup grid takes a second, ragged trip
PLANS = {"T1": ([1], []), "T257_one_leaf": ([257], []),
         "T257_empty_segments": ([100, 60, 60, 197], [60, 60, 40]),     # leaves 1 and 2 are prefixes of leaf 0: two empty segments at offset 100
         "T257_forks": ([90, 120, 64, 78], [30, 64, 1]),                 # leaf 2 is a prefix of leaf 1: an empty segment between forks
         "big": ([200000, 200010, BIG - 400000 + 20], [10, 20])}


@pytest.mark.parametrize("name", list(PLANS))
def test_preorder_meta_and_window_lo(name):
    lens, lcps = PLANS[name]
    plan, tokens, leaf_off = _plan_case(lens, lcps)
    M, T = plan.M, plan.T
    assert T == {"T1": 1, "big": BIG}.get(name, 257)
    if name == "T257_empty_segments":
        assert list(plan.seg_off[1:4]) == [100, 100, 100]
    seg, depth, parent, se = hostmirror.expand_plan_host(plan)
    nbrk = len(plan.brk_depth)
    label = f"preorder_meta {name} M={M} T={T}"

    def tables(poison):
        return {"seg_off": _in("seg_off", plan.seg_off, poison, T, guard_rows=64), "seg_depth0": _in("seg_depth0", plan.seg_depth0, poison, int(plan.seg_depth0.max()), guard_rows=64),
                "parent_of_seg": _in("parent_of_seg", plan.parent_of_seg, poison, T - 1, guard_rows=64)}

    def run(fill, poison):
        a = tables(poison)
        a.update(tokens=_in("tokens", tokens, poison, 1 << 40, guard_rows=256), leaf_tok_off=_in("leaf_tok_off", leaf_off, poison, int(leaf_off.max()), guard_rows=64),
                 brk_ptr=_in("brk_ptr", plan.brk_ptr, poison, nbrk, guard_rows=64), brk_depth=_in("brk_depth", plan.brk_depth, poison, int(plan.brk_depth.max()), guard_rows=64),
                 brk_end=_in("brk_end", plan.brk_end, poison, T, guard_rows=64), out_token=_out("out_token", (T,), I64, fill, guard_rows=256),
                 out_depth=_out("out_depth", (T,), I32, fill, guard_rows=256), out_parent=_out("out_parent", (T,), I32, fill, guard_rows=256),
                 out_subtree_end=_out("out_subtree_end", (T,), I32, fill, guard_rows=256))
        A.launch("dta_preorder_meta", a["tokens"], a["leaf_tok_off"], a["seg_off"], a["seg_depth0"], a["parent_of_seg"], a["brk_ptr"], a["brk_depth"],
                 a["brk_end"], M, T, a["out_token"], a["out_depth"], a["out_parent"], a["out_subtree_end"])
        return a
    _expect(A.check_case(run, label), {"out_token": tokens[leaf_off[seg] + depth], "out_depth": depth, "out_parent": parent, "out_subtree_end": se}, label)

    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    for window in (1, 64, int(depth.max()) + 2):
        lb = f"window_lo {name} M={M} T={T} window={window}"

        def wrun(fill, poison):
            a = tables(poison)
            a.update(depth=_in("depth", depth, poison, int(depth.max()), guard_rows=256), out_win_lo=_out("out_win_lo", (T,), I32, fill, guard_rows=256))
            A.launch("dta_window_lo", a["depth"], a["seg_off"], a["seg_depth0"], a["parent_of_seg"], M, T, window, a["out_win_lo"])
            return a
        got = A.check_case(wrun, lb)
        _expect(got, {"out_win_lo": packing.window_lo_host(plan, window)}, lb)
        A.assert_same_bits(got["out_win_lo"], ops.window_lo_device(up(depth), up(plan.seg_off), up(plan.seg_depth0), up(plan.parent_of_seg), window),
                           lb + " out_win_lo: the arena call against the ops wrapper")
