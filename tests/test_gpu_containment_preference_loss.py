"""Containment of the preference-objective kernels: dta_preference_loss is called through the C ABI on the guarded arenas of
tests/arena.py - the smallest trie (one duplicate pair) and many_seqs (the grid strides of the sequence and the pair pass repeat), in
both forms of the reference and without one - and must return 0, leave every guard byte of its outputs and workspaces alone, write
every row of dlp, every element of g, u, n^ and P / n^, the partial sums and the statistics, not depend on memory past an input's extent
(the path and pair tables included), and give, bit for bit, what the allocating ops.preference_loss gives for the same inputs (whose
values tests/test_gpu_preference_loss.py bounds against float64).  Guards are at least one workgroup's rows (256).  Limits as in
tests/arena.py."""
import functools

import numpy as np
import pytest
import torch

import arena as A
import preference_ref64 as P
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._lib import lib
from dynamictreeattn_amd._staging import upload
from dynamictreeattn_amd.losses import PREFERENCE_KINDS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
_in, _out = functools.partial(A.in_arena, device=DEV), functools.partial(A.out_arena, device=DEV)


@pytest.mark.parametrize("name,cfg", [("single_len2", "dpo"), ("single_len2", "simpo"), ("many_seqs", "cdpo_sft"), ("many_seqs", "ipo_ln_sft"),
                                      ("filler", "slic")])
def test_preference_loss_stays_inside_its_buffers(name, cfg):
    loss, (plan, att_lens, depth, n_real, pair_c, pair_r, lp, atts), _ = P.case(name, cfg, seed=9)
    tatts = [{k: (torch.from_numpy(np.asarray(v)) if isinstance(v, np.ndarray) else v) for k, v in a.items()} for a in atts]
    attach_lists = P.attach_lists_of(att_lens, tatts)
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    run_ptr, row0, depth0, seq_leaf = packing.policy_path_tables(plan, attach_lists)
    ref_lp, ref_sum, mask = ops.preference_token_inputs(loss, attach_lists, seq_ptr, torch.device(DEV))
    T, S, N, M, R, NP = plan.T, len(seq_ptr) - 1, int(seq_ptr[-1]), len(run_ptr) - 1, len(row0), len(pair_c)
    nb = lib().dta_preference_loss_blocks(T, S, NP)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32))
    label = f"preference_loss {name} {cfg}"

    def run(fill, poison):
        a = {"lp": _in("lp", torch.from_numpy(lp), poison, guard_rows=256),
             "depth": _in("depth", i32(depth), poison, hi=int(depth.max()), guard_rows=256),
             "row_lo": _in("row_lo", i32(lo), poison, hi=S, guard_rows=256), "row_hi": _in("row_hi", i32(hi), poison, hi=S, guard_rows=256),
             "seq_ptr": _in("seq_ptr", i32(seq_ptr), poison, hi=N, guard_rows=256),
             "run_ptr": _in("run_ptr", i32(run_ptr), poison, hi=R, guard_rows=256),
             "run_row0": _in("run_row0", i32(row0), poison, hi=T - 1, guard_rows=256),
             "run_depth0": _in("run_depth0", i32(depth0), poison, hi=int(depth.max()), guard_rows=256),
             "seq_leaf": _in("seq_leaf", i32(seq_leaf), poison, hi=M - 1, guard_rows=256),
             "pair_c": _in("pair_c", i32(pair_c), poison, hi=S - 1, guard_rows=256),
             "pair_r": _in("pair_r", i32(pair_r), poison, hi=S - 1, guard_rows=256),
             "mask": _in("mask", mask.cpu(), poison, guard_rows=256)}
        if ref_lp is not None:
            a["ref_lp"] = _in("ref_lp", ref_lp.cpu(), poison, guard_rows=256)
        if ref_sum is not None:
            a["ref_sum"] = _in("ref_sum", ref_sum.cpu(), poison, guard_rows=256)
        for k in ("nhat", "u", "sft", "g"):
            a[k] = _out(k, (S,), F32, fill, guard_rows=256)
        a["dlp"] = _out("dlp", (T,), F32, fill, guard_rows=256)
        a["partial"] = _out("partial", (nb, 8), F32, fill, guard_rows=4)
        a["stats"] = _out("stats", (8,), F32, fill, guard_rows=64)
        A.launch("dta_preference_loss", a["lp"], a["depth"], a["row_lo"], a["row_hi"], a["seq_ptr"], a["run_ptr"], a["run_row0"], a["run_depth0"],
                 a["seq_leaf"], a["pair_c"], a["pair_r"], a.get("ref_lp"), a.get("ref_sum"), a["mask"], a["nhat"], a["u"], a["sft"], a["g"],
                 a["dlp"], a["partial"], a["stats"], T, S, M, R, NP, PREFERENCE_KINDS.index(loss.kind), float(loss.beta),
                 float(loss.label_smoothing), float(loss.gamma), int(loss.length_normalize), int(loss.reference_free), float(loss.sft_coef),
                 float(loss.scale))
        return a

    got = A.check_case(run, label)
    lo_d, hi_d, ptr_d, depth_d, *rest = upload([lo, hi, seq_ptr, depth, run_ptr, row0, depth0, seq_leaf, pair_c, pair_r], DEV, np.int32)
    dlp, stats, g, u = ops.preference_loss(loss, torch.from_numpy(lp).to(DEV), depth_d, lo_d, hi_d, ptr_d, tuple(rest[:4]), tuple(rest[4:]),
                                           ref_lp, ref_sum, mask)
    A.assert_matches(got, {"dlp": dlp, "stats": stats, "g": g, "u": u}, label)
    assert nb == -(-NP // 256) and got["partial"].shape == (nb, 8)
    assert np.array_equal(got["nhat"].cpu().numpy(), np.asarray([max(float(np.asarray(a["loss_mask"]).sum()), 1.0) for a in atts], np.float32))
    if name == "filler":
        assert T > n_real and (got["dlp"][n_real:] == 0).all()
