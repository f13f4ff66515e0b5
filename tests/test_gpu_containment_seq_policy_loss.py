"""Containment of the sequence-level policy-objective kernels: dta_policy_loss_seq is called through the C ABI on the guarded arenas
of tests/arena.py - a folded trie (sequences that end inside another one's path, a duplicate) and the trie with filler rows, with the
optional pointers given and NULL - and must return 0, leave every guard byte of its outputs and workspaces alone, write every element
of w, c, dlp, dent, the partial sums and the statistics, not depend on memory past an input's extent (the path tables included), and
give, bit for bit, what the allocating ops.policy_loss gives for the same inputs (whose values tests/test_gpu_seq_policy_loss.py bounds
against float64).  Guards are at least one workgroup's rows (256).  Limits as in tests/arena.py."""
import functools

import numpy as np
import pytest
import torch

import arena as A
import seq_policy_loss_ref64 as Q
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._lib import lib
from dynamictreeattn_amd._staging import upload
from dynamictreeattn_amd.losses import AGGREGATIONS, KL_ESTIMATORS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
_in, _out = functools.partial(A.in_arena, device=DEV), functools.partial(A.out_arena, device=DEV)


@pytest.mark.parametrize("name,cfg,on_policy", [("folded", "dual_k3", False), ("filler", "k1_sum", False), ("filler", "ppo", True)])
def test_seq_policy_loss_stays_inside_its_buffers(name, cfg, on_policy):
    loss, (plan, att_lens, depth, n_real, lp, ent, atts), _ = Q.case(name, cfg, seed=9, on_policy=on_policy)
    tatts = [{k: torch.from_numpy(np.asarray(v)) for k, v in a.items()} for a in atts]
    attach_lists = Q.attach_lists_of(att_lens, tatts)
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    run_ptr, row0, depth0, seq_leaf = packing.policy_path_tables(plan, attach_lists)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, torch.device(DEV))
    T, S, N, M, R = plan.T, len(seq_ptr) - 1, int(seq_ptr[-1]), len(run_ptr) - 1, len(row0)
    nb = lib().dta_policy_loss_seq_blocks(T, S)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32))
    label = f"policy_loss_seq {name} {cfg}"

    def run(fill, poison):
        a = {"lp": _in("lp", torch.from_numpy(lp), poison, guard_rows=256), "ent": _in("ent", torch.from_numpy(ent), poison, guard_rows=256),
             "depth": _in("depth", i32(depth), poison, hi=int(depth.max()), guard_rows=256),
             "row_lo": _in("row_lo", i32(lo), poison, hi=S, guard_rows=256), "row_hi": _in("row_hi", i32(hi), poison, hi=S, guard_rows=256),
             "seq_ptr": _in("seq_ptr", i32(seq_ptr), poison, hi=N, guard_rows=256),
             "run_ptr": _in("run_ptr", i32(run_ptr), poison, hi=R, guard_rows=256),
             "run_row0": _in("run_row0", i32(row0), poison, hi=T - 1, guard_rows=256),
             "run_depth0": _in("run_depth0", i32(depth0), poison, hi=int(depth.max()), guard_rows=256),
             "seq_leaf": _in("seq_leaf", i32(seq_leaf), poison, hi=M - 1, guard_rows=256),
             "mask": _in("mask", mask.cpu(), poison, guard_rows=256), "adv": _in("adv", adv.cpu(), poison, guard_rows=256)}
        if old is not None:
            a["old"] = _in("old", old.cpu(), poison, guard_rows=256)
        if ref is not None:
            a["ref"] = _in("ref", ref.cpu(), poison, guard_rows=256)
        a["w"] = _out("w", (S,), F32, fill, guard_rows=256)
        a["c"] = _out("c", (S,), F32, fill, guard_rows=256)
        a["dlp"] = _out("dlp", (T,), F32, fill, guard_rows=256)
        a["dent"] = _out("dent", (T,), F32, fill, guard_rows=256)
        a["partial"] = _out("partial", (nb, 8), F32, fill, guard_rows=4)
        a["stats"] = _out("stats", (8,), F32, fill, guard_rows=64)
        A.launch("dta_policy_loss_seq", a["lp"], a["ent"], a["depth"], a["row_lo"], a["row_hi"], a["seq_ptr"], a["run_ptr"], a["run_row0"],
                 a["run_depth0"], a["seq_leaf"], a.get("old"), a.get("ref"), a["mask"], a["adv"], int(per_seq), a["w"], a["c"], a["dlp"], a["dent"],
                 a["partial"], a["stats"], T, S, M, R, float(loss.clip_low), float(loss.clip_high),
                 0.0 if loss.dual_clip is None else float(loss.dual_clip), float(loss.kl_coef), KL_ESTIMATORS.index(loss.kl_estimator),
                 float(loss.entropy_coef), AGGREGATIONS.index(loss.agg), float(loss.scale))
        return a

    got = A.check_case(run, label)
    lo_d, hi_d, ptr_d, depth_d, *path_d = upload([lo, hi, seq_ptr, depth, run_ptr, row0, depth0, seq_leaf], DEV, np.int32)
    dlp, dent, stats, w = ops.policy_loss(loss, torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d,
                                          old, ref, mask, adv, per_seq, tuple(path_d))
    A.assert_matches(got, {"dlp": dlp, "dent": dent, "stats": stats, "w": w}, label)
    assert nb == -(-T // 256) + S and got["partial"].shape == (nb, 8)
    if name == "filler":
        assert T > n_real and (got["dlp"][n_real:] == 0).all() and (got["dent"][n_real:] == 0).all()
