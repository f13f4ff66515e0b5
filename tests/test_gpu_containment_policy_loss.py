"""Containment of the policy-objective kernels: dta_policy_loss is called through the C ABI on the guarded arenas of tests/arena.py -
a trie whose root rows take the wave-wide path and whose other rows the single-thread path, T off a workgroup multiple, a folded trie
(sequences that end inside another one's path, a duplicate), 300 sequences through the root rows and the trie with filler rows; with
the path tables given and NULL, old_lp given and NULL, no rollout weight, a weight per token and per sequence, both ratio levels and
CISPO - and must return 0, leave every guard byte of its outputs and workspaces alone, write every element of w, c, omega, dlp, dent,
the partial sums and the statistics, not depend on memory past an input's extent (the path tables and rollout_lp included), and give,
bit for bit, what the allocating ops.policy_loss gives for the same inputs (whose values tests/test_gpu_policy_loss.py,
tests/test_gpu_seq_policy_loss.py and tests/test_gpu_offpolicy_loss.py bound against float64).  The kernel always writes eight
statistics: without a rollout weight the last two are the masked-token count again and 0, exactly, whatever the ratio level.
Guards are at least one workgroup's rows (256).  Limits as in tests/arena.py."""
import functools

import numpy as np
import pytest
import torch

import arena as A
import offpolicy_loss_ref64 as O
import policy_loss_ref64 as R
import seq_policy_loss_ref64 as Q
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._lib import lib
from dynamictreeattn_amd._staging import upload
from dynamictreeattn_amd.losses import AGGREGATIONS, IS_LEVELS, IS_MODES, KL_ESTIMATORS, RATIOS, SURROGATES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
_in, _out = functools.partial(A.in_arena, device=DEV), functools.partial(A.out_arena, device=DEV)

# (configurations of, trie, configuration, without old_logprobs)
CASES = [("token", "fan70", "dual_k3", False), ("token", "past_block", "ppo", True),
         ("sequence", "folded", "dual_k3", False), ("sequence", "filler", "k1_sum", False), ("sequence", "filler", "ppo", True),
         ("offpolicy", "folded", "tok_mask", False), ("offpolicy", "folded", "seq_trunc", True), ("offpolicy", "folded", "gspo_tok_trunc", True),
         ("offpolicy", "fan300", "mean_mask", False), ("offpolicy", "fan300", "gspo_seq_mask", False), ("offpolicy", "fan300", "cispo", False),
         ("offpolicy", "filler", "seq_mask", True), ("offpolicy", "filler", "cispo_tok_trunc_k3", True),
         ("offpolicy", "filler", "gspo_tok_trunc", False)]


def _case(family, name, cfg, on_policy):
    if family == "token":
        return R.CONFIGS()[cfg], R.make_inputs(name, seed=9, on_policy=on_policy)
    return (Q if family == "sequence" else O).case(name, cfg, seed=9, on_policy=on_policy)[:2]


@pytest.mark.parametrize("family,name,cfg,on_policy", CASES)
def test_policy_loss_stays_inside_its_buffers(family, name, cfg, on_policy):
    loss, (plan, att_lens, depth, n_real, lp, ent, atts) = _case(family, name, cfg, on_policy)
    assert (loss.ratio == "sequence") == (family == "sequence" or cfg.startswith("gspo")) and loss.extended == (family == "offpolicy")
    tatts = [{k: torch.from_numpy(np.asarray(v)) for k, v in a.items()} for a in atts]
    attach_lists = R.attach_lists_of(att_lens, tatts)
    lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
    old, ref, mask, adv, per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, torch.device(DEV))
    rollout = ops.policy_rollout_input(loss, attach_lists, seq_ptr, torch.device(DEV))
    walks = ops.policy_walks_paths(loss, old is None)
    assert (old is None) == on_policy and (rollout is None) == (loss.is_level is None)
    path = packing.policy_path_tables(plan, attach_lists) if walks else None
    T, S, N = plan.T, len(seq_ptr) - 1, int(seq_ptr[-1])
    M, R_ = (len(path[0]) - 1, len(path[1])) if walks else (0, 0)
    nb = lib().dta_policy_loss_blocks(T, S)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32))
    label = f"policy_loss {family} {name} {cfg}"

    def run(fill, poison):
        a = {"lp": _in("lp", torch.from_numpy(lp), poison, guard_rows=256), "ent": _in("ent", torch.from_numpy(ent), poison, guard_rows=256),
             "depth": _in("depth", i32(depth), poison, hi=int(depth.max()), guard_rows=256),
             "row_lo": _in("row_lo", i32(lo), poison, hi=S, guard_rows=256), "row_hi": _in("row_hi", i32(hi), poison, hi=S, guard_rows=256),
             "seq_ptr": _in("seq_ptr", i32(seq_ptr), poison, hi=N, guard_rows=256),
             "mask": _in("mask", mask.cpu(), poison, guard_rows=256), "adv": _in("adv", adv.cpu(), poison, guard_rows=256)}
        if walks:
            run_ptr, row0, depth0, seq_leaf = path
            a["run_ptr"] = _in("run_ptr", i32(run_ptr), poison, hi=R_, guard_rows=256)
            a["run_row0"] = _in("run_row0", i32(row0), poison, hi=T - 1, guard_rows=256)
            a["run_depth0"] = _in("run_depth0", i32(depth0), poison, hi=int(depth.max()), guard_rows=256)
            a["seq_leaf"] = _in("seq_leaf", i32(seq_leaf), poison, hi=M - 1, guard_rows=256)
        for key, t in (("old", old), ("ref", ref), ("rollout", rollout)):
            if t is not None:
                a[key] = _in(key, t.cpu(), poison, guard_rows=256)
        for key in ("w", "c", "omega"):
            a[key] = _out(key, (S,), F32, fill, guard_rows=256)
        a["dlp"] = _out("dlp", (T,), F32, fill, guard_rows=256)
        a["dent"] = _out("dent", (T,), F32, fill, guard_rows=256)
        a["partial"] = _out("partial", (nb, 8), F32, fill, guard_rows=4)
        a["stats"] = _out("stats", (8,), F32, fill, guard_rows=64)
        A.launch("dta_policy_loss", a["lp"], a["ent"], a["depth"], a["row_lo"], a["row_hi"], a["seq_ptr"], a.get("run_ptr"), a.get("run_row0"),
                 a.get("run_depth0"), a.get("seq_leaf"), a.get("old"), a.get("ref"), a.get("rollout"), a["mask"], a["adv"], int(per_seq),
                 a["w"], a["c"], a["omega"], a["dlp"], a["dent"], a["partial"], a["stats"], T, S, M, R_, float(loss.clip_low),
                 float(loss.clip_high), 0.0 if loss.dual_clip is None else float(loss.dual_clip), float(loss.kl_coef),
                 KL_ESTIMATORS.index(loss.kl_estimator), float(loss.entropy_coef), AGGREGATIONS.index(loss.agg), float(loss.scale),
                 RATIOS.index(loss.ratio), SURROGATES.index(loss.surrogate), 0 if loss.is_level is None else IS_LEVELS.index(loss.is_level) + 1,
                 IS_MODES.index(loss.is_mode), float(loss.is_cap), float(loss.is_floor))
        return a

    got = A.check_case(run, label)
    lo_d, hi_d, ptr_d, depth_d, *path_d = upload([lo, hi, seq_ptr, depth, *(path or [])], DEV, np.int32)
    ws = {}
    dlp, dent, stats, w = ops.policy_loss(loss, torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV), depth_d, lo_d, hi_d, ptr_d,
                                          old, ref, mask, adv, per_seq, tuple(path_d) or None, rollout, ws)
    assert stats.shape == (8 if loss.extended else 6,)                   # the wrapper hands out the statistics the objective names
    A.assert_matches({**got, "stats": got["stats"][:stats.shape[0]]},
                     {"dlp": dlp, "dent": dent, "stats": stats, "w": w, "c": ws["c"], "omega": ws["omega"]}, label)
    assert nb == -(-T // 256) + S and got["partial"].shape == (nb, 8)
    if loss.is_level is None:                                            # counts of a 0 / 1 mask: exact under either ratio level
        assert got["stats"][6] == got["stats"][5] and got["stats"][7] == 0, (label, got["stats"])
    if name == "filler":
        assert T > n_real and (got["dlp"][n_real:] == 0).all() and (got["dent"][n_real:] == 0).all()
