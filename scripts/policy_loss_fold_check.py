#!/usr/bin/env python3
"""The fold of the three policy-loss entries into dta_policy_loss, checked against the library of the commit before it: two shared
libraries are loaded by path and called through ctypes on identical inputs, each by its own entry names.

  --parent PATH   a build of the commit before the fold: dta_policy_loss (token level), dta_policy_loss_seq, dta_policy_loss_ex
  --new PATH      a build of this tree: dta_policy_loss alone
Either may be the whole libdta_mi355x.so or csrc/loss_kernels.hip compiled on its own (hipcc --offload-arch=gfx950 -O3 -fPIC -shared).

bits   every case and configuration of tests/test_gpu_policy_loss.py, test_gpu_seq_policy_loss.py and test_gpu_offpolicy_loss.py
       (the tries, seeds and variants those tests run): dlp, dent, w, stats[0:6], c under a sequence-level ratio, omega and stats[6:8]
       where the parent's entry wrote them, compared bit for bit with +0 == -0.  Per array: elements compared, elements that differ,
       the largest difference in ulps.
speed  HIP-event time of one entry call (its three launches) at a tau2-shaped trie of T = 28 160 rows (8 leaves of 6 turn-prefix
       sequences behind a 2 560-token prompt) and at the `short` workload of scripts/policy_loss_bench.py (512 sequences of 1 024
       tokens behind 256 shared ones), for the default token-level objective of that script, ratio="sequence" and a per-token rollout
       weight; the two libraries alternate in three rounds.  A sample is the mean over --calls back-to-back calls; a round's figure is
       the median of --samples samples.  Pass: every round of the new library is no slower than the parent's slowest round.  The
       outputs at these shapes are compared too.
One JSON object goes to --out.
Usage: python scripts/policy_loss_fold_check.py --parent PATH --new PATH [--skip-bits] [--skip-speed] [--out profiles/policy_loss_fold.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import offpolicy_loss_ref64 as O
import policy_loss_ref64 as R
import seq_policy_loss_ref64 as Q
from dynamictreeattn_amd import ops, packing
from dynamictreeattn_amd._staging import upload
from dynamictreeattn_amd.losses import AGGREGATIONS, IS_LEVELS, IS_MODES, KL_ESTIMATORS, RATIOS, SURROGATES, PolicyLoss

DEV = torch.device("cuda:0")
_i32, _f32, _vp = C.c_int32, C.c_float, C.c_void_p
HYPER = [_f32] * 4 + [_i32, _f32, _i32, _f32]                          # clip_low clip_high dual_clip kl_coef | kl_estimator | entropy_coef | agg | scale
OPTIONS = [_i32] * 4 + [_f32, _f32]                                     # ratio_level surrogate is_level is_mode | is_cap is_floor
FOLDED = [_vp] * 15 + [_i32] + [_vp] * 7 + [_i32] * 4 + HYPER + OPTIONS + [_vp]
PARENT_PROTOS = {"dta_policy_loss": [_vp] * 10 + [_i32] + [_vp] * 5 + [_i32] * 2 + HYPER + [_vp],
                 "dta_policy_loss_seq": [_vp] * 14 + [_i32] + [_vp] * 6 + [_i32] * 4 + HYPER + [_vp], "dta_policy_loss_ex": FOLDED}
NEW_PROTOS = {"dta_policy_loss": FOLDED}


def load(path, protos):
    lib = C.CDLL(os.path.abspath(path))
    for name, args in protos.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    return lib


class Call:
    """The staged inputs of one objective on one trie, and one set of outputs per library"""

    def __init__(self, loss, plan, att_lens, depth, lp, ent, atts):
        tatts = [{k: (v if isinstance(v, float) else torch.from_numpy(np.asarray(v))) for k, v in a.items()} for a in atts]
        attach_lists = R.attach_lists_of(att_lens, tatts)
        lo, hi, seq_ptr, _ = packing.policy_row_tables(plan, attach_lists)
        self.loss, self.T, self.S = loss, plan.T, len(seq_ptr) - 1
        self.old, self.ref, self.mask, self.adv, self.per_seq = ops.policy_token_inputs(loss, attach_lists, seq_ptr, DEV)
        self.rollout = ops.policy_rollout_input(loss, attach_lists, seq_ptr, DEV)
        self.walks = ops.policy_walks_paths(loss, self.old is None)
        path = list(packing.policy_path_tables(plan, attach_lists)) if self.walks else []
        self.M, self.Rn = (len(path[0]) - 1, len(path[1])) if self.walks else (0, 0)
        self.lo, self.hi, self.seq_ptr, self.depth, *self.path = upload([lo, hi, seq_ptr, depth, *path], DEV, np.int32)
        self.path = self.path or [None] * 4
        self.lp, self.ent = torch.from_numpy(lp).to(DEV), torch.from_numpy(ent).to(DEV)
        self.nb = -(-self.T // 256) + min(self.S, 2048)                  # enough partial rows for every entry
        self.entry = "dta_policy_loss_ex" if loss.extended else "dta_policy_loss_seq" if loss.ratio == "sequence" else "dta_policy_loss"
        self.hyper = (float(loss.clip_low), float(loss.clip_high), 0.0 if loss.dual_clip is None else float(loss.dual_clip), float(loss.kl_coef),
                      KL_ESTIMATORS.index(loss.kl_estimator), float(loss.entropy_coef), AGGREGATIONS.index(loss.agg), float(loss.scale))
        self.options = (RATIOS.index(loss.ratio), SURROGATES.index(loss.surrogate), 0 if loss.is_level is None else IS_LEVELS.index(loss.is_level) + 1,
                        IS_MODES.index(loss.is_mode), float(loss.is_cap), float(loss.is_floor))

    def outputs(self):
        nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
        return {"w": nan(self.S), "c": nan(self.S), "omega": nan(self.S), "dlp": nan(self.T), "dent": nan(self.T), "partial": nan(8 * self.nb),
                "stats": nan(8)}

    def launcher(self, lib, out, entry, folded=False):
        """a closure that calls `entry` of `lib` once on the current stream; folded: the one entry of this tree"""
        p = lambda t: None if t is None else t.data_ptr()
        rows = [p(t) for t in (self.lp, self.ent, self.depth, self.lo, self.hi, self.seq_ptr)]
        tail = [p(out[k]) for k in ("dlp", "dent", "partial", "stats")]
        if entry == "dta_policy_loss" and not folded:                    # the parent's token-level entry
            argv = rows + [p(self.old), p(self.ref), p(self.mask), p(self.adv), int(self.per_seq), p(out["w"])] + tail + [self.T, self.S, *self.hyper]
        elif entry == "dta_policy_loss_seq":
            argv = (rows + [p(t) for t in self.path] + [p(self.old), p(self.ref), p(self.mask), p(self.adv), int(self.per_seq), p(out["w"]), p(out["c"])]
                    + tail + [self.T, self.S, self.M, self.Rn, *self.hyper])
        else:
            argv = (rows + [p(t) for t in self.path] + [p(self.old), p(self.ref), p(self.rollout), p(self.mask), p(self.adv), int(self.per_seq),
                                                         p(out["w"]), p(out["c"]), p(out["omega"])]
                    + tail + [self.T, self.S, self.M, self.Rn, *self.hyper, *self.options])
        fn, stream = getattr(lib, entry), torch.cuda.current_stream().cuda_stream

        def call():
            rc = fn(*argv, stream)
            if rc != 0:
                raise RuntimeError(f"{entry} returned {rc}")
        return call

    def compared(self):
        """name -> slice of the arrays the parent's entry writes"""
        names = {"dlp": slice(None), "dent": slice(None), "w": slice(None), "stats[0:6]": slice(0, 6)}
        if self.loss.ratio == "sequence" or self.loss.extended:
            names["c"] = slice(None)
        if self.loss.extended:
            names.update({"omega": slice(None), "stats[6:8]": slice(6, 8)})
        return names


def ulps(a, b):
    """distance in units in the last place between two fp32 arrays (bit patterns mapped to a monotone integer line; +0 == -0)"""
    def line(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


def compare(call, parent, new, tally, label):
    a, b = call.outputs(), call.outputs()
    call.launcher(parent, a, call.entry)()
    call.launcher(new, b, "dta_policy_loss", folded=True)()
    torch.cuda.synchronize()
    for name, sl in call.compared().items():
        key = name.split("[")[0]
        x, y = a[key].cpu().numpy()[sl], b[key].cpu().numpy()[sl]
        assert np.isfinite(x).all() and np.isfinite(y).all(), (label, name, "an element was left unwritten")
        d = ulps(x, y)
        t = tally.setdefault(name, {"elements": 0, "differing": 0, "max_ulps": 0, "first_differing_case": None})
        t["elements"] += int(d.size); t["differing"] += int((d > 0).sum()); t["max_ulps"] = max(t["max_ulps"], int(d.max(initial=0)))
        if (d > 0).any() and t["first_differing_case"] is None:
            t["first_differing_case"] = label
    if not call.loss.extended:                                          # what the folded entry adds: the masked count again, and 0
        s = b["stats"].cpu().numpy()
        assert s[6] == s[5] and s[7] == 0, (label, s.tolist())


def bit_cases():
    """(label, loss, inputs) of every case the three GPU loss tests run"""
    for name in R.TRIES:
        for cfg, loss in R.CONFIGS().items():
            yield f"token {name} {cfg}", loss, R.make_inputs(name, seed=11)
    for name, cfg in (("folded", "dual_k3"), ("fan300", "ppo"), ("filler", "k1_sum")):
        for seed, kw in ((5, dict(on_policy=True)), (6, dict(scalar_adv=True)), (7, dict(scalar_adv=True, on_policy=True))):
            yield f"token {name} {cfg} {kw}", R.CONFIGS()[cfg], R.make_inputs(name, seed=seed, **kw)
    for name, cfg in (("folded", "dual_k3"),):
        yield f"token {name} {cfg} seed 2", R.CONFIGS()[cfg], R.make_inputs(name, seed=2)
    seq = Q.SEQ_CONFIGS()
    for name in Q.TRIES:
        for cfg, loss in seq.items():
            yield f"sequence {name} {cfg}", loss, Q.make_inputs(name, seed=11)
    for i, name in enumerate(Q.TRIES):
        cfg = list(seq)[i % 3]
        yield f"sequence {name} {cfg} on policy", seq[cfg], Q.make_inputs(name, seed=5, on_policy=True)
        yield f"sequence {name} {cfg} scalar", seq[cfg], Q.make_inputs(name, seed=6, scalar_adv=True)
    yield "sequence folded dual_k3 seed 2", seq["dual_k3"], Q.make_inputs("folded", seed=2)
    for name in R.TRIES:
        for cfg, loss in O.CONFIGS().items():
            for on_policy in (False, True):
                for scalar in (False, True):
                    yield (f"offpolicy {name} {cfg} {'no old' if on_policy else 'old'} {'scalar' if scalar else 'per token'}", loss,
                           O.make_inputs(name, seed=11, on_policy=on_policy, scalar_adv=scalar, seq_ratio=loss.ratio == "sequence"))
    yield "offpolicy folded cispo_tok_trunc_k3 seed 2", O.CONFIGS()["cispo_tok_trunc_k3"], O.make_inputs("folded", seed=2)


def run_bits(parent, new):
    tally, n = {}, 0
    for label, loss, (plan, att_lens, depth, _, lp, ent, atts) in bit_cases():
        compare(Call(loss, plan, att_lens, depth, lp, ent, atts), parent, new, tally, label)
        n += 1
    return {"cases": n, "arrays": tally, "differing_elements": sum(t["differing"] for t in tally.values())}


# ---- speed -------------------------------------------------------------------------------------------------------------------------
SHAPES = {
    # name: (leaf lengths, adjacent leaves' common prefixes, per-leaf sequence lengths)
    "tau2_shaped": ([5760] * 8, [2560] * 7, [[2560 + 533 * k for k in range(1, 6)] + [5760]] * 8),
    "short": ([1024] * 512, [256] * 511, [[1024]] * 512),
}
BENCH = dict(clip_low=0.2, clip_high=0.28, kl_coef=0.02, kl_estimator="k3", entropy_coef=0.001)      # scripts/policy_loss_bench.py
SPEED_CONFIGS = {"token": PolicyLoss(**BENCH), "sequence": PolicyLoss(ratio="sequence", **BENCH),
                 "token_is_token_truncate": PolicyLoss(is_level="token", is_mode="truncate", is_cap=2.0, **BENCH)}


def speed_inputs(shape, seed=0):
    lens, lcp, att_lens = SHAPES[shape]
    plan = packing.plan_segments(lens, lcp)
    if plan.T >= 2048 and plan.T % 256:
        plan = packing.pad_plan(plan, 256)
    seg = np.repeat(np.arange(plan.M), np.diff(plan.seg_off))
    depth = (plan.seg_depth0[seg] + np.arange(plan.T) - plan.seg_off[seg]).astype(np.int32)
    rng = np.random.default_rng(seed)
    lp, ent = (-rng.uniform(0.05, 6.0, plan.T)).astype(np.float32), rng.uniform(0.0, 5.0, plan.T).astype(np.float32)
    atts = []
    for rows in R.paths_of(plan, att_lens):
        n, mine = rows.size - 1, lp[rows[1:]]
        old = (mine + rng.uniform(-0.3, 0.3, n)).astype(np.float32)
        atts.append({"advantages": rng.normal(0, 1.0, n).astype(np.float32), "old_logprobs": old,
                     "ref_logprobs": (mine + rng.uniform(-0.3, 0.3, n)).astype(np.float32), "loss_mask": rng.random(n) < 0.8,
                     "rollout_logprobs": (old + rng.uniform(-0.05, 0.05, n)).astype(np.float32)})
    return plan, att_lens, depth, lp, ent, atts


def time_round(call, samples, calls):
    """median over `samples` of the HIP-event time of `calls` back-to-back entry calls, in microseconds per call"""
    out = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record(); b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / calls)
    return statistics.median(out)


def run_speed(parent, new, rounds, samples, calls):
    records = []
    for shape in SHAPES:
        plan, att_lens, depth, lp, ent, atts = speed_inputs(shape)
        for cfg, loss in SPEED_CONFIGS.items():
            call = Call(loss, plan, att_lens, depth, lp, ent, atts)
            tally = {}
            compare(call, parent, new, tally, f"{shape} {cfg}")
            outs = call.outputs()
            fns = {"parent": call.launcher(parent, outs, call.entry), "new": call.launcher(new, outs, "dta_policy_loss", folded=True)}
            for fn in fns.values():                                     # warm up: code objects loaded, clocks up
                for _ in range(3 * calls):
                    fn()
            torch.cuda.synchronize()
            us = {"parent": [], "new": []}
            for _ in range(rounds):
                for which in ("parent", "new"):
                    us[which].append(round(time_round(fns[which], samples, calls), 3))
            rec = {"shape": shape, "T": call.T, "S": call.S, "N": int(call.mask.shape[0]), "config": cfg, "parent_entry": call.entry,
                   "parent_us_per_call": us["parent"], "new_us_per_call": us["new"],
                   "pass": max(us["new"]) <= max(us["parent"]), "differing_elements": sum(t["differing"] for t in tally.values())}
            print(json.dumps(rec), flush=True)
            records.append(rec)
    return records


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--skip-bits", action="store_true")
    ap.add_argument("--skip-speed", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=21)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_loss_fold.json"))
    a = ap.parse_args()
    torch.zeros(1, device=DEV)                                          # torch's HIP runtime is resident before either library
    parent, new = load(a.parent, PARENT_PROTOS), load(a.new, NEW_PROTOS)
    rec = {"metric": "policy_loss_fold", "label": a.label, "device": torch.cuda.get_device_name(0)}
    if not a.skip_bits:
        rec["bits"] = run_bits(parent, new)
        print(json.dumps(rec["bits"]), flush=True)
    if not a.skip_speed:
        rec["speed"] = {"rounds": a.rounds, "samples_per_round": a.samples, "calls_per_sample": a.calls,
                        "records": run_speed(parent, new, a.rounds, a.samples, a.calls)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
