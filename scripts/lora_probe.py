#!/usr/bin/env python3
"""The three LoRA kernels (csrc/lora_kernels.hip) against the torch / hipBLASLt expression each replaces, at the bench shapes: T = 28 160
packed rows; K, N of the Qwen3-0.6B and Qwen3-8B projections; r in {8, 16, 64}; bf16, random operands.

    down     ops.lora_down(x, A)                 vs  x @ A.t()
    up_add   the in-place MFMA kernel of scripts/diag/lora_up_add_experiment.hip (an experiment, not in the product; measured when
             its library has been built - the command is in that file)   vs  y.addmm_(xa, B.t(), alpha=s), which the product ships
    wgrad    ops.lora_wgrad(dxa, x, dtype)       vs  dxa.t() @ x   and   ops._wgrad(x, dxa, False)  (the manual split-K form)

Kernel and expression alternate in ONE process after a warm-up of every shape; each figure is the median over `reps` device-event
timings of `inner` back-to-back calls.  bytes/s: the algorithmic bytes of the product (one read of every input, one write of every
output; up_add reads and writes y) over that time, and its share of 6.29 TB/s - the MEASURED copy rate of this card (not the HBM peak).
Usage: python scripts/lora_probe.py [out.json] [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes

import numpy as np
import torch
from dynamictreeattn_amd import ops
from dynamictreeattn_amd._lib import lib as _product_lib

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lora_probe.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
inner = 10
dev = torch.device("cuda:0")
BF = torch.bfloat16
T = 28160
COPY_RATE = 6.29e12
# the K (input) and N (output) extents of the fused projection groups: q|k|v, o, gate|up, down
GEOM = {"Qwen3-0.6B": {"qkv": (1024, 4096), "o": (2048, 1024), "gate_up": (1024, 6144), "down": (3072, 1024)},
        "Qwen3-8B": {"qkv": (4096, 6144), "o": (4096, 4096), "gate_up": (4096, 24576), "down": (12288, 4096)}}
RANKS = (8, 16, 64)
g = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, device=dev, generator=g)).to(BF)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def compare(forms):
    for fn in forms.values():               # warm-up: code objects, hipBLASLt solution choice
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():         # alternating
            ms[k].append(timed(fn))
    return {k: sorted(v)[len(v) // 2] for k, v in ms.items()}


_product_lib()                                # the product library first: one HIP runtime (torch's) for everything loaded after it
UP_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diag", "liblora_up_add_experiment.so")
up_fn = None
if os.path.exists(UP_LIB):
    up_fn = ctypes.CDLL(UP_LIB).lora_up_add_experiment
    up_fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    up_fn.restype = ctypes.c_int


def up_add_experiment(y, xa, m, scale):
    seg = np.asarray([0, y.shape[1], 0, xa.shape[1]], np.int32)
    sc = np.asarray([scale], np.float32)
    st = up_fn(y.data_ptr(), y.stride(0), xa.data_ptr(), xa.stride(0), m.data_ptr(), m.stride(0), 1, seg.ctypes.data, sc.ctypes.data,
               y.shape[0], y.shape[1], torch.cuda.current_stream().cuda_stream)
    assert st == 0, st


rows = []
extents = sorted({e for geo in GEOM.values() for kn in geo.values() for e in kn})
for E in extents:
    x = rnd(T, E)
    y = rnd(T, E)
    for r in RANKS:
        A, B = rnd(r, E, scale=0.05), rnd(E, r, scale=0.05)
        xa, dxa = rnd(T, r), rnd(T, r)
        used = [f"{m}:{p}" for m, geo in GEOM.items() for p, kn in geo.items() if E in kn]
        t = compare({"kernel": lambda: ops.lora_down(x, A), "torch": lambda: x @ A.t()})
        nbytes = 2 * (T * E + r * E + T * r)
        rows.append({"op": "down", "K": E, "r": r, "ms": t, "bytes": nbytes, "used_by": used})
        if up_fn is not None:
            ya, yb = y.clone(), y.clone()
            up_add_experiment(ya, xa, B, 2.0); yb.addmm_(xa, B.t(), alpha=2.0)
            assert float((ya.float() - yb.float()).abs().max()) <= 2.0 ** -6 * float(yb.float().abs().max()), "the experiment computes something else"
            del ya, yb
            t = compare({"kernel": lambda: up_add_experiment(y, xa, B, 2.0), "torch": lambda: y.addmm_(xa, B.t(), alpha=2.0)})
            nbytes = 2 * (2 * T * E + r * E + T * r)
            rows.append({"op": "up_add", "N": E, "r": r, "ms": t, "bytes": nbytes, "used_by": used, "kernel_is": "scripts/diag experiment, not shipped"})
            y.copy_(rnd(T, E))                  # the timed calls accumulated into y: fresh values before the next rank
        t = compare({"kernel": lambda: ops.lora_wgrad(dxa, x, BF), "torch": lambda: dxa.t() @ x, "split_k": lambda: ops._wgrad(x, dxa, False)})
        nbytes = 2 * (T * E + T * r + r * E)
        rows.append({"op": "wgrad", "K": E, "r": r, "ms": t, "bytes": nbytes, "used_by": used})
    del x, y
for row in rows:
    k = row["ms"]["kernel"]
    row["ms"] = {n: round(v, 4) for n, v in row["ms"].items()}
    row["kernel_TB_per_s"] = round(row["bytes"] / (k * 1e-3) / 1e12, 2)
    row["kernel_share_of_copy_rate"] = round(row["bytes"] / (k * 1e-3) / COPY_RATE, 3)
    row["kernel_speedup_vs_best_other"] = round(min(v for n, v in row["ms"].items() if n != "kernel") / k, 2)
summary = {}
for op in ("down", "up_add", "wgrad"):
    s = [r_["kernel_speedup_vs_best_other"] for r_ in rows if r_["op"] == op]
    if not s:
        summary[op] = "not measured (build scripts/diag/lora_up_add_experiment.hip)"
        continue
    summary[op] = {"min_speedup": min(s), "max_speedup": max(s), "kernel_at_least_as_fast_everywhere": min(s) >= 1.0,
                   "kernel_loses_everywhere": max(s) < 1.0}
for row in rows:
    if row["op"] == "down":
        row["product_uses"] = "kernel" if ops._down_by_kernel(row["K"], 32 * -(-row["r"] // 32)) else "torch"
    elif row["op"] == "wgrad":
        row["product_uses"] = "kernel" if ops._wgrad_by_kernel(row["K"]) else "torch (fp32-output GEMM)"
    else:
        row["product_uses"] = "torch (addmm_)"
res = {"T": T, "dtype": "bf16", "reps": reps, "inner": inner, "denominator": "6.29 TB/s measured copy rate", "device": torch.cuda.get_device_name(0),
       "summary": summary, "rows": rows}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print(json.dumps(summary))
