"""CPU checks of tests/logprob_ref64.py, the float64 references and per-element bounds of the log-prob / entropy kernels:

* a torch fp32 EMULATION of the kernels' arithmetic (256 lanes of 8-element vectors, per-lane online (m, s, t), the scalar tail, the
  butterfly and four-wave merges, the storage roundings, the rounded extra-pick update; every exp2 / log2 / rcp result moved by one ulp
  in a random direction, so the emulation is no better than the hardware) stays inside every bound on the shared input generators and
  reaches the 0.99 a single 2-byte rounding must reach;
* the references agree with oracle/model_oracle.logprobs_entropy_of, with float64 autograd and with tests/golden/logprob_cases.pt;
* named corruptions of the emulation are rejected by the bounds; for each the test computes whether the tolerance of
  test_gpu_logprob.py::test_kernels_vs_oracle (values 2e-5 / 5e-5 (1 + max|ref|), gradient one Frobenius norm at 1e-2 in bf16) accepts it.
"""
import math
import os

import numpy as np
import pytest
import torch

import logprob_ref64 as L
from oracle import model_oracle as mo

F32, BF, F16 = torch.float32, torch.bfloat16, torch.float16
GOLD = os.path.join(os.path.dirname(__file__), "golden")
LOG2E_F, LN2_F = np.float32(1.4426950408889634), np.float32(0.6931471805599453)
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the emulation
class HW:
    """exp2 / log2 / rcp as the hardware's 1-ulp instructions: the correctly rounded result moved one ulp in a random direction."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def _jog(self, exact):
        """`exact`: the float64 result.  One that fp32 represents exactly (2^integer, 1 / 2^n, 0, inf) is returned as it is."""
        r = exact.float()
        up = torch.rand(r.shape, generator=self.g) < 0.5
        j = torch.nextafter(r, torch.where(up, torch.full_like(r, INF), torch.full_like(r, -INF)))
        return torch.where((r.double() == exact) | torch.isinf(r), r, j)

    def ex2(self, a):
        return self._jog(torch.exp2(a.double()))

    def lg2(self, a):
        return self._jog(torch.log2(a.double()))

    def rcp(self, a):
        return self._jog(1.0 / a.double())


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def f32(v):
    return torch.tensor(float(v), dtype=F32)


def _consts(T, cap):
    inv = f32(1.0) / f32(T)
    k = f32(LOG2E_F) * inv
    kt, cs = None, f32(1.0)
    if cap > 0:
        kt, cs = f32(2.0) * f32(LOG2E_F) / f32(cap), f32(cap)
        k = k * cs
    return inv, k, kt, cs


def _tanh(hw, a):
    return fma(torch.full_like(a, -2.0), hw.rcp(1.0 + hw.ex2(a)), torch.ones_like(a))


def _merge(hw, a, b):
    m = torch.maximum(a[0], b[0])
    fa, fb = hw.ex2(a[0] - m), hw.ex2(b[0] - m)
    return m, a[1] * fa + b[1] * fb, a[2] * fa + b[2] * fb


def emu_fwd(x, labels, ptr, exl, T, cap, hw, stats=False, corrupt=None):
    """-> dict of fp32 outputs as the kernel forms them (lse, entropy, logprob, extra_logprob - or stats [R, 4], extra_picked)."""
    R, V = x.shape
    inv, k, kt, cs = _consts(T, cap)
    xf = x.float()
    tt = _tanh(hw, xf * kt) if cap > 0 else None
    y = tt * k if cap > 0 else xf * k
    fin = (lambda v: v) if cap > 0 else (lambda v: torch.maximum(v, f32(L.MASKED_Y)))      # the factor of p in t (the kernel's `finite`)
    nv = V >> 3
    passes = -(-nv // 256)
    m, s, t = torch.full((R, 256), -1e30), torch.zeros(R, 256), torch.zeros(R, 256)
    Y = torch.full((R, passes * 256 * 8), -1e30)
    Y[:, :nv * 8] = y[:, :nv * 8]
    Y = Y.view(R, passes, 256, 8)
    lane = torch.arange(256)
    for ps in range(passes):
        yy = Y[:, ps]
        valid = (ps * 256 + lane < nv)[None, :]
        mn = torch.maximum(m, yy.max(-1).values)
        f = hw.ex2(m - mn)
        s2, t2 = s * f, (t if corrupt == "t_no_rescale" else t * f)
        for j in range(8):
            p = hw.ex2(yy[..., j] - mn)
            s2, t2 = s2 + p, fma(p, fin(yy[..., j]), t2)
        m, s, t = torch.where(valid, mn, m), torch.where(valid, s2, s), torch.where(valid, t2, t)
    nt = V - nv * 8
    if nt:
        yt = torch.full((R, 256), -1e30); yt[:, :nt] = y[:, nv * 8:]
        valid = (lane < nt)[None, :]
        mn = torch.maximum(m, yt)
        f, p = hw.ex2(m - mn), hw.ex2(yt - mn)
        s2 = s * f + p
        t2 = fma(p, fin(yt), t if corrupt == "t_no_rescale" else t * f)
        m, s, t = torch.where(valid, mn, m), torch.where(valid, s2, s), torch.where(valid, t2, t)
    if corrupt == "lane_out":
        m[:, 5], s[:, 5], t[:, 5] = -1e30, 0.0, 0.0
    v = tuple(a.view(R, 4, 64) for a in (m, s, t))
    for o in (32, 16, 8, 4, 2, 1):
        idx = torch.arange(64) ^ o
        v = _merge(hw, v, tuple(a[..., idx] for a in v))
    r = tuple(a[:, 0, 0] for a in v)
    for w in range(1, 4):
        r = _merge(hw, r, tuple(a[:, w, 0] for a in v))
    m, s, t = r

    def pick(rows_, labs):
        ok = (labs >= 0) & (labs < V)
        li = labs.clamp(0, V - 1)
        val = (cs * tt[rows_, li] * inv) if cap > 0 else xf[rows_, li] * inv
        return val, ok

    out = {}
    ar = torch.arange(R)
    if ptr is not None:
        f0, f1, rw = L._extra_rows(ptr, R, "cpu")
    if stats:
        lab = labels if labels is not None else torch.full((R,), -1)
        val, ok = pick(ar, lab)
        out["stats"] = torch.stack([m, s, t, torch.where(ok, val, torch.zeros(()))], -1)
        if ptr is not None:
            val, ok = pick(rw, exl[f0:f1])
            out["extra_picked"] = torch.where(ok, val, torch.zeros(()))
        return out
    l = (m + hw.lg2(s)) * f32(LN2_F)
    out["lse"], out["entropy"] = l, l - (t / s) * f32(LN2_F)
    if labels is not None:
        val, ok = pick(ar, labels)
        out["logprob"] = torch.where(ok, val - l, torch.zeros(()))
    if ptr is not None:
        val, ok = pick(rw, exl[f0:f1])
        out["extra_logprob"] = torch.where(ok, val - l[rw], torch.zeros(()))
    return out


def _store(g, dtype, trunc=False):
    if trunc and dtype == BF:
        return (g.view(torch.int32) & -65536).view(F32).to(BF)
    return g.to(dtype)


def emu_bwd(x, labels, ptr, exl, lse, ent, glp, gex, gent, T, cap, hw, corrupt=None):
    """-> dlogits in x's dtype, as the kernel forms it out of place."""
    R, V = x.shape
    dtype = x.dtype
    inv, k, kt, cs = _consts(T, cap)
    zero = torch.zeros(R)
    l, en = lse.float(), (ent.float() if ent is not None else zero)
    if corrupt == "ent_neighbour":
        en = en.roll(1)
    ge, g1 = (gent.float() if gent is not None else zero), (glp.float() if glp is not None else zero)
    G = g1.clone()
    if ptr is not None:
        p_ = ptr.long()
        for r in range(R):
            for f in range(int(p_[r]), int(p_[r + 1])):
                G[r] = G[r] + gex[f]
    a = -G + ge * (l - en)
    l2 = (l * f32(LOG2E_F))[:, None]
    c2 = -ge * inv * inv
    if cap > 0:
        c2 = c2 * cs
    c1, gl = a * inv, g1 * inv
    xf = x.float()
    if cap > 0:
        xf = _tanh(hw, xf * kt)
        sech2 = fma(-xf, xf, torch.ones_like(xf))
    p = hw.ex2(fma(xf, k.expand_as(xf), -l2.expand_as(xf)))
    if cap <= 0:
        xf = torch.maximum(xf, f32(L.MASKED_Y))
    nv8 = (V >> 3) << 3
    lab = labels if labels is not None else torch.full((R,), -1)
    # the vector part
    g = p * fma(xf, c2[:, None].expand_as(xf), c1[:, None].expand_as(xf))
    for r in range(R):
        lb = int(lab[r])
        if 0 <= lb < nv8:
            g[r, lb ^ 1 if corrupt == "label_lane" else lb] += gl[r]
    if cap > 0:
        g = g * sech2
    # the scalar tail
    if V > nv8:
        xt = xf[:, nv8:]
        gt = p[:, nv8:] * (a[:, None] - ge[:, None] * (xt * cs * inv))
        for r in range(R):
            if nv8 <= int(lab[r]) < V:
                gt[r, int(lab[r]) - nv8] += g1[r]
        if cap > 0:
            gt = gt * sech2[:, nv8:]
        g = torch.cat([g[:, :nv8], gt * inv], -1)
    if corrupt == "scale":
        g = g * 1.005
    o = _store(g, dtype, corrupt == "trunc")
    if corrupt == "tail_zero":
        o[:, nv8:] = 0
    if ptr is not None:
        for r in range(R):
            for i, f in enumerate(range(int(p_[r]), int(p_[r + 1]))):
                le = int(exl[f])
                if not 0 <= le < V or (corrupt == "drop_pick" and i == 150):
                    continue
                w = sech2[r, le] if cap > 0 else f32(1.0)
                o[r, le] = _store(o[r, le].float() + gex[f] * inv * w, dtype, corrupt == "trunc")
    return o


# ------------------------------------------------------------------------------------------------ a case
def _case(kind, R, V, dtype, seed, per_row=7, shift=0):
    g = torch.Generator().manual_seed(seed + 17)
    x = L.rows(kind, R, V, dtype, seed)
    labels = L.labels_for(R, V, shift)
    ptr, exl = L.extras(R, V, labels, per_row, seed)
    glp, gent = torch.randn(R, generator=g), torch.randn(R, generator=g)
    gex = torch.randn(exl.numel(), generator=g)
    return x, labels, ptr, exl, glp, gex, gent


def _run(x, labels, ptr, exl, glp, gex, gent, T, cap, seed=0, corrupt=None):
    """The emulated forward, statistics and backward against the bounds -> {output: worst err / bound}."""
    hw = HW(seed)
    fw = emu_fwd(x, labels, ptr, exl, T, cap, hw, corrupt=corrupt)
    res = L.check_all("emu", fw, L.fwd_ref(x, labels, ptr, exl, T, cap))
    st = emu_fwd(x, labels, ptr, exl, T, cap, hw, stats=True, corrupt=corrupt)
    view = L.stats_view(st["stats"]); view["extra_picked"] = st.get("extra_picked")
    res.update(L.check_all("emu.stats", view, L.stats_ref(x, labels, ptr, exl, T, cap)))
    dl = emu_bwd(x, labels, ptr, exl, fw["lse"], fw["entropy"], glp, gex, gent, T, cap, hw, corrupt=corrupt)
    res.update(L.check_all("emu", {"dlogits": dl}, L.bwd_ref(x, labels, ptr, exl, fw["lse"], fw["entropy"], glp, gex, gent, T, cap)))
    return res, fw, dl


@pytest.mark.parametrize("cap", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("dtype", [BF, F16, F32])
def test_emulation_stays_inside_every_bound(dtype, cap):
    """Every row kind at V = 7 (tail only), 264 and 2061 (a full pass, a partial second one and a tail), T in {0.25, 1, 4}."""
    worst = {}
    for i, (kind, V) in enumerate((k, v) for k in L.KINDS for v in (7, 264, 2061)):
        T = L.large_temp(dtype) if kind == "large" else (0.25, 1.0, 4.0)[i % 3]
        res, _, _ = _run(*_case(kind, 3, V, dtype, 100 + i, shift=i), T, cap, seed=i)
        for n, v in res.items():
            worst[n] = max(worst.get(n, 0.0), v)
    print("\nWORST emulation", str(dtype).split(".")[-1], cap, {n: round(v, 3) for n, v in sorted(worst.items())})
    assert all(v <= 1.0 for v in worst.values())
    if dtype != F32:
        # u is the exact worst case of ONE rounding (an element just above a power of two, half an ulp away): bf16 meets it within a
        # few thousand elements (0.99), f16 with its 8 times finer grid less closely (0.93)
        assert worst["dlogits"] >= 0.9, "the 2-byte bound is tight: a single correct rounding nearly reaches it"


@pytest.mark.parametrize("cap", [0.0, 30.0])
@pytest.mark.parametrize("dtype", [BF, F16, F32])
def test_emulation_of_masked_columns(dtype, cap):
    """-inf columns and finite ones whose scaled value overflows: exactly 0 gradient, everything else as the row without them."""
    for where, n, value in (("vector", 1, None), ("vector", 40, None), ("tail", 1, None), ("vector", 40, float(torch.finfo(dtype).min))):
        x, labels, ptr, exl, glp, gex, gent = _case("randn", 2, 2061, dtype, 7, per_row=0)
        x, cols = L.mask_columns(x, n, where, value)
        labels = torch.tensor([5, 2048 + 13])
        res, fw, dl = _run(x, labels, None, None, glp, None, gent, 1.0, cap)
        assert bool((dl[:, cols] == 0).all()) and bool(torch.isfinite(dl).all())
        if cap == 0:
            keep = torch.ones(2061, dtype=torch.bool); keep[cols] = False
            small = L.fwd_ref(x[:, keep], None, None, None, 1.0)
            assert torch.equal(small["lse"][0], L.fwd_ref(x, None, None, None, 1.0)["lse"][0])
            L.check("emu.lse", fw["lse"], *small["lse"]); L.check("emu.entropy", fw["entropy"], *small["entropy"])


# ------------------------------------------------------------------------------------------------ agreement with the other references
def test_references_agree_with_the_oracle_and_float64_autograd():
    for (R, V, T, cap, dtype) in ((5, 301, 0.7, 0.0, F32), (4, 264, 1.3, 0.0, BF), (3, 77, 0.7, 3.0, F32)):
        x, labels, ptr, exl, glp, gex, gent = _case("randn", R, V, dtype, R + V)
        labels = labels.clamp(0, V - 1)
        fr = L.fwd_ref(x, labels, ptr, exl, T, cap)
        if not cap:
            lp_o, ent_o = mo.logprobs_entropy_of(x.float(), labels, T)
            assert (lp_o.double() - fr["logprob"][0]).abs().max() <= 1e-5 * (1 + fr["logprob"][0].abs().max())
            assert (ent_o.double() - fr["entropy"][0]).abs().max() <= 1e-5 * (1 + fr["entropy"][0].abs().max())
        xd = x.double().requires_grad_(True)
        Tf = L.temp32(T)
        xc = (cap * torch.tanh(xd / cap) if cap else xd) / Tf
        lse = torch.logsumexp(xc, -1)
        lpa = xc - lse[:, None]
        ent = -(lpa.exp() * lpa).sum(-1)
        rw = torch.repeat_interleave(torch.arange(R), (ptr[1:] - ptr[:-1]).long())
        ok = (exl >= 0) & (exl < V)
        # a pick outside [0, V) is somebody else's: 0 in the forward, and its gradient still acts through -lse (the kernels' contract)
        lp2 = xc[rw, exl.clamp(0, V - 1)] * ok - lse[rw]
        lp = lpa[torch.arange(R), labels]
        for got, want in ((fr["lse"][0], lse), (fr["entropy"][0], ent), (fr["logprob"][0], lp), (fr["extra_logprob"][0], lp2 * ok)):
            assert (got - want.detach()).abs().max() <= 1e-12 * (1 + want.detach().abs().max())
        ((lp * glp.double()).sum() + (lp2 * gex.double()).sum() + (ent * gent.double()).sum()).backward()
        br = L.bwd_ref(x, labels, ptr, exl, lse.detach(), ent.detach(), glp, gex, gent, T, cap)["dlogits"]
        assert (br[0] - xd.grad).abs().max() <= 1e-12 * (1 + xd.grad.abs().max())
        assert bool((br[1] > 0).all()) and bool(torch.isfinite(br[1]).all())


def test_references_agree_with_the_recorded_golden_cases():
    gold = torch.load(os.path.join(GOLD, "logprob_cases.pt"), weights_only=True)
    for name, c in gold.items():
        g = torch.Generator().manual_seed(c["seed"])
        logits = torch.randn(c["R"], c["V"], generator=g) * 3
        labels = torch.randint(0, c["V"], (c["R"],), generator=g)
        go_lp, go_ent = torch.randn(c["R"], generator=g), torch.randn(c["R"], generator=g)
        fr = L.fwd_ref(logits, labels, None, None, c["temp"])
        assert (fr["logprob"][0] - c["logprobs"]).abs().max() <= 2e-5 * (1 + c["logprobs"].abs().max()), name
        assert (fr["entropy"][0] - c["entropy"]).abs().max() <= 5e-5 * (1 + c["entropy"].abs().max()), name
        g1 = L.bwd_ref(logits, labels, None, None, fr["lse"][0], None, go_lp, None, None, c["temp"])["dlogits"][0]
        g2 = L.bwd_ref(logits, None, None, None, fr["lse"][0], fr["entropy"][0], None, None, go_ent, c["temp"])["dlogits"][0]
        assert torch.allclose(g1[:, :48].float(), c["grad_lp_head"], atol=5e-6, rtol=1e-4), name
        assert torch.allclose(g2[:, :48].float(), c["grad_ent_head"], atol=5e-6, rtol=1e-4), name


# ------------------------------------------------------------------------------------------------ corruptions
def _old_accepts(x, labels, ptr, exl, glp, gex, gent, T, fw, dl):
    """Would test_gpu_logprob.py::test_kernels_vs_oracle accept these outputs?  Its tolerances, against float64."""
    fr = L.fwd_ref(x, labels, ptr, exl, T)
    tol = {BF: 1e-2, F16: 2e-3, F32: 2e-5}[x.dtype]
    ok = True
    for n, c in (("logprob", 2e-5), ("extra_logprob", 2e-5), ("entropy", 5e-5)):
        if n in fw:
            ok &= bool((fw[n].double() - fr[n][0]).abs().max() <= c * (1 + fr[n][0].abs().max()))
    ref = L.bwd_ref(x, labels, ptr, exl, fr["lse"][0], fr["entropy"][0], glp, gex, gent, T)["dlogits"][0]
    return ok and float((dl.double() - ref).norm() / ref.norm()) <= tol


# corruption -> (case, does the old tolerance accept it).  The first two are the gap measured in the issue: accepted before, rejected now.
CORRUPTIONS = {
    "trunc": (("randn", 37, 64, BF, 300), True),
    "tail_zero": (("randn", 2, 151936 + 5, BF, 7), True),
    "scale": (("randn", 5, 301, BF, 7), True),
    "label_lane": (("randn", 5, 301, BF, 7), False),
    "drop_pick": (("randn", 2, 2061, BF, 300), False),
    "lane_out": (("flat", 3, 2061, BF, 7), False),
    "ent_neighbour": (("randn", 5, 301, BF, 7), False),
}


@pytest.mark.parametrize("name", list(CORRUPTIONS))
def test_bounds_reject_the_corruption(name):
    (kind, R, V, dtype, per_row), old = CORRUPTIONS[name]
    x, labels, ptr, exl, glp, gex, gent = _case(kind, R, V, dtype, 11, per_row=per_row)
    labels = labels.clamp(0, V - 1)
    if name == "label_lane":
        labels = labels.clamp(0, 8 * (V // 8) - 1)
    hw = HW(3)
    fw = emu_fwd(x, labels, ptr, exl, 1.0, 0.0, hw)
    dl = emu_bwd(x, labels, ptr, exl, fw["lse"], fw["entropy"], glp, gex, gent, 1.0, 0.0, hw)
    assert _old_accepts(x, labels, ptr, exl, glp, gex, gent, 1.0, fw, dl), "the honest emulation passes the old tolerance"
    _run(x, labels, ptr, exl, glp, gex, gent, 1.0, 0.0, seed=3)                      # ... and the bounds
    hw = HW(3)
    fwc = emu_fwd(x, labels, ptr, exl, 1.0, 0.0, hw, corrupt=name)
    dlc = emu_bwd(x, labels, ptr, exl, fw["lse"], fw["entropy"], glp, gex, gent, 1.0, 0.0, hw, corrupt=name)
    accepted = _old_accepts(x, labels, ptr, exl, glp, gex, gent, 1.0, fwc, dlc)
    print(f"\ncorruption {name}: the old tolerance {'ACCEPTS' if accepted else 'rejects'} it; the bounds reject it")
    assert accepted == old
    with pytest.raises(AssertionError):
        L.check_all("emu", fwc, L.fwd_ref(x, labels, ptr, exl, 1.0))
        L.check_all("emu", {"dlogits": dlc}, L.bwd_ref(x, labels, ptr, exl, fw["lse"], fw["entropy"], glp, gex, gent, 1.0))


def test_bounds_reject_unrescaled_t_in_the_shard_statistics():
    """stats.t not rescaled when a lane's maximum moves (the ascending row moves it at every step).  Before, the raw statistics were
    seen only through two ranks at 2e-3 (1 + max|ref|) on the combined values: computed here for the combined entropy."""
    x = L.rows("asc", 2, 4104, BF, 1)
    hw = HW(1)
    ref = L.stats_ref(x, None, None, None, 1.0)
    good = emu_fwd(x, None, None, None, 1.0, 0.0, hw, stats=True)["stats"]
    L.check_all("emu.stats", L.stats_view(good), ref)
    bad = emu_fwd(x, None, None, None, 1.0, 0.0, hw, stats=True, corrupt="t_no_rescale")["stats"]
    ent_ref = L.fwd_ref(x, None, None, None, 1.0)["entropy"][0]
    ent_bad = (bad[:, 0].double() + torch.log2(bad[:, 1].double())) * L.LN2 - bad[:, 2].double() / bad[:, 1].double() * L.LN2
    accepted = bool((ent_bad - ent_ref).abs().max() <= 2e-3 * (1 + ent_ref.abs().max()))
    print(f"\ncorruption t_no_rescale: the old tolerance {'ACCEPTS' if accepted else 'rejects'} it; the bounds reject it")
    assert not accepted
    with pytest.raises(AssertionError):
        L.check_all("emu.stats", L.stats_view(bad), ref)
