"""Float64 restatement of the log-prob / entropy kernels of csrc/logprob_kernels.hip (dta_logprob_entropy_fwd, _shard_stats, _bwd; plain
and soft-capped, with a temperature, extra picks as a CSR with absolute indices, labels outside [0, V)) and a per-element error bound for
every output.

The references take the kernels' ROUNDED inputs and, in the backward, the fp32 lse / entropy the kernel really receives, so an error of
the forward is not charged to the backward again.  Contract for a label outside [0, V) (dta.h; -1 = owned by another rank): the forward
yields 0; in the backward g_logprob still acts through -lse and only the one-hot term is absent.  Masked columns (plain form): a logit of
-inf, or one whose scaled value is below -1e30 (it overflows fp32), has probability 0, adds nothing to any statistic and gets a gradient of
exactly 0; a label on a -inf column yields logprob = -inf.  Under a cap a -inf logit is x' = -c like any other very negative one; its
gradient is exactly 0 through 1 - tanh^2 = 0.

Notation.  u32 = 2^-24 (one fp32 rounding), u = U[dtype] (one rounding to the storage type), T the temperature as a float, x' = x or
c tanh(x / c), y = x' log2(e) / T the scaled logit (log2 domain), M = max y, p = 2^(y - M) / s, E_p[.] the mean under p.  Every bound
is a sum of the following named steps of the kernel's arithmetic.

  scaled logit   y = fl(x k), k = fl(log2e * fl(1 / T)) (capped: times c once more): the float log2(e) (0.22 u32), 1 / T, the product k
                 and the product x k: dy = KY u32 |y|, KY = 3.25 (4.25 capped).  It moves 2^y by the relative ln 2 dy: the |y| term that
                 carries large logits - nothing else in the bounds grows with the magnitude of the row.
  tanh           t = 1 - 2 / (1 + 2^a), a = fl(x fl(2 log2e / c)): the error of 2^a (ln 2 KA |a| + 2) u32 enters with (1 - t^2) / 2, the
                 sum 1 + 2^a and the 1-ulp reciprocal with 3 (1 - t), the last fma with |t|:  dt.  It adds (c log2e / T) dt to dy,
                 (c / T) dt to a pick, and 1 - t^2 (one fma) is off by 2 |t| dt + u32 (1 - t^2) - absolutely: for |x| >> c it cancels.
  exp2 / log2    the hardware's 1-ulp exp2 and log2: 2 u32 relative each.  The exponent y - m is rounded: ln 2 u32 |y - m|.
  online rescale a lane's (s, t) are multiplied by 2^(m_old - m_new) whenever its maximum moves: exp2, the product and the rounded exponent
                 difference.  The differences an element sees on its way to M sum to at most M - y: a second ln 2 u32 |y - M|; the other two
                 cost 3 u32 per step, `steps` = ceil(V / 8 / 256) (+ 1 with a tail) at the most (the ascending row: at every step).
  merge tree     six butterfly steps and three wave merges, each a rescale of both sides and one addition: 3 u32 each, nm = 9.
  sums           a lane adds n = 8 ceil(V / 8 / 256) + 1 positive terms, the tree nm more: C32 sqrt(n + nm) u32 (the statistical growth of
                 ref64_common.bound).  Together: an element's weight is off by the relative w u32,
                     w = ln 2 (dy / u32 + 2 |y - M|) + 2 + C32 sqrt(n + nm) + 3 (steps + nm).
  lse            ln 2 (m + log2 s): rel(s) = u32 E_p[w], log2 (2 u32 |log2 s|), the sum and the product (3 u32 |lse|).
  entropy        lse - ln 2 t / s, a difference of large terms, bounded on the magnitudes BEFORE the cancellation: t / s is off by
                 u32 (E_p[|y| (w + 1)] + E_p[dy / u32] + |t / s| (E_p[w] + 2)); the subtraction rounds |lse| + ln 2 |t / s| (2 u32).
  picks          x'[label] / T: the product by fl(1 / T), 2 u32 (+ (c / T) dt); logprob = pick - lse adds the bound of lse and u32 |logprob|.
  stats          scale-free: m against M (dy at the maximum), m + log2 s against log2 sum 2^y, t / s against E_p[y], picked raw.
  backward       p = exp2(fma(x', k, -fl(lse log2e))): relative ln 2 (dy - u32 |y| + u32 |y - l2| + 1.25 u32 |l2|) + 2 u32.
                 a = -G + ge (lse - ent): G a chain of ne + 1 additions (C32 sqrt(ne + 1) u32 sum |g|), the difference lse - ent bounded
                 absolutely on |lse| + |ent| (2 u32 |ge| of it) and the last sum (u32 of all magnitudes): da.  h = a - ge x' / T, formed as
                 fma(x', c2, c1): da + 6 u32 (|a|_mag + |ge x' / T|) (+ |ge| (c / T) dt).  g = (p h + [label] g1) / T: 4 u32 more of each
                 term; capped: times 1 - t^2 with its absolute error.  An exp2 result under 2^-126 may be flushed: FLUSH (1 + |h|_mag) / T.
  dlogits        ONE rounding to the storage type: u |g| + TINY.
  extra picks    the kernel adds g_extra / T (times 1 - t^2) to the ALREADY ROUNDED element and rounds again: u |g_new| + 3 u32 |term|
                 more per pick, on top of u |g_old|.

No constant is fitted: every figure above is the count of a named step.

OBSERVED worst err / bound (bf16 / f16 / fp32 storage).  CPU emulation of tests/test_logprob_ref64.py (every exp2 / log2 / rcp one ulp off):
    dlogits .992/.940/.721   lse .31/.24/.45   entropy .15/.14/.13   logprob .42/.34/.35   extra_logprob .48/.45/.47
    stats: m .82/.82/.82   m + log2 s .31/.28/.25   t / s .04/.04/.04   picked .72/.82/.73 (capped; plain: 0, one exact product)
The 2-byte dlogits figures sit at 0.99 (bf16) because u is the exact worst case of ONE rounding (an element just above a power of two,
half an ulp away); f16's finer grid meets it less closely over these sizes.  What is left for the fp32 part shows in the fp32 column.
MI355X, over tests/test_gpu_logprob_bounds.py (the WORST lines it prints):
    plain     dlogits .995/.985/.898   lse .19/.23/.20   entropy .08/.07/.08   logprob .23/.20/.28   extra_logprob .23/.22/.28
              stats: m .31/.36/.33   m + log2 s .09/.08/.06   t / s .03/.03/.03   picked .12/.13/.12   extra_picked .28/.27/.45
    capped    dlogits .990/.966/.965   lse .21/.17/.21   entropy .08/.10/.12   logprob .20/.22/.17   extra_logprob .19/.19/.21
              stats: m .23/.29/.28   m + log2 s .17/.16/.23   t / s .06/.06/.06   picked .40/.38/.34   extra_picked .47/.36/.38
    masked    dlogits .993/.966/.46    lse .14/.13/.15   entropy .02/.02/.02   against the row WITHOUT the columns: the same figures
    shards    m .29/.29/.32   m + log2 s .05/.05/.05   t / s .02/.02/.02   combined: lse .07/.11/.20   entropy .02/.02/.02   logprob .06/.10/.15
    public    ops.logprob_entropy dlogits .985/-/.42   ops.lm_head_rows dh .71 (bf16)
No derived constant proved short, so none carries a measured factor.  With fp32 storage the last rounding is itself one of the u32 terms,
so the fp32 dlogits column shows the fp32 part alone (.90 plain, .97 capped: closer to 1 than the statistics, whose bounds count every
loop step as a rescale); no output sits at 1.0.
"""
import math

import numpy as np
import torch

from ref64_common import C32, TINY, U, U32

LN2, LOG2E = math.log(2.0), 1.0 / math.log(2.0)
KY, KA = 3.25, 3.25
FLUSH = 2.0 ** -126
MASKED_Y = -1e30                 # the kernels hold the factor that multiplies p at this value (csrc/logprob_kernels.hip)
NM = 9
WORST: dict = {}
KINDS = ("randn", "peaked", "flat", "asc", "desc", "large")


def temp32(T):
    return float(np.float32(T))


def chain(V):
    """(n, steps): additions along one lane, and loop steps (rescales at the most) of one lane."""
    passes = -(-(V // 8) // 256)
    return 8 * passes + 1, passes + (1 if V % 8 else 0)


def _c_chain(V):
    n, steps = chain(V)
    return C32 * math.sqrt(n + NM) + 3.0 * (steps + NM)


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and GPU tests
def large_temp(dtype):
    """The temperature the "large" rows are meant for."""
    return 1.0 if dtype == torch.float16 else 0.25


def rows(kind, R, V, dtype, seed):
    """[R, V] logits rounded to `dtype`.  randn: N(0, 3).  peaked: N(0, 1) and one logit 30 .. 60 above (entropy ~ 0, most p underflow).
    flat: all equal (entropy ln V).  asc / desc: monotone along the vocabulary over 40 units (every lane rescales at every step / none
    does).  large: f16 +-(5e4 .. 6.5e4), near the type's maximum; otherwise +-1e4 (1 + 0.01 N) for T = 0.25."""
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        x = torch.randn(R, V, generator=g) * 3
    elif kind == "peaked":
        x = torch.randn(R, V, generator=g)
        for r in range(R):
            x[r, (r * 977 + V // 3) % V] += 30.0 + 30.0 * r / max(R - 1, 1)
    elif kind == "flat":
        x = torch.full((R, V), 1.5) * (1 + torch.arange(R)[:, None]) * torch.tensor([1.0, -1.0])[torch.arange(R) % 2][:, None]
    elif kind in ("asc", "desc"):
        x = torch.linspace(-20, 20, V)[None, :].repeat(R, 1) + torch.arange(R)[:, None]
        if kind == "desc":
            x = x.flip(-1)
    elif kind == "large":
        sgn = torch.where(torch.rand(R, V, generator=g) < 0.5, -1.0, 1.0)
        if dtype == torch.float16:
            x = sgn * (5e4 + 1.5e4 * torch.rand(R, V, generator=g))
        else:
            x = sgn * 1e4 * (1 + 0.01 * torch.randn(R, V, generator=g))
    else:
        raise ValueError(kind)
    return x.to(dtype)


def mask_columns(x, n, where, value=None):
    """A copy of x with n masked columns per row: where = "vector" (from column 3 on, stride 5 - inside the 8-element groups) or "tail"
    (the last V % 8 columns; n is cut to them).  value: -inf (default) or a finite logit whose scaled value overflows."""
    R, V = x.shape
    x = x.clone()
    v = -math.inf if value is None else value
    if where == "tail":
        cols = torch.arange(V - min(n, V % 8), V)
    else:
        cols = (3 + 5 * torch.arange(n)) % (V // 8 * 8)
    x[:, cols] = v
    return x, cols


def label_positions(V):
    """Label positions that reach every branch of the kernels at this V (kept inside [0, V)) and the two outside: -1 and V."""
    nv8 = 8 * (V // 8)
    inside = [0, 7, 8, nv8 - 1, nv8, V - 1, 2048 + (V - 2049) // 2 if V > 2048 else -5]     # the last: in the second pass
    return sorted({p for p in inside if 0 <= p < V}) + [-1, V]


def labels_for(R, V, shift=0):
    pos = label_positions(V)
    return torch.tensor([pos[(r + shift) % len(pos)] for r in range(R)], dtype=torch.int64)


def extras(R, V, labels, per_row, seed):
    """CSR (ptr int32 [R + 1], labels int64 [F]) with `per_row` picks on every row.  7: one equal to the row's own label (if inside), one
    in the tail (or the last column), one outside [0, V); the picks of a row are distinct tokens."""
    g = torch.Generator().manual_seed(seed)
    ptr, lab = [0], []
    for r in range(R):
        picks = torch.randperm(V, generator=g)[:per_row].tolist()
        if per_row == 7:
            own = int(labels[r]) if labels is not None else -1
            forced = [V - 1, V if r % 2 else -1] + ([own] if 0 <= own < V - 1 else [])
            picks = (forced + [p for p in picks if p not in forced])[:7]
        lab += picks
        ptr.append(len(lab))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(lab, dtype=torch.int64)


# ------------------------------------------------------------------------------------------------ the scaled logits
def _d(t):
    return t.detach().double()


def _scaled(x, T, cap):
    """x [R, V] -> dict: xs = x' / T (masked columns held finite), y, dy (absolute, log2 domain), masked, and with a cap sech2, dsech2,
    dt."""
    x64, Tf = _d(x), temp32(T)
    o = {"T": Tf}
    if cap and cap > 0:
        c = float(np.float32(cap))
        z = x64 / c
        t = torch.tanh(z)
        e2 = torch.exp(-2 * z.abs())
        sech2 = 4 * e2 / (1 + e2) ** 2
        a = (2 * LOG2E * z).abs().clamp(max=1e4)
        dt = U32 * (0.5 * sech2 * (LN2 * KA * a + 2) + 3 * (1 - t) + t.abs())
        xp = c * t
        y = xp * (LOG2E / Tf)
        o.update(sech2=sech2, dsech2=2 * t.abs() * dt + U32 * sech2, dt=dt, c=c, masked=torch.zeros_like(y, dtype=torch.bool))
        o["dy"] = U32 * (KY + 1) * y.abs() + (c * LOG2E / Tf) * dt
        o["dpick"] = (c / Tf) * dt + 3 * U32 * (xp / Tf).abs()
        o["xs"], o["xs_raw"] = xp / Tf, xp / Tf
    else:
        y = x64 * (LOG2E / Tf)
        masked = y < MASKED_Y
        o["masked"] = masked
        o["xs_raw"] = x64 / Tf                                          # -inf on a -inf column: what a pick of it yields
        o["xs"] = (x64.clamp(min=MASKED_Y)) / Tf
        y = torch.where(masked, torch.full_like(y, -math.inf), y)
        ys = torch.where(masked, torch.zeros_like(y), y)
        o["dy"] = U32 * KY * ys.abs()
        o["dpick"] = 2 * U32 * o["xs"].abs()
        o["c"] = 0.0
    o["y"] = y
    o["ys"] = torch.where(o["masked"], torch.zeros_like(y), y)       # y with 0 on masked columns, for the magnitudes
    return o


def _row_stats(sc, V):
    y, ys = sc["y"], sc["ys"]
    M = y.max(-1, keepdim=True).values
    q = torch.exp2(y - M)                                               # 0 on masked columns
    s = q.sum(-1, keepdim=True)
    p = q / s
    w = LN2 * (sc["dy"] / U32 + 2 * torch.where(sc["masked"], torch.zeros_like(y), (ys - M).abs())) + 2 + _c_chain(V)
    Ew = (p * w).sum(-1)
    L2 = (M + torch.log2(s)).squeeze(-1)
    E1 = (p * ys).sum(-1)
    rel_s = U32 * Ew
    b_L2 = rel_s / LN2 + U32 * (2 * torch.log2(s).abs().squeeze(-1) + L2.abs())
    b_E1 = U32 * ((p * ys.abs() * (w + 1)).sum(-1) + (p * sc["dy"]).sum(-1) / U32 + E1.abs() * (Ew + 2))
    near = (y >= M - 1.0)
    b_m = torch.where(near, sc["dy"], torch.zeros_like(y)).max(-1).values + 1e-300
    return dict(M=M.squeeze(-1), s=s.squeeze(-1), p=p, L2=L2, E1=E1, b_L2=b_L2, b_E1=b_E1, b_m=b_m)


def _pick(sc, rows_, labs, V):
    """(value, bound, ok) of x'[rows_, labs] / T; 0 where the label lies outside [0, V)."""
    ok = (labs >= 0) & (labs < V)
    li = labs.clamp(0, V - 1)
    val = torch.where(ok, sc["xs_raw"][rows_, li], torch.zeros((), dtype=torch.float64, device=li.device))
    bnd = torch.where(ok, sc["dpick"][rows_, li], torch.zeros((), dtype=torch.float64, device=li.device))
    bnd = torch.where(torch.isfinite(val), bnd, torch.zeros_like(bnd))
    return val, bnd, ok


def _extra_rows(extra_ptr, R, dev):
    """(f0, f1, row of every extra f0 .. f1) of a CSR with absolute offsets."""
    ptr = extra_ptr.long().cpu()
    f0, f1 = int(ptr[0]), int(ptr[R])
    rows_ = torch.repeat_interleave(torch.arange(R), ptr[1:] - ptr[:-1]).to(dev)
    return f0, f1, rows_


def fwd_ref(x, labels, extra_ptr, extra_labels, T, cap=0.0):
    """-> {"lse", "entropy", "logprob" (with labels), "extra_logprob" (with extras: entries extra_ptr[0] .. extra_ptr[R] only)}:
    (ref, bound)."""
    R, V = x.shape
    sc = _scaled(x, T, cap)
    st = _row_stats(sc, V)
    lse = LN2 * st["L2"]
    b_lse = LN2 * st["b_L2"] + 2 * U32 * lse.abs()
    ent = lse - LN2 * st["E1"]
    b_ent = b_lse + LN2 * st["b_E1"] + 2 * U32 * (lse.abs() + LN2 * st["E1"].abs())
    out = {"lse": (lse, b_lse), "entropy": (ent, b_ent)}
    ar = torch.arange(R, device=x.device)
    if labels is not None:
        val, bnd, ok = _pick(sc, ar, labels, V)
        lp = torch.where(ok, val - lse, torch.zeros_like(lse))
        out["logprob"] = (lp, torch.where(ok & torch.isfinite(lp), bnd + b_lse + U32 * lp.abs(), torch.zeros_like(lse)) + 1e-300)
    if extra_ptr is not None:
        f0, f1, rw = _extra_rows(extra_ptr, R, x.device)
        val, bnd, ok = _pick(sc, rw, extra_labels[f0:f1], V)
        lp = torch.where(ok, val - lse[rw], torch.zeros_like(val))
        out["extra_logprob"] = (lp, torch.where(ok & torch.isfinite(lp), bnd + b_lse[rw] + U32 * lp.abs(), torch.zeros_like(val)) + 1e-300)
    return out


def stats_ref(x, labels, extra_ptr, extra_labels, T, cap=0.0):
    """The shard statistics, scale-free (see stats_view): {"m", "L2", "E1", "picked", "extra_picked"}: (ref, bound)."""
    R, V = x.shape
    sc = _scaled(x, T, cap)
    st = _row_stats(sc, V)
    out = {"m": (st["M"], st["b_m"]), "L2": (st["L2"], st["b_L2"]), "E1": (st["E1"], st["b_E1"])}
    lab = labels if labels is not None else torch.full((R,), -1, dtype=torch.int64, device=x.device)
    val, bnd, _ = _pick(sc, torch.arange(R, device=x.device), lab, V)
    out["picked"] = (val, bnd + 1e-300)
    if extra_ptr is not None:
        f0, f1, rw = _extra_rows(extra_ptr, R, x.device)
        val, bnd, _ = _pick(sc, rw, extra_labels[f0:f1], V)
        out["extra_picked"] = (val, bnd + 1e-300)
    return out


def stats_view(stats):
    """The kernel's {m, s, t, picked} [R, 4] as the scale-free quantities stats_ref bounds."""
    s64 = _d(stats)
    return {"m": stats[:, 0], "L2": s64[:, 0] + torch.log2(s64[:, 1]), "E1": s64[:, 2] / s64[:, 1], "picked": stats[:, 3]}


def bwd_ref(x, labels, extra_ptr, extra_labels, lse32, ent32, glp, gex, gent, T, cap=0.0):
    """-> {"dlogits": (ref, bound)} [R, V]; lse32 / ent32: the fp32 values the kernel receives; any of labels / glp / gex / gent /
    ent32 may be None as at the raw entry."""
    R, V = x.shape
    dev, dtype = x.device, x.dtype
    sc = _scaled(x, T, cap)
    Tf = sc["T"]
    zero = torch.zeros(R, dtype=torch.float64, device=dev)
    l, en = _d(lse32), (_d(ent32) if ent32 is not None else zero)
    ge, g1 = (_d(gent) if gent is not None else zero), (_d(glp) if glp is not None else zero)
    G, Gabs, ne = g1.clone(), g1.abs().clone(), torch.zeros(R, dtype=torch.float64, device=dev)
    if extra_ptr is not None:
        f0, f1, rw = _extra_rows(extra_ptr, R, dev)
        gx = _d(gex)[f0:f1]
        G.index_add_(0, rw, gx); Gabs.index_add_(0, rw, gx.abs()); ne.index_add_(0, rw, torch.ones_like(gx))
    a = -G + ge * (l - en)
    amag = Gabs + ge.abs() * (l.abs() + en.abs())
    da = U32 * (C32 * torch.sqrt(ne + 1) * Gabs + 2 * ge.abs() * (l.abs() + en.abs()) + amag)
    y, ys, xs = sc["y"], sc["ys"], sc["xs"]
    l2 = (l * LOG2E)[:, None]
    p = torch.where(sc["masked"], torch.zeros_like(y), torch.exp2(y - l2))
    relp = LN2 * (sc["dy"] - U32 * ys.abs() + U32 * (ys - l2).abs() + 1.25 * U32 * l2.abs()) + 2 * U32
    h = a[:, None] - ge[:, None] * xs
    hmag = amag[:, None] + (ge[:, None] * xs).abs()
    dh = da[:, None] + 6 * U32 * hmag
    if sc["c"]:
        dh = dh + ge.abs()[:, None] * (sc["c"] / Tf) * sc["dt"]
    gp = p * h
    one = torch.zeros_like(y)
    if labels is not None:
        ok = (labels >= 0) & (labels < V)
        one[torch.arange(R, device=dev)[ok], labels[ok]] = 1.0
    lab_term = one * g1[:, None]
    g = (gp + lab_term) / Tf
    err = (p * relp * h.abs() + p * dh + 4 * U32 * (gp.abs() + lab_term.abs())) / Tf + FLUSH * (1 + hmag) / Tf
    if sc["c"]:
        err = err * sc["sech2"] + g.abs() * sc["dsech2"]
        g = g * sc["sech2"]
        err = err + U32 * g.abs()
    bound = U[dtype] * g.abs() + err + TINY[dtype]
    if extra_ptr is not None and f1 > f0:
        le = extra_labels[f0:f1]
        ok = (le >= 0) & (le < V)
        rr, cc, gg = rw[ok], le[ok], gx[ok] / Tf
        term, dterm = gg, torch.zeros_like(gg)
        if sc["c"]:
            term, dterm = gg * sc["sech2"][rr, cc], gg.abs() * sc["dsech2"][rr, cc]
        g.index_put_((rr, cc), term, accumulate=True)               # the picks of a row are distinct tokens
        bound.index_put_((rr, cc), U[dtype] * g[rr, cc].abs() + 3 * U32 * term.abs() + dterm + TINY[dtype], accumulate=True)
    return {"dlogits": (g, bound)}


# ------------------------------------------------------------------------------------------------ the check
def check(name, got, ref, bound, label=""):
    """|got - ref| <= bound for EVERY element; where the reference is +-inf `got` must equal it; any other non-finite `got` violates.
    Returns the worst err / bound, also kept in WORST[(name, dtype)]."""
    g = _d(got)
    assert g.shape == ref.shape, f"{label} {name}: shape {tuple(g.shape)}, reference {tuple(ref.shape)}"
    inf = torch.isinf(ref)
    bad_inf = inf & (g != ref)
    assert not bool(bad_inf.any()), f"{label} {name}: {int(bad_inf.sum())} elements differ from an infinite reference"
    err = torch.where(inf, torch.zeros_like(g), (g - torch.where(inf, torch.zeros_like(ref), ref)).abs())
    ratio = err / (bound + 1e-300)
    ratio = torch.where(torch.isfinite(g) | inf, ratio, torch.full_like(ratio, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = (name, str(got.dtype).split(".")[-1])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        cols = g.shape[-1] if g.dim() > 1 else g.numel()
        i = int(ratio.reshape(-1).argmax())
        row, col = divmod(i, cols)
        raise AssertionError(f"{label} {name} ({key[1]}): {int((~(ratio <= 1.0)).sum())} of {g.numel()} elements over the bound, worst "
                             f"err/bound {worst:.3g} at (row {row}, column {col}): got {float(g.reshape(-1)[i]):.9g}, reference "
                             f"{float(ref.reshape(-1)[i]):.9g}, bound {float(bound.expand_as(g).reshape(-1)[i]):.3e}")
    return worst


def check_all(prefix, got: dict, ref: dict, label=""):
    """check() of every tensor in `got` (None entries skipped) against ref[name] = (ref, bound) -> {name: worst err / bound}."""
    return {n: check(f"{prefix}.{n}", t, *ref[n], label=label) for n, t in got.items() if t is not None}
