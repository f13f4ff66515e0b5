"""Float64 restatement of the GEMM layer of ops.py (`_Linear`, `_dgrad`, `_wgrad`, `stack_rows`, the weight gradient of `_HeadRows`) for
the ROUNDED operands the product sees, with the operand magnitudes of the project's per-element bound ref64_common.bound(ref, mag, n, dtype):

    |out - ref| <= u |ref| + C32 sqrt(n) u32 mag (+ tiny)        u: ONE rounding to the output type, n: the contraction length, mag = |A| |B|

* forward  y = x Wᵀ + b:   ref as written, mag = |x| |W|ᵀ + |b|, n = in.  The library may round the product to the output type before its
                           epilogue adds the bias: with a bias the bound carries one more rounding of the product, u |x Wᵀ|.
* dgrad    dx = dy W:      mag = |dy| |W|, n = out.  The cached transposed copy is the same product: no term of its own.
* wgrad    dW = dyᵀ x:     mag = |dy|ᵀ |x|, n = T.  The split form (ops._wgrad: WGRAD_SPLIT_K slices of `per` = (T // S) // 64 * 64 rows into fp32
                           slabs, the T - S per left-over rows as one more fp32 product, summed in fp32 and rounded ONCE by sum_slabs) is
                           the same single rounding over a longer fp32 chain, which sqrt(T) already counts: no term of its own either.
* db = Σ_t dy:             mag = Σ |dy|, n = T.
* head     dW = gᵀ h with g the log-prob kernel's ROUNDED dlogits, known only within logprob_ref64.bwd_ref's (gref, gbound):
                           ref = grefᵀ h,  bound = gboundᵀ |h| + bound(ref, |gref|ᵀ |h|, T, dtype)
                           (every element's dlogits bound carried through |h|, then the GEMM over the T rows and the one rounding to the
                           model dtype).  The chunked non-fused form (`dW += mm(g_cᵀ, h_c)` in fp32) rounds EACH chunk's product to the model
                           dtype before the fp32 sum - _HeadRows's documented arithmetic: + Σ_c u |gref_cᵀ h_c|.
No constant is fitted.  A form that is nothing but one library GEMM (`a.t() @ b`, `dy @ w`, F.linear) is also evaluated as that library
call at the same shape: were the library alone over the bound, the form is held to 1.25 x the library's own worst ratio (the margin: another
tile order) and the figure is listed below as a statement about the library.  Forms with the project's arithmetic in them (the split, sum_slabs,
cached transposes, stacked rows, the head's chunk sum) get no allowance.

`emulate_wgrad` restates the split on the CPU (fp32 slabs, one rounding) and offers the corruptions a whole-tensor norm of 3e-3
(tests/test_gpu_properties.py) lets through; tests/test_linear_ref64.py holds the honest form inside the bound and every corruption outside.

OBSERVED worst err / bound (bf16 / f16 / fp32; "-": not a case of that type).
CPU emulation of tests/test_linear_ref64.py (T = 8192, 8193, 8447; out x in = 256 x 512 and 72 x 200; Gaussian operands unless said):
    wgrad honest .89/.52/-  (f16, one-signed operands: .78)
    corrupted (lowest over the cases)  slabs rounded 4.1 / 1.25 (f16: one-signed; Gaussian f16 only .68 - 1.04)   slab twice 1700/1800
                 left-over dropped or doubled 45/53   rounded, left-over added, rounded again 1.43 / 1.46 (f16: one-signed)
                 not transposed back 2200/2600
    head dW, aligned rows (T = 2 x 4096, V = H = 64): a rounding per chunk WITH the chunk term .73/.69, without it 1.17/1.08; one rounding
                 without it .81/.81.  Gaussian rows: .21/.18, .24/.21, .15/.17 - the dlogits term hides the chunk roundings there
MI355X, over tests/test_gpu_linear_bounds.py (the WORST lines it prints):
    _wgrad       plain (8191 rows; fp32; 72 tiles) .897/.527/.017   split, no left-over .882/.522/-   1 left-over row .897/.530/-
                 255 left-over rows .884/.516/-   strided operands .892/.522/-
    _dgrad       plain .992/.971/.103   transposed copy .991/.967/-   two views of one storage .992/.968/-
    ops.linear   y .991/.967/-   dx .992/.969/-   dw .915/.714/-   db .797/.513/-   stacked rows: y .987/.959/-, members' dw .894/.526/-
    _HeadRows    dh .798/.796/-   dW kept .471/.524/-   fused accumulation .471/.524/-   chunk sum (with the chunk term) .540/.492/-
                 forward: logprob .24/.23   fork logprob .08/.07   entropy .11/.11
                 aligned rows (bf16): chunk sum with the term .79, without it 1.48; fused accumulation without it .87; dh .45
No library-only form (a.t() @ b, dy @ w, F.linear, dy.sum(0)) exceeded the bound at any shape of the tests, so none carries the 1.25 x allowance.
The 16-bit GEMM outputs sit at .88 - .99 because u is the exact worst case of ONE rounding; f16 sits lower wherever the product cancels
(weight gradients over 8 k rows), where the fp32 term is the larger part of its bound.
"""
import torch

import logprob_ref64
from ref64_common import C32, TINY, U, U32, bound      # noqa: F401  (C32, U32, TINY: the constants the docstring's bound names)

SPLIT_K = 4                        # ops.WGRAD_SPLIT_K
WORST: dict = {}
CORRUPTIONS = ("round_slabs", "slab_twice", "drop_rest", "rest_twice", "round_then_rest", "not_transposed_back")
LEFT_OVER_ONLY = ("drop_rest", "rest_twice", "round_then_rest")      # change something only when T leaves rows over


def _d(t):
    return t.detach().double()


# ------------------------------------------------------------------------------------------------ references: (ref, mag, n)
def wgrad_ref(x, dy):
    return _d(dy).t() @ _d(x), _d(dy).abs().t() @ _d(x).abs(), x.shape[0]


def dgrad_ref(dy, w):
    return _d(dy) @ _d(w), _d(dy).abs() @ _d(w).abs(), w.shape[0]


def fwd_ref(x, w, b=None):
    """-> (ref, mag, n, extra): `extra` is the epilogue's rounding of the product before the bias is added (0 without a bias)."""
    prod, mag = _d(x) @ _d(w).t(), _d(x).abs() @ _d(w).abs().t()
    if b is None:
        return prod, mag, x.shape[1], torch.zeros_like(prod)
    return prod + _d(b), mag + _d(b).abs(), x.shape[1], prod.abs()


def fwd_bound(ref, mag, n, extra, dtype):
    return bound(ref, mag, n, dtype) + U[dtype] * extra


def bias_grad_ref(dy):
    return _d(dy).sum(0), _d(dy).abs().sum(0), dy.shape[0]


def head_dw_ref(h, logits, labels, fork_ptr, fork_tok, lse32, ent32, g_next, g_fork, g_ent, temperature=1.0, cap=0.0, chunk=None):
    """The LM head's weight gradient -> (dW [V, H] float64, bound, gref, gbound).  logits: the model-dtype logits the backward kernel
    received; lse32 / ent32: the forward's fp32 statistics.  chunk: rows per chunk of the NON-FUSED chunked form (each chunk's product
    rounded to the model dtype before the fp32 sum); None for the kept form and the fused accumulation (one rounding)."""
    dtype = logits.dtype
    gref, gbound = logprob_ref64.bwd_ref(logits, labels, fork_ptr, fork_tok, lse32, ent32, g_next, g_fork, g_ent, temperature, cap)["dlogits"]
    h64 = _d(h)
    dw = gref.t() @ h64
    bnd = gbound.t() @ h64.abs() + bound(dw, gref.abs().t() @ h64.abs(), h.shape[0], dtype)
    if chunk is not None:
        for a in range(0, h.shape[0], chunk):
            bnd = bnd + U[dtype] * (gref[a:a + chunk].t() @ h64[a:a + chunk]).abs()
    return dw, bnd, gref, gbound


# ------------------------------------------------------------------------------------------------ the split weight gradient, restated
def split_plan(T, S=SPLIT_K):
    """(per, body) of ops._wgrad: S slices of `per` rows; rows body .. T are left over."""
    per = (T // S) // 64 * 64
    return per, per * S


def takes_split(T, out_f, in_f, dtype, S=SPLIT_K):
    """Whether ops._wgrad takes the split form for this problem on the device."""
    per, _ = split_plan(T, S)
    return -(-out_f // 256) * -(-in_f // 256) <= 64 and per >= 2048 and dtype != torch.float32


def emulate_wgrad(x, dy, dtype, corrupt=None, transposed=False):
    """ops._wgrad's split form on the host: x [T, in], dy [T, out] already rounded to `dtype` -> dW [out, in] in `dtype`.  fp32 slabs
    (each a float64 product rounded to fp32: an fp32-accumulating GEMM is no closer), the left-over rows as one more fp32 product, ONE
    fp32 sum in slab order and ONE rounding.  corrupt: one of CORRUPTIONS."""
    assert corrupt is None or corrupt in CORRUPTIONS, corrupt
    T = x.shape[0]
    a, b = (x, dy) if transposed else (dy, x)
    S = SPLIT_K
    per, body = split_plan(T)
    part = torch.bmm(_d(a[:body]).reshape(S, per, a.shape[1]).transpose(1, 2), _d(b[:body]).reshape(S, per, b.shape[1])).float()
    rest = (_d(a[body:]).t() @ _d(b[body:])).float() if body < T else None
    if corrupt == "round_slabs":             # a 16-bit output type of the batched GEMM
        part = part.to(dtype).float()
        rest = rest.to(dtype).float() if rest is not None else None
    if corrupt == "slab_twice":              # slice 0 read in the place of slice 1
        part = torch.cat([part[:1], part[:1], part[2:]])
    if corrupt == "drop_rest":
        rest = None
    if corrupt == "rest_twice" and rest is not None:
        rest = rest + rest
    acc = part[0].clone()
    for s in range(1, S):
        acc += part[s]
    if corrupt == "round_then_rest" and rest is not None:
        out = (acc.to(dtype).float() + rest).to(dtype)
    else:
        out = (acc + rest if rest is not None else acc).to(dtype)
    if not transposed:
        return out
    if corrupt == "not_transposed_back":     # the [in, out] memory handed on under the shape [out, in]
        return out.reshape(out.shape[1], out.shape[0])
    return out.t().contiguous()


def emulate_head_dw(g, h, dtype, chunk=None):
    """The head's weight gradient on the host from rounded dlogits g [T, V] and h [T, H]: chunk None - one product, one rounding (kept
    logits, fused accumulation); else every chunk's product rounded to `dtype`, summed in fp32, rounded."""
    if chunk is None:
        return (_d(g).t() @ _d(h)).float().to(dtype)
    acc = torch.zeros(g.shape[1], h.shape[1], dtype=torch.float32)
    for a in range(0, g.shape[0], chunk):
        acc += (_d(g[a:a + chunk]).t() @ _d(h[a:a + chunk])).float().to(dtype).float()
    return acc.to(dtype)


# ------------------------------------------------------------------------------------------------ the check
def ratio(got, ref, bnd):
    """Worst |got - ref| / bound over all elements; inf for a shape mismatch or a non-finite result."""
    if tuple(got.shape) != tuple(ref.shape):
        return float("inf")
    g = _d(got)
    r = (g - ref).abs() / (bnd + 1e-300)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def check(name, got, ref, bnd, label="", limit=1.0):
    """|got - ref| <= limit * bound for EVERY element (limit 1 unless a library-only form carries the library's own ratio).  Returns the
    worst err / bound, also kept in WORST[(name, dtype)]."""
    assert tuple(got.shape) == tuple(ref.shape), f"{label} {name}: shape {tuple(got.shape)}, reference {tuple(ref.shape)}"
    worst = ratio(got, ref, bnd)
    key = (name, str(got.dtype).split(".")[-1])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= limit:
        g = _d(got)
        r = (g - ref).abs() / (bnd + 1e-300)
        i = int(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).reshape(-1).argmax())
        row, col = divmod(i, g.shape[-1]) if g.dim() > 1 else (0, i)
        raise AssertionError(f"{label} {name} ({key[1]}): {int((~(r <= limit)).sum())} of {g.numel()} elements over the bound, worst err/bound "
                             f"{worst:.3g} (limit {limit:.3g}) at (row {row}, column {col}): got {float(g.reshape(-1)[i]):.9g}, reference "
                             f"{float(ref.reshape(-1)[i]):.9g}, bound {float(bnd.reshape(-1)[i]):.3e}")
    return worst


def norm_error(got, ref):
    """The whole-tensor relative error tests/test_gpu_properties.py::test_split_k_weight_gradient_equals_the_single_gemm asserts <= 3e-3."""
    return float((_d(got) - ref).norm() / ref.norm())
