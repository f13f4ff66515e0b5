"""Shapes and contents shared by the GPU tests of the quantisation kernels (test_gpu_quant_kernels.py, test_gpu_containment_quant.py).
Everything here is built on the host and is deterministic; importing it needs no GPU."""
import torch

from dynamictreeattn_amd import quant

# (fmt, R, C): one block; a few rows; three nf4 blocks (one and a half fp8 blocks: nf4 only); more than one workgroup of rows with a
# ragged row count; a long row; the transposed tile's edge in both directions (nf4 only: 320 = 5 x 64); 129 rows x three fp8 blocks
_RC = [(1, 64, "nf4"), (3, 128, None), (5, 192, "nf4"), (257, 1024, None), (64, 8192, None), (130, 320, "nf4"), (129, 384, None)]
SHAPES = [(fmt, R, C) for R, C, only in _RC for fmt in ("nf4", "fp8") if only in (None, fmt)]


def shape_id(v):
    return str(v)


def _specials(fmt, B, in_dtype, g):
    """The special blocks, each a vector of B fp32 values representable in `in_dtype`."""
    out = [torch.zeros(B)]                                                         # an all-zero block
    tiny = 1e-30 if in_dtype != torch.float16 else 1e-7
    big_of = torch.bfloat16 if in_dtype == torch.float32 else in_dtype
    one_big = torch.full((B,), tiny); one_big[1::2] = -tiny; one_big[5] = torch.finfo(big_of).max
    out.append(one_big)                                                            # the largest finite value among tiny ones
    neg = 0.3 * torch.randn(B, generator=g).clamp(-3, 3); neg[3] = -2.5
    out.append(neg)                                                                # the absmax element is negative
    if fmt == "nf4" and in_dtype == torch.float32:
        mid = quant.midpoints()
        v = torch.zeros(B)
        v[:15], v[15], v[16], v[17:32] = mid, 1.0, -1.0, torch.nextafter(mid, torch.full_like(mid, 2.0))
        v[32:47] = -mid
        out.append(v)                                                              # on the 15 midpoints, just above them, mirrored; absmax 1
    if fmt == "fp8":
        e = torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).float()      # 0, the subnormals, ... 448
        ties = (e[:-1] + e[1:]) / 2                                                # 126 ties; four mantissa bits: bf16 / f16 values
        v = torch.cat([ties, torch.tensor([448.0, -ties[5]])])
        v[1:126:2] = -v[1:126:2]
        out.append(v)                                                              # scale = 448 / 448 = 1: every element on a rounding tie
    for k in ((10, 14) if in_dtype == torch.float16 else (10, 40, 70, 100)):
        v = torch.randn(B, generator=g).clamp(-3, 3) / 4 * 2.0 ** -k
        v[7] = -(2.0 ** -k)
        out.append(v)                                                              # block absmax 2^-k
    return out


def content(R, C, fmt, in_dtype, seed):
    """A weight [R, C] in `in_dtype` (on the host): random, with the special blocks from the first block of the first row on."""
    B = quant.BLOCK[fmt]
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(R, C, generator=g) * torch.exp(2 * torch.randn(R, 1, generator=g).clamp(-3, 3))
    blocks = w.view(R * (C // B), B)
    specials = _specials(fmt, B, in_dtype, g)
    if blocks.shape[0] < len(specials):                                            # a shape of a few blocks: the zero block must not be all of it
        specials = specials[2:] + specials[:2]
    for i, v in enumerate(specials[:blocks.shape[0]]):
        blocks[i] = v
    return w.to(in_dtype)


def codes(R, C, fmt, seed):
    """(codes, scales) on the host for the expansion tests: the mirror's quantisation of `content` (fp32 input: with the midpoint
    block) and, from the fourth row on where there is one, every byte value as a code (fp8: but the two NaN encodings)."""
    q, s = quant.quantize_host(content(R, C, fmt, torch.float32, seed), fmt)
    if R > 3:
        every = torch.arange(q.shape[1], dtype=torch.int64) % 256
        if fmt == "fp8":
            every[(every & 0x7F) == 0x7F] = 0x3C
        q[3] = every.to(torch.uint8)
    return q, s
