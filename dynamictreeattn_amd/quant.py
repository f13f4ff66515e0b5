"""Quantised frozen base for LoRA: the frozen projection weights stored in a 4- or 8-bit block format, expanded per use.

Two formats, both cutting a weight [out, in] into blocks along ``in`` with one fp32 scale per block (include/dta.h states them bit by
bit): ``"nf4"`` - blocks of 64, scale = absmax, the 16 NormalFloat-4 levels, two codes per byte - and ``"fp8"`` - blocks of 128, scale =
absmax / 448, OCP e4m3.  `quantize_base` replaces the frozen projections of every decoder layer by `QuantLinear`; the engine
(model._project -> ops.quant_linear) expands a fused group into one transient 16-bit operand where a GEMM needs it and keeps nothing of
it for the backward.  On the device the codes are written and read by the HIP kernels of csrc/quant_kernels.hip; `quantize_host` /
`dequantize_host` are their host mirror in torch expressions, bit for bit, and serve host tensors (the CPU stand-ins)."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lora

# The one Python copy of the NormalFloat-4 table of csrc/dta_quant_tables.h (fp32 literals; tests/test_quant_host.py compares the bits).
NF4_CODEBOOK = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
                -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
BLOCK = {"nf4": 64, "fp8": 128}
FMT_ID = {"nf4": 0, "fp8": 1}                     # DTA_QUANT_NF4 / DTA_QUANT_FP8
BITS_PER_ELEMENT = {"nf4": 4.5, "fp8": 8.25}      # codes + one fp32 scale per block
FP8_MAX = 448.0
# the projections model._project serves: the seven adapter targets and Phi-3's fused ones
PROJECTIONS = (("self_attn", ("q_proj", "k_proj", "v_proj", "qkv_proj", "o_proj")), ("mlp", ("gate_proj", "up_proj", "gate_up_proj", "down_proj")))


def codebook(device=None) -> torch.Tensor:
    return torch.tensor(NF4_CODEBOOK, dtype=torch.float32, device=device)


def midpoints(device=None) -> torch.Tensor:
    """mid_i = (c_i + c_{i+1}) / 2, formed in float64 and rounded to fp32: the 15 decision thresholds of the nf4 encoder."""
    c = torch.tensor(NF4_CODEBOOK, dtype=torch.float32).double()
    return ((c[:-1] + c[1:]) / 2).float().to(device)


def _check_fmt(fmt):
    if fmt not in BLOCK:
        raise ValueError(f"fmt = {fmt!r} is not supported ({' / '.join(BLOCK)})")


def quantize_host(w: torch.Tensor, fmt: str):
    """(codes uint8, scales fp32 [out, in / block]) of a 2-D weight in torch expressions: what dta_quant_blockwise writes, bit for bit."""
    _check_fmt(fmt)
    R, C = w.shape
    B = BLOCK[fmt]
    assert C % B == 0, (C, B)
    x = w.detach().float().reshape(R, C // B, B)
    absmax = x.abs().amax(-1)
    if fmt == "nf4":
        scale = absmax
        v = x / scale[..., None]                                           # 0 / 0 = NaN in an all-zero block: its code is set below
        code = torch.bucketize(v, midpoints(w.device), right=False)        # the number of midpoints strictly below v: a tie takes the lower code
        code = torch.where(scale[..., None] == 0, torch.full_like(code, 7), code).reshape(R, C)
        q = ((code[:, 0::2] << 4) | code[:, 1::2]).to(torch.uint8)
    else:
        scale = absmax / torch.full_like(absmax, FP8_MAX)                  # a tensor divisor: a true fp32 division wherever this runs
        y = (x / scale[..., None]).clamp(-FP8_MAX, FP8_MAX)
        y = torch.where(scale[..., None] == 0, torch.zeros_like(y), y)
        q = y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(R, C)
    return q.contiguous(), scale.contiguous()


def code_values(q: torch.Tensor, fmt: str) -> torch.Tensor:
    """value(code) of every element, fp32 [out, in]."""
    if fmt == "nf4":
        codes = torch.stack(((q >> 4) & 15, q & 15), dim=-1).reshape(q.shape[0], -1).long()
        return codebook(q.device)[codes]
    return q.view(torch.float8_e4m3fn).float()


def dequantize_host(q: torch.Tensor, scales: torch.Tensor, fmt: str, dtype: torch.dtype) -> torch.Tensor:
    """round_to(dtype, value(code) * scale) - one fp32 product, one rounding: what dta_dequant_blockwise writes, bit for bit."""
    _check_fmt(fmt)
    R, nb = scales.shape
    v = code_values(q, fmt).reshape(R, nb, BLOCK[fmt])
    return (v * scales[..., None]).reshape(R, nb * BLOCK[fmt]).to(dtype)


def quantize(w: torch.Tensor, fmt: str):
    """Codes and scales of a weight where it lives: the HIP kernel on the device, the host mirror otherwise."""
    if w.is_cuda:
        from . import ops
        return ops.quant_blockwise(w, fmt)
    return quantize_host(w, fmt)


class QuantLinear(nn.Module):
    """A frozen linear module whose weight is held as block codes: buffers ``qweight`` (uint8) and ``scales`` (fp32), both persistent, an
    optional frozen ``bias``; ``in_features``, ``out_features``, ``fmt``, ``block``, ``dtype`` (the model dtype the weight expands to).
    There is no ``weight`` parameter.  The ``weight`` *property* dequantises the whole matrix on every read: it is what HF's own forward /
    generate, `LoraLinear.forward` and the state-dict exports use, and what the engine never touches."""

    def __init__(self, qweight, scales, bias, in_features: int, out_features: int, fmt: str, dtype: torch.dtype):
        super().__init__()
        _check_fmt(fmt)
        self.in_features, self.out_features, self.fmt, self.block, self.dtype = int(in_features), int(out_features), fmt, BLOCK[fmt], dtype
        self.register_buffer("qweight", qweight)
        self.register_buffer("scales", scales)
        self.bias = bias

    @classmethod
    def from_weight(cls, w: torch.Tensor, bias, fmt: str) -> "QuantLinear":
        q, s = quantize(w.detach(), fmt)
        return cls(q, s, bias, w.shape[1], w.shape[0], fmt, w.dtype)

    def _apply(self, fn, recurse=True):
        """Moves follow the module.  A floating cast (model.half()) changes the dtype the weight expands to and must not round the fp32
        scales."""
        s = self.scales
        super()._apply(fn, recurse)
        if self.scales.dtype != torch.float32:
            self.scales = s.to(self.scales.device)
        probe = fn(torch.empty(0, dtype=self.dtype))
        if probe.is_floating_point():
            self.dtype = probe.dtype
        return self

    @property
    def weight(self) -> torch.Tensor:
        if self.qweight.is_cuda:
            from . import ops
            out = torch.empty((self.out_features, self.in_features), dtype=self.dtype, device=self.qweight.device)
            ops.dequant_blockwise(self.qweight, self.scales, self.fmt, out)
            return out
        return dequantize_host(self.qweight, self.scales, self.fmt, self.dtype)

    def forward(self, x):
        return F.linear(x, self.weight, self.bias)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, fmt={self.fmt}, bias={self.bias is not None}"


def _projections(model):
    """(name, holder, attribute, base module) of every projection module of the decoder layers that model._project serves."""
    for li, layer in enumerate(model.model.layers):
        for parent, names in PROJECTIONS:
            p = getattr(layer, parent, None)
            for t in names:
                m = getattr(p, t, None) if p is not None else None
                if m is None or not isinstance(m, nn.Module):
                    continue
                name = f"model.layers.{li}.{parent}.{t}"
                if lora.carries_adapter(m):
                    yield name + ".base_layer", m, "base_layer", m.base_layer
                else:
                    yield name, p, t, m


@torch.no_grad()
def quantize_base(model, fmt: str = "nf4") -> List[str]:
    """Replaces, in every decoder layer, each frozen 2-D projection module that model._project serves - q/k/v/o/gate/up/down_proj and
    Phi-3's fused qkv_proj / gate_up_proj - by a `QuantLinear` in `fmt` ("nf4" or "fp8"); a module wrapped in a LoRA adapter gets its
    ``base_layer`` replaced, so this works before and after `lora.attach`.  Returns the names of the replaced modules.

    Left alone, at 16 bits: the embeddings, ``lm_head``, every norm, the router gate and the 3-D expert tensors - a mixture-of-experts
    model gets its attention projections quantised and nothing else.

    Refused with a ValueError that names the module and the field, before anything is replaced: a projection whose weight has
    requires_grad = True, in_features not a multiple of the block (64 / 128), an fp32 model, an unknown fmt, a model that is already
    quantised, non-finite weights."""
    _check_fmt(fmt)
    B = BLOCK[fmt]
    todo = []
    for name, holder, attr, base in _projections(model):
        if lora.is_quantized(base):
            raise ValueError(f"{name}.qweight: the model is already quantised ({getattr(base, 'fmt', '?')})")
        w = getattr(base, "weight", None)
        if not isinstance(w, torch.Tensor) or w.dim() != 2:
            continue
        if w.requires_grad:
            raise ValueError(f"{name}.weight.requires_grad = True: a trainable weight is not quantised - freeze it or attach adapters first")
        if w.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"{name}.weight.dtype = {w.dtype}: an fp32 model is not quantised (bf16 / f16 models only)")
        if w.shape[1] % B:
            raise ValueError(f"{name}.in_features = {w.shape[1]} is not a multiple of the {fmt} block of {B}")
        if not bool(torch.isfinite(w).all()):
            raise ValueError(f"{name}.weight holds non-finite values")
        todo.append((name, holder, attr, base, w))
    names = []
    for name, holder, attr, base, w in todo:
        setattr(holder, attr, QuantLinear.from_weight(w, getattr(base, "bias", None), fmt))
        names.append(name)
    return names


@torch.no_grad()
def dequantized_state_dict(model) -> Dict[str, torch.Tensor]:
    """The model's weights under their plain HF names (no ``base_layer``, no adapter keys), every quantised projection as its dequantised
    ``weight`` in the model dtype.  `lora.merged_state_dict` is this plus scaling * B A."""
    return lora._plain_state_dict(model, False)
