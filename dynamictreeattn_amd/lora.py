"""LoRA adapters: frozen base weights, a pair of low-rank matrices per projection trained.

A projection module *carries an adapter* iff it has ``base_layer``, ``lora_A``, ``lora_B`` and ``scaling`` - the layout of PEFT's
``lora.Linear``, duck-typed (PEFT is not imported): ``base_layer`` the original linear; ``lora_A[name]`` / ``lora_B[name]`` bias-free
linears of shape [r, in] / [out, r] in ``ModuleDict``s; ``scaling[name]`` a float; optional ``active_adapters``, ``disable_adapters``,
``merged``, ``use_dora``, ``lora_dropout``.  The arithmetic is ``y = base(x) + scaling * (x Aᵀ) Bᵀ``.

The model layer (model._layer_forward) resolves every projection through `resolve`; the engine runs the base GEMM of a fused group
(q|k|v, gate|up) once and the adapters of its members through ops.lora_linear (each low-rank product as the HIP kernel of csrc/lora_kernels.hip or the GEMM expression, whichever was
measured faster at its shape).  `attach`
builds the layout on a model in plain torch; a module tree from elsewhere with the same attributes is served the same way."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
MAX_RANK = 256
_GROUPS = (("self_attn", ("q_proj", "k_proj", "v_proj", "o_proj")), ("mlp", ("gate_proj", "up_proj", "down_proj")))


class LoraLinear(nn.Module):
    """A linear module with one low-rank adapter, attribute for attribute PEFT's ``lora.Linear``.  Its own forward is the formula, so
    the model's own forward / generate keep working; the engine does not call it."""

    def __init__(self, base: nn.Module, r: int, alpha: float, adapter_name: str = "default", dtype: torch.dtype = torch.float32):
        super().__init__()
        out_f, in_f, _, dev = base_geometry(base)
        self.base_layer = base
        self.in_features, self.out_features = in_f, out_f
        self.lora_A = nn.ModuleDict({adapter_name: nn.Linear(in_f, r, bias=False, device=dev, dtype=dtype)})
        self.lora_B = nn.ModuleDict({adapter_name: nn.Linear(r, out_f, bias=False, device=dev, dtype=dtype)})
        self.lora_dropout = nn.ModuleDict({adapter_name: nn.Identity()})
        self.r, self.lora_alpha, self.scaling = {adapter_name: r}, {adapter_name: alpha}, {adapter_name: alpha / r}
        self.use_dora, self.lora_bias = {adapter_name: False}, {adapter_name: False}
        self.active_adapters = [adapter_name]
        self.disable_adapters = self.merged = self.fan_in_fan_out = False

    @property
    def weight(self):
        return self.base_layer.weight

    @property
    def bias(self):
        return getattr(self.base_layer, "bias", None)

    def forward(self, x):
        y = F.linear(x, self.base_layer.weight, getattr(self.base_layer, "bias", None))
        if self.disable_adapters or self.merged:
            return y
        for n in self.active_adapters:
            if n in self.lora_A:
                A = self.lora_A[n]
                y = (y + self.lora_B[n](A(x.to(A.weight.dtype))) * self.scaling[n]).to(y.dtype)
        return y


QUANT_FORMATS = ("nf4", "fp8")      # quant.BLOCK's keys (quant.py imports this module, not the reverse)


def is_quantized(m) -> bool:
    """A base module that holds block codes of THIS project's formats instead of a weight (quant.QuantLinear, duck-typed: ``qweight``,
    ``scales`` and ``fmt`` one of quant.BLOCK).  A GPTQ / AWQ module has the first two and another layout: it is not taken for one."""
    return hasattr(m, "qweight") and hasattr(m, "scales") and getattr(m, "fmt", None) in QUANT_FORMATS


def base_geometry(base):
    """(out_features, in_features, dtype, device) of a 2-D base projection, None for anything else.  A quantised base answers from its
    attributes: its ``weight`` is a property that dequantises the whole matrix, and nothing on the per-call path may touch it."""
    if is_quantized(base):
        return int(base.out_features), int(base.in_features), base.dtype, base.qweight.device
    w = getattr(base, "weight", None)
    if not isinstance(w, torch.Tensor) or w.dim() != 2:
        return None
    return int(w.shape[0]), int(w.shape[1]), w.dtype, w.device


def carries_adapter(m) -> bool:
    return all(hasattr(m, f) for f in ("base_layer", "lora_A", "lora_B", "scaling"))


def _active_names(m) -> List[str]:
    names = getattr(m, "active_adapters", None)
    if names is None:
        names = getattr(m, "active_adapter", None)
    if names is None:
        names = list(m.lora_A.keys())
    if isinstance(names, str):
        names = [names]
    return [n for n in names if n in m.lora_A]


def resolve(m):
    """(module that holds the base weight and bias, adapter) of a projection module: adapter = (A [r, in], B [out, r], scaling) of its
    one active adapter, or None - a plain module, or ``merged`` / ``disable_adapters`` set (the base path alone, as PEFT computes it)."""
    if not carries_adapter(m):
        return m, None
    base = m.base_layer
    if getattr(m, "disable_adapters", False) or getattr(m, "merged", False):
        return base, None
    names = _active_names(m)
    if not names:
        return base, None
    if len(names) > 1:
        raise ValueError(f"{type(m).__name__}.active_adapters = {names}: one active adapter per module is supported")
    n = names[0]
    return base, (m.lora_A[n].weight, m.lora_B[n].weight, float(m.scaling[n]))


def _wrapped(model):
    return [(name, m) for name, m in model.named_modules() if carries_adapter(m) or len(getattr(m, "lora_embedding_A", ())) > 0]


def rank_elems_per_token(model) -> float:
    """Elements per token and layer (the mean over the layers) the adapters keep for the backward: x·Aᵀ, Σr over the adapted projections."""
    layers = getattr(getattr(model, "model", None), "layers", None)
    if not layers:
        return 0.0
    total = 0
    for layer in layers:
        for parent, names in _GROUPS:
            p = getattr(layer, parent, None)
            for t in names:
                m = getattr(p, t, None)
                if m is not None and carries_adapter(m):
                    total += sum(int(m.lora_A[n].weight.shape[0]) for n in _active_names(m))
    return total / len(layers)


def check_supported(model) -> None:
    """Refuses, with a ValueError that names the module and the field, an adapter configuration the engine cannot honour (it would run,
    and compute something else): DoRA, lora_dropout p > 0 on a model in training mode, more than one active adapter on a module,
    fan_in_fan_out, lora_bias, an adapter on anything that is not one of the seven projections of a decoder layer (embedding, lm_head,
    router gate, the 3-D expert tensors), an adapter dtype that is neither fp32 nor the model dtype, r > 256.  ``merged`` or
    ``disable_adapters`` set: the base path alone - nothing to check."""
    training = bool(getattr(model, "training", True))
    for name, m in _wrapped(model):
        leaf = name.rsplit(".", 1)[-1]
        base = getattr(m, "base_layer", None)
        geo = base_geometry(base) if base is not None else None
        if not carries_adapter(m) or leaf not in TARGETS or ".layers." not in "." + name or geo is None or ".experts" in name:
            raise ValueError(f"{name}: an adapter on this module is not supported (adapters go on {' / '.join(TARGETS)} of the decoder "
                             f"layers; not on embeddings, lm_head, the router gate or the expert tensors)")
        if getattr(m, "disable_adapters", False) or getattr(m, "merged", False):
            continue
        names = _active_names(m)
        if len(names) > 1:
            raise ValueError(f"{name}.active_adapters = {names}: one active adapter per module is supported")
        if getattr(m, "fan_in_fan_out", False):
            raise ValueError(f"{name}.fan_in_fan_out is not supported")
        for n in names:
            if _flag(getattr(m, "use_dora", None), n):
                raise ValueError(f"{name}.use_dora[{n!r}]: DoRA is not supported")
            if _flag(getattr(m, "lora_bias", None), n) or getattr(m.lora_B[n], "bias", None) is not None or getattr(m.lora_A[n], "bias", None) is not None:
                raise ValueError(f"{name}.lora_bias[{n!r}]: adapter biases are not supported")
            drop = getattr(m, "lora_dropout", None)
            d = drop[n] if drop is not None and n in drop else None
            if training and float(getattr(d, "p", 0.0) or 0.0) > 0:
                raise ValueError(f"{name}.lora_dropout[{n!r}] p = {d.p} on a model in training mode is not supported (model.eval(), or p = 0)")
            A, B = m.lora_A[n].weight, m.lora_B[n].weight
            if A.shape[0] > MAX_RANK or A.shape[0] != B.shape[1]:
                raise ValueError(f"{name}.lora_A[{n!r}]: r = {A.shape[0]} is not supported (1..{MAX_RANK}, lora_B [out, r])")
            if A.shape[1] != geo[1] or B.shape[0] != geo[0]:
                raise ValueError(f"{name}.lora_A / lora_B[{n!r}]: shapes {tuple(A.shape)} / {tuple(B.shape)} do not fit the base weight {geo[:2]}")
            for t, f in ((A, "lora_A"), (B, "lora_B")):
                if t.dtype not in (torch.float32, geo[2]):
                    raise ValueError(f"{name}.{f}[{n!r}] dtype {t.dtype} is not supported: fp32 or the model dtype ({geo[2]})")


def _flag(d, n) -> bool:
    if isinstance(d, dict):
        return bool(d.get(n, False))
    return bool(d)


def _rank_of(full_name: str, r: int, rank_pattern: Optional[Dict[str, int]]) -> int:
    for key, val in (rank_pattern or {}).items():
        if full_name == key or full_name.endswith("." + key):
            return int(val)
    return int(r)


def attach(model, r: int, alpha: float, target_modules: Iterable[str] = TARGETS, adapter_name: str = "default",
           dtype: torch.dtype = torch.float32, rank_pattern: Optional[Dict[str, int]] = None, seed: Optional[int] = None) -> List[nn.Parameter]:
    """Wraps the named projections of every decoder layer in `LoraLinear` (rank r, or rank_pattern[name suffix]; scaling = alpha / rank),
    initialises as PEFT does (A Kaiming-uniform with a = sqrt(5), B zero), freezes every other parameter and returns the adapter
    parameters.  Parameter names follow PEFT: ``…q_proj.base_layer.weight``, ``…q_proj.lora_A.default.weight``,
    ``…q_proj.lora_B.default.weight``.  The MLP of a mixture-of-experts layer has no such projections: its experts stay frozen."""
    targets = tuple(target_modules)
    bad = [t for t in targets if t not in TARGETS]
    if bad:
        raise ValueError(f"target_modules {bad} are not supported ({' / '.join(TARGETS)})")
    have = [name for name, m in model.named_modules() if carries_adapter(m)]
    if have:           # freezing "every other parameter" would silently freeze the adapters already there
        raise ValueError(f"the model already carries adapters ({have[0]} and {len(have) - 1} more): lora.detach(model) first")
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    made = []
    for li, layer in enumerate(model.model.layers):
        for parent, names in _GROUPS:
            p = getattr(layer, parent, None)
            for t in names:
                m = getattr(p, t, None)
                if t not in targets or m is None or carries_adapter(m) or base_geometry(m) is None:
                    continue
                rank = _rank_of(f"model.layers.{li}.{parent}.{t}", r, rank_pattern)
                if not 1 <= rank <= MAX_RANK:
                    raise ValueError(f"r = {rank} is not supported (1..{MAX_RANK})")
                wrapped = LoraLinear(m, rank, float(alpha), adapter_name, dtype)
                A = wrapped.lora_A[adapter_name].weight
                with torch.no_grad():
                    init = torch.empty(A.shape, dtype=torch.float32)
                    nn.init.kaiming_uniform_(init, a=math.sqrt(5), generator=gen)
                    A.copy_(init)
                    wrapped.lora_B[adapter_name].weight.zero_()
                setattr(p, t, wrapped)
                made.append(wrapped)
    for prm in model.parameters():
        prm.requires_grad_(False)
    out = []
    for w in made:
        for prm in (w.lora_A[adapter_name].weight, w.lora_B[adapter_name].weight):
            prm.requires_grad_(True)
            out.append(prm)
    return out


def detach(model) -> None:
    """Puts the plain base modules back in place of every wrapped projection (requires_grad flags are left as they are)."""
    for layer in model.model.layers:
        for parent, names in _GROUPS:
            p = getattr(layer, parent, None)
            for t in names:
                m = getattr(p, t, None)
                if m is not None and carries_adapter(m):
                    setattr(p, t, m.base_layer)


def _is_adapter_key(k: str) -> bool:
    return ".lora_A." in k or ".lora_B." in k


def adapter_state_dict(model) -> Dict[str, torch.Tensor]:
    return {k: v.detach().clone() for k, v in model.state_dict().items() if _is_adapter_key(k)}


@torch.no_grad()
def load_adapter_state_dict(model, sd: Dict[str, torch.Tensor]) -> None:
    own = {k: v for k, v in model.state_dict().items() if _is_adapter_key(k)}
    if set(own) != set(sd):
        raise KeyError(f"adapter keys differ: missing {sorted(set(own) - set(sd))[:3]}, unexpected {sorted(set(sd) - set(own))[:3]}")
    for k, v in own.items():
        v.copy_(sd[k])


def _plain_state_dict(model, fold: bool) -> Dict[str, torch.Tensor]:
    """The model's weights under their plain names: adapter keys dropped, ``.base_layer.`` removed, a quantised base (its ``qweight`` /
    ``scales`` buffers) as its dequantised ``weight`` and, with `fold`, every active adapter added in fp32 and rounded once."""
    delta = {}
    if fold:
        for name, m in model.named_modules():
            if carries_adapter(m):
                _, ad = resolve(m)
                if ad is not None:
                    A, B, s = ad
                    delta[name + ".base_layer.weight"] = s * (B.float() @ A.float())
    quantized = {name: m for name, m in model.named_modules() if is_quantized(m)}
    out = {}
    for k, v in model.state_dict().items():
        if _is_adapter_key(k):
            continue
        t = v.detach()
        mod, _, leaf = k.rpartition(".")
        if mod in quantized and leaf in ("qweight", "scales"):
            if leaf == "scales":
                continue
            k, t = mod + ".weight", quantized[mod].weight
        if k in delta:
            t = (t.float() + delta[k].to(t.device)).to(t.dtype)
        out[k.replace(".base_layer.", ".")] = t.clone()
    return out


@torch.no_grad()
def merged_state_dict(model) -> Dict[str, torch.Tensor]:
    """The model's weights under their plain names with every active adapter folded in: W + scaling * B A, formed in fp32 and rounded
    once to the weight's dtype - what a rollout engine is handed after a step.  On a quantised base (quant.quantize_base) W is the
    dequantised matrix."""
    return _plain_state_dict(model, True)
