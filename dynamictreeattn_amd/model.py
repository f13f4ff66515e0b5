"""Qwen3-family decoder over a *packed trie* (one pass over all tree tokens).

The reference drives an unmodified HuggingFace causal LM once per trie segment
(tree_training_engine.py:182-186, 248-252, 351-353).  Here the whole trie is one batch of T packed
tokens: position = trie depth, attention = `ops.tree_attention` (HIP), GEMMs = hipBLASLt through
torch.  `Qwen3TreeLM` mirrors the HF module/parameter tree (``model.embed_tokens.weight``,
``model.layers.N.self_attn.q_proj.weight`` …, tied head) so that

* gradients compare name by name with grad/Qwen3-0.6B-TB-vs-DB-bf16.txt (310 tensors), and
* `packed_hidden_states` also accepts a HuggingFace Qwen2/Qwen3/Qwen3-MoE/Llama/Mistral/Mixtral/Gemma-2/OLMo-2/OLMo-3/Phi-3/Phi-4/GLM-4/Cohere/Cohere2 ``*ForCausalLM`` by duck typing —
  its own ``nn.Parameter`` objects are used, so ``param.grad`` lands where the training loop expects.
"""
from __future__ import annotations

import weakref
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lora, ops


class _Norm(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(n))


class _Lin(nn.Module):
    def __init__(self, i, o):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(o, i))


class _Attn(nn.Module):
    def __init__(self, c):
        super().__init__()
        H, Hq, Hkv, D = c.hidden_size, c.num_attention_heads, c.num_key_value_heads, c.head_dim
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = _Lin(H, Hq * D), _Lin(H, Hkv * D), _Lin(H, Hkv * D), _Lin(Hq * D, H)
        if not is_cohere(c):                                  # (the supported Cohere models have no q/k norm)
            self.q_norm, self.k_norm = _Norm(D), _Norm(D)


class _MLP(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _Lin(c.hidden_size, c.intermediate_size), _Lin(c.hidden_size, c.intermediate_size), _Lin(c.intermediate_size, c.hidden_size)


def moe_geometry(c):
    """(experts, expert intermediate size, renormalise the top-k weights) of an MoE configuration: Qwen3-MoE names them num_experts /
    moe_intermediate_size / norm_topk_prob; Mixtral num_local_experts / intermediate_size, and its router always renormalises.
    (0, 0, False) for a dense model."""
    E = getattr(c, "num_experts", 0) or 0
    if E and getattr(c, "moe_intermediate_size", None) is not None:      # (MixtralConfig answers num_experts too, as an alias)
        return E, c.moe_intermediate_size, bool(getattr(c, "norm_topk_prob", False))
    E = getattr(c, "num_local_experts", 0) or 0
    return (E, c.intermediate_size, True) if E else (0, 0, False)


class _Router(nn.Module):
    def __init__(self, c):
        super().__init__()
        E, _, norm = moe_geometry(c)
        self.top_k, self.num_experts, self.norm_topk_prob = c.num_experts_per_tok, E, norm
        self.weight = nn.Parameter(torch.empty(E, c.hidden_size))


class _Experts(nn.Module):
    def __init__(self, c):
        super().__init__()
        (E, I, _), H = moe_geometry(c), c.hidden_size
        self.gate_up_proj = nn.Parameter(torch.empty(E, 2 * I, H))
        self.down_proj = nn.Parameter(torch.empty(E, H, I))


class _MoE(nn.Module):
    """HF Qwen3MoeSparseMoeBlock's parameter tree: mlp.gate.weight [E, H], mlp.experts.gate_up_proj [E, 2I, H], mlp.experts.down_proj [E, H, I]."""

    def __init__(self, c):
        super().__init__()
        self.gate, self.experts = _Router(c), _Experts(c)


def is_moe_layer(c, l: int) -> bool:
    """The rule of HF Qwen3MoeDecoderLayer: experts unless the layer is in mlp_only_layers, when num_experts > 0 and (l + 1) is a
    multiple of decoder_sparse_step.  A Mixtral configuration (num_local_experts, neither of the two lists) has experts in every layer."""
    E = moe_geometry(c)[0]
    return E > 0 and l not in (getattr(c, "mlp_only_layers", None) or []) and (l + 1) % (getattr(c, "decoder_sparse_step", 1) or 1) == 0


class _Layer(nn.Module):
    def __init__(self, c, l=0):
        super().__init__()
        self.self_attn, self.mlp = _Attn(c), (_MoE(c) if is_moe_layer(c, l) else _MLP(c))
        self.input_layernorm = _Norm(c.hidden_size)
        if not is_cohere(c):                                  # Cohere's parallel block has one norm per layer
            self.post_attention_layernorm = _Norm(c.hidden_size)


class _Body(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.embed_tokens = nn.Embedding(c.vocab_size, c.hidden_size)
        self.layers = nn.ModuleList(_Layer(c, l) for l in range(c.num_hidden_layers))
        self.norm = _Norm(c.hidden_size)


def make_config(d: dict) -> SimpleNamespace:
    """Configuration of a Qwen3TreeLM from a dict of HF field names.  `rope_parameters` is the dict HF configurations keep
    (rope_type default / linear / llama3 / yarn with the type's fields; its rope_theta goes before the top-level one).
    model_type "cohere" / "cohere2" builds the Cohere parameter tree: one LayerNorm weight per layer, no q/k norms."""
    c = SimpleNamespace(**d)
    if not hasattr(c, "head_dim"):
        c.head_dim = c.hidden_size // c.num_attention_heads
    c.rms_norm_eps = getattr(c, "rms_norm_eps", 1e-6)
    c.rope_theta = getattr(c, "rope_theta", 1e6)
    return c


class Qwen3TreeLM(nn.Module):
    """Parameter container with the HF names; tied LM head (no lm_head parameter)."""

    def __init__(self, config):
        super().__init__()
        self.config = make_config(config) if isinstance(config, dict) else config
        self.model = _Body(self.config)

    @property
    def device(self):
        return self.model.embed_tokens.weight.device

    @torch.no_grad()
    def load_named(self, weights: dict):
        own = dict(self.named_parameters())
        for k, p in own.items():
            p.copy_(weights[k])
        return self

    @classmethod
    def from_named(cls, config, weights: dict, device, dtype):
        m = cls(config)
        m.load_named(weights)
        return m.to(device=device, dtype=dtype)


def is_olmo(config) -> bool:
    """OLMo-2 / OLMo-3 arithmetic (q/k RMSNorm over the whole projection row before RoPE, and the post-norm layer
    h = x + norm(attn(x)), y = h + norm(mlp(h))) is keyed on config.model_type in ("olmo2", "olmo3") and on nothing else."""
    return getattr(config, "model_type", None) in ("olmo2", "olmo3")


def is_cohere(config) -> bool:
    """Cohere / Cohere2 arithmetic (mean-centred LayerNorm without bias, the parallel block x + attn(h) + mlp(h) behind ONE norm,
    interleaved RoPE pairs over the whole head, a scale on the final logits and, for cohere2, full-attention layers without RoPE) is
    keyed on config.model_type in ("cohere", "cohere2") and on nothing else."""
    return getattr(config, "model_type", None) in ("cohere", "cohere2")


def logit_scale_of(model) -> float:
    """The factor on the final logits the LM-head kernels apply for `model` as their temperature 1 / scale: config.logit_scale of a
    Cohere model, 1.0 for every other (their head runs bit for bit as without it)."""
    return float(model.config.logit_scale) if is_cohere(model.config) else 1.0


def is_phi3(config) -> bool:
    """Phi-3 / Phi-4 arithmetic (fused qkv_proj and gate_up_proj modules, half-split RoPE over the first rotary_dim elements of the
    head, rope_type longrope, a sliding window on every layer) is keyed on config.model_type == "phi3" and on nothing else."""
    return getattr(config, "model_type", None) == "phi3"


def is_glm4(config) -> bool:
    """GLM-4 arithmetic (interleaved RoPE pairs (2i, 2i+1) over the first rotary_dim elements of the head, four sandwich norms with
    weight offset 0, a fused gate_up_proj) is keyed on config.model_type == "glm4" and on nothing else."""
    return getattr(config, "model_type", None) == "glm4"


def _head_dim(c) -> int:
    return getattr(c, "head_dim", None) or c.hidden_size // c.num_attention_heads


def rotary_dim(config) -> int:
    """int(head_dim * partial_rotary_factor), the factor from config.rope_parameters first, then from the configuration, as HF's
    rotary-embedding initialisers take it (1.0 when neither has one)."""
    rp = getattr(config, "rope_parameters", None) or getattr(config, "rope_scaling", None) or {}
    prf = rp.get("partial_rotary_factor") if isinstance(rp, dict) else None
    if prf is None:
        prf = getattr(config, "partial_rotary_factor", None)
    return int(_head_dim(config) * (1.0 if prf is None else float(prf)))


def rope_layer_types(c):
    """The layer types that carry their own RoPE parameters: for model_type "olmo3" (HF's Olmo3RotaryEmbedding keeps one set of
    frequencies per layer type) the sorted set of config.layer_types; None for every other model type (one table per model)."""
    if getattr(c, "model_type", None) != "olmo3":
        return None
    types = getattr(c, "layer_types", None)
    if not types:
        raise ValueError("config.layer_types is missing: an olmo3 configuration keeps its rope_parameters per layer type")
    return sorted(set(types))


def _rope_dict(c, layer_type=None) -> dict:
    """The flat RoPE parameter dict of a configuration: config.rope_parameters (transformers 5.x) or the older rope_scaling, with
    rope_type and rope_theta always present (HF's standardisation: the dict's own rope_theta goes before config.rope_theta, and a
    top-level original_max_position_embeddings before the dict's).  A dict nested per layer type is refused - except for
    model_type "olmo3" (rope_layer_types), whose dict MUST be nested with exactly the configuration's layer types as its keys:
    `layer_type` then picks the sub-dict, which goes through the same standardisation."""
    rp = getattr(c, "rope_parameters", None) or getattr(c, "rope_scaling", None) or {}
    if not isinstance(rp, dict):
        raise ValueError(f"config.rope_parameters must be a dict, got {type(rp).__name__}")
    types = rope_layer_types(c)
    if types is not None:
        if sorted(map(str, rp)) != types or not all(isinstance(v, dict) for v in rp.values()):
            raise ValueError(f"config.rope_parameters of an olmo3 configuration must be nested per layer type with exactly the keys "
                             f"{', '.join(types)} (config.layer_types); got {', '.join(map(str, rp)) or 'nothing'}")
        if layer_type not in rp:
            raise ValueError(f"config.rope_parameters is nested per layer type ({', '.join(types)}): name one of them, got {layer_type!r}")
        rp = rp[layer_type]
    elif rp and all(isinstance(v, dict) for v in rp.values()):
        raise ValueError(f"config.rope_parameters is nested per layer type ({', '.join(map(str, rp))}): one RoPE table per model is supported")
    rp = dict(rp)
    rp["rope_type"] = rp.get("rope_type", rp.get("type")) or "default"
    if rp.get("rope_theta") is None:
        theta = getattr(c, "rope_theta", None)
        rp["rope_theta"] = 1e6 if theta is None else theta
    if getattr(c, "original_max_position_embeddings", None) is not None:
        rp["original_max_position_embeddings"] = c.original_max_position_embeddings
    return rp


_ROPE: dict = {}


def is_longrope(c) -> bool:
    """A phi3 configuration with rope_type longrope: two sets of frequencies (short_factor / long_factor), one per call."""
    return is_phi3(c) and _rope_dict(c)["rope_type"] == "longrope"


def longrope_boundary(c) -> int:
    """original_max_position_embeddings of a longrope configuration: a sequence longer than this takes the long factors."""
    return int(_rope_dict(c)["original_max_position_embeddings"])


def rope_of(c, layer_type=None, long=False):
    """(inv_freq [D/2] fp32 on the host, attention_factor) of a configuration (ops.rope_inv_freq), resolved once per distinct
    parameter set: every consumer of one model - the packed pass, the block-wise walk, dense.py, engine.forward, warm_gemm_shapes -
    reaches it through packed_hidden_states and so builds its table from the same frequencies.  `layer_type`: which of the nested
    parameter sets of an olmo3 configuration (rope_layer_types); two layer types with equal parameters resolve to the same pair.
    For phi3 and glm4 the vector has rotary_dim(c) / 2 entries; `long` picks the long_factor set of a longrope configuration
    (ops.longrope_inv_freq; one cached pair per set) and means nothing elsewhere."""
    rp = _rope_dict(c, layer_type)
    D = rotary_dim(c) if is_phi3(c) or is_glm4(c) else _head_dim(c)
    max_pos = getattr(c, "max_position_embeddings", None)
    longrope = is_phi3(c) and rp["rope_type"] == "longrope"
    key = (D, max_pos, bool(long) and longrope, tuple(sorted((k, repr(v)) for k, v in rp.items())))
    hit = _ROPE.get(key)
    if hit is None:
        hit = _ROPE[key] = ops.longrope_inv_freq(D, rp, max_pos, bool(long)) if longrope else ops.rope_inv_freq(D, rp, max_pos)
    return hit


_SOFTCAP_SINK_FIELDS = ("attn_logit_softcapping", "final_logit_softcapping", "attn_softcap", "logit_softcap", "attention_sink",
                        "attention_sinks", "use_attention_sinks", "num_sink_tokens")


def is_gemma2(config) -> bool:
    """Gemma-2 arithmetic (soft-capped attention and final logits, GeGLU, the four `1 + w` sandwich norms, the scaled embedding and
    query_pre_attn_scalar) is keyed on config.model_type == "gemma2" and on nothing else: the same fields on any other configuration
    stay refused by check_supported."""
    return getattr(config, "model_type", None) == "gemma2"


def gemma2_arith(config):
    """(attention scale, attention soft-cap, final-logit soft-cap) of a Gemma-2 configuration; a cap of None or 0 is no cap (0.0)."""
    c = config
    return float(c.query_pre_attn_scalar) ** -0.5, float(getattr(c, "attn_logit_softcapping", None) or 0.0), \
        float(getattr(c, "final_logit_softcapping", None) or 0.0)


def final_softcap_of(model) -> float:
    """The final-logit soft-cap the LM-head kernels apply for `model` (0.0: none)."""
    return gemma2_arith(model.config)[2] if is_gemma2(model.config) else 0.0


def _check_gemma2(c) -> None:
    act = getattr(c, "hidden_activation", None)
    if act != "gelu_pytorch_tanh":
        raise ValueError(f"config.hidden_activation = {act!r} is not supported for gemma2: the MLP kernel computes gelu_pytorch_tanh(gate) * up")
    D = _head_dim(c)
    if D not in (64, 128):
        raise ValueError(f"config.head_dim = {D} is not supported: the attention kernels cover head_dim 64 and 128 (Gemma-2-27B; the 2B / 9B use 256)")
    qs = getattr(c, "query_pre_attn_scalar", None)
    if qs is None or not float(qs) > 0:
        raise ValueError(f"config.query_pre_attn_scalar = {qs!r} is not supported: gemma2 attention scales by query_pre_attn_scalar ** -0.5")
    for f in ("attn_logit_softcapping", "final_logit_softcapping"):
        v = getattr(c, f, None)
        if v is not None and not (0.0 <= float(v) < float("inf")):
            raise ValueError(f"config.{f} = {v!r} is not supported: a soft-cap is a finite number >= 0 (None or 0: no cap)")


def _check_olmo(c) -> None:
    D = _head_dim(c)
    if D not in (64, 128):
        raise ValueError(f"config.head_dim = {D} is not supported for {c.model_type}: the projection-wide q/k norm kernels cover head_dim 64 and 128")
    for f in ("num_attention_heads", "num_key_value_heads"):
        if getattr(c, f) * D > 8192:
            raise ValueError(f"config.{f} * head_dim = {getattr(c, f)} * {D} is not supported: the projection-wide q/k norm kernels hold "
                             f"one row of at most 8192 elements")


def _check_cohere(c) -> None:
    """cohere / cohere2: what the LayerNorm kernel, the attention kernels and the head's temperature take."""
    mt, D, H = c.model_type, _head_dim(c), c.hidden_size
    if D not in (64, 128):
        raise ValueError(f"config.head_dim = {D} is not supported for {mt}: the attention and RoPE kernels cover head_dim 64 and 128")
    if H % 8 or H > 8192:
        raise ValueError(f"config.hidden_size = {H} is not supported for {mt}: the LayerNorm kernel holds one row of a multiple of 8 and at "
                         f"most 8192 elements (Command-R+ and Command-A are wider)")
    if getattr(c, "use_qk_norm", False):
        raise ValueError(f"config.use_qk_norm = True is not supported for {mt} (Command-R+): there is no per-head LayerNorm kernel")
    ls = getattr(c, "logit_scale", None)
    if isinstance(ls, bool) or not isinstance(ls, (int, float)) or not 0.0 < float(ls) < float("inf"):
        raise ValueError(f"config.logit_scale = {ls!r} is not supported for {mt}: the head scales its logits by a finite number > 0")
    act = getattr(c, "hidden_act", None)
    if act != "silu":
        raise ValueError(f"config.hidden_act = {act!r} is not supported for {mt}: the MLP kernels compute silu(gate) * up")
    if mt == "cohere2":
        types = getattr(c, "layer_types", None)
        if not types or len(types) != c.num_hidden_layers:
            raise ValueError(f"config.layer_types has {len(types or [])} entries for {c.num_hidden_layers} layers: a cohere2 layer rotates "
                             f"(sliding_attention) or not (full_attention) by its type")
        for t in types:
            if t not in ("full_attention", "sliding_attention"):
                raise ValueError(f"config.layer_types entry {t!r} is not supported for cohere2 (full_attention / sliding_attention)")
        W = getattr(c, "sliding_window", None)
        if "sliding_attention" in types and not (isinstance(W, int) and not isinstance(W, bool) and W > 0):
            raise ValueError(f"config.sliding_window = {W!r} is not supported for cohere2: a sliding_attention layer needs its window")


def _check_partial_rope(c, training: bool) -> None:
    """phi3 / glm4: the head_dim and rotary_dim the partial RoPE kernels take, longrope's lists (phi3 only), Phi-3's dropouts."""
    mt, D = c.model_type, _head_dim(c)
    if D not in (64, 128):
        raise ValueError(f"config.head_dim = {D} is not supported for {mt}: the attention and RoPE kernels cover head_dim 64 and 128"
                         + (" (Phi-3-mini and Phi-3.5-mini use 96)" if D == 96 else ""))
    R, step = rotary_dim(c), 16 if is_phi3(c) else 8
    if not 0 < R <= D or R % step:
        raise ValueError(f"config partial_rotary_factor gives a rotary dimension of {R} of head_dim {D}, which is not supported for {mt}: "
                         f"the {'half-split' if is_phi3(c) else 'interleaved'} RoPE kernel rotates a multiple of {step} elements, at most head_dim")
    rp = _rope_dict(c)
    if rp["rope_type"] == "longrope" and is_phi3(c):
        if rp.get("original_max_position_embeddings") is None:
            raise ValueError("config.original_max_position_embeddings is missing: longrope picks its factors by it")
        for f in ("short_factor", "long_factor"):
            v = rp.get(f)
            if not isinstance(v, (list, tuple)) or len(v) != R // 2:
                raise ValueError(f"config.rope_parameters[{f!r}] must be a list of {R // 2} numbers (rotary dimension {R}), got "
                                 f"{len(v) if isinstance(v, (list, tuple)) else v!r}")
    for f in ("resid_pdrop", "embd_pdrop"):
        if training and float(getattr(c, f, 0.0) or 0.0) > 0:
            raise ValueError(f"config.{f} = {getattr(c, f)} on a model in training mode is not supported (model.eval(), or set it to 0)")


def check_supported(config, training: bool = True) -> None:
    """Refuses, with a ValueError that names the field, a configuration whose arithmetic the engine cannot honour - it would run,
    and compute something else: a rope_type other than default / linear / llama3 / yarn, rope_parameters nested per layer type,
    partial rotary embedding, an activation other than silu, attention dropout on a model in training mode, router jitter noise,
    attention soft-capping or sinks.  A Gemma-2 configuration (is_gemma2) is the exception for soft-capping and the activation: its
    attn_logit_softcapping / final_logit_softcapping and hidden_activation == "gelu_pytorch_tanh" are honoured; any other activation,
    a head_dim other than 64 / 128 and a missing or non-positive query_pre_attn_scalar are refused.  An OLMo-2 / OLMo-3 configuration
    (is_olmo) needs head_dim 64 / 128 and num_attention_heads * head_dim, num_key_value_heads * head_dim <= 8192 (the projection-wide
    q/k norm kernels); for model_type "olmo3" alone rope_parameters nested per layer type is honoured - its keys must be exactly the
    configuration's layer types, and every sub-dict passes the checks above.  OLMo-1 (model_type "olmo") is refused by name.
    A Phi-3 / Phi-4 or GLM-4 configuration (is_phi3, is_glm4) is the exception for partial rotary embedding: a partial_rotary_factor
    whose rotary_dim is a multiple of 16 (phi3, half-split pairs) or 8 (glm4, interleaved pairs) and at most head_dim is honoured, and
    on phi3 alone rope_type longrope with short_factor and long_factor of rotary_dim / 2 entries and original_max_position_embeddings.
    Refused there: a head_dim other than 64 / 128 (Phi-3-mini's 96), any other rotary_dim, resid_pdrop or embd_pdrop above 0 on a model
    in training mode, longrope on glm4.
    A Cohere / Cohere2 configuration (is_cohere) needs head_dim 64 / 128, hidden_size a multiple of 8 and at most 8192, use_qk_norm off,
    a finite logit_scale > 0 and hidden_act silu; for cohere2, layer_types of full_attention / sliding_attention, one per layer, and a
    sliding_window wherever a layer slides.  attention_bias is honoured."""
    c = config
    gemma = is_gemma2(c)
    partial = is_phi3(c) or is_glm4(c)
    if partial:
        _check_partial_rope(c, training)
    if gemma:
        _check_gemma2(c)
    if getattr(c, "model_type", None) == "olmo":
        raise ValueError("config.model_type = 'olmo' (OLMo-1: LayerNorm without weights, clip_qkv) is not supported; olmo2 and olmo3 are")
    if is_olmo(c):
        _check_olmo(c)
    if is_cohere(c):
        _check_cohere(c)
    for lt in rope_layer_types(c) or [None]:
        rp = _rope_dict(c, lt)
        if rp["rope_type"] not in ops.ROPE_TYPES and not (is_phi3(c) and rp["rope_type"] == "longrope"):
            raise ValueError(f"config.rope_parameters['rope_type'] = {rp['rope_type']!r} is not supported ({' / '.join(ops.ROPE_TYPES)})")
        prf = rp.get("partial_rotary_factor", getattr(c, "partial_rotary_factor", None))
        if not partial and prf is not None and float(prf) != 1.0:
            raise ValueError(f"config partial_rotary_factor = {prf} is not supported: the rotary kernels rotate the whole head")
    act = getattr(c, "hidden_act", None)
    if not gemma and act is not None and act != "silu":         # (Gemma2Config keeps hidden_act as a legacy field; hidden_activation decides)
        raise ValueError(f"config.hidden_act = {act!r} is not supported: the MLP kernels compute silu(gate) * up")
    if training and float(getattr(c, "attention_dropout", 0.0) or 0.0) > 0:
        raise ValueError(f"config.attention_dropout = {c.attention_dropout} on a model in training mode is not supported (model.eval(), or set it to 0)")
    if float(getattr(c, "router_jitter_noise", 0.0) or 0.0) > 0:
        raise ValueError(f"config.router_jitter_noise = {c.router_jitter_noise} is not supported")
    for f in _SOFTCAP_SINK_FIELDS:
        if gemma and f in ("attn_logit_softcapping", "final_logit_softcapping"):
            continue
        if getattr(c, f, None):
            raise ValueError(f"config.{f} = {getattr(c, f)!r} is not supported: the attention kernels have neither soft-capping nor sinks")


_CHECKED = weakref.WeakKeyDictionary()


def _check_olmo_norms(model) -> None:
    """The q_norm / k_norm weights of an OLMo model span the whole projection row: Hq*D and Hkv*D elements (a per-head [D] weight
    is another model's arithmetic)."""
    c = model.config
    D = _head_dim(c)
    for l, layer in enumerate(model.model.layers):
        for name, heads in (("q_norm", c.num_attention_heads), ("k_norm", c.num_key_value_heads)):
            w = getattr(getattr(layer.self_attn, name, None), "weight", None)
            if w is None or w.numel() != heads * D:
                raise ValueError(f"model.layers.{l}.self_attn.{name}.weight has {None if w is None else w.numel()} elements: "
                                 f"{c.model_type} normalises the whole projection row of {heads} * {D}")


def ensure_supported(model) -> None:
    """check_supported(model.config), once per model object and training mode, and lora.check_supported(model) on EVERY call (the engine
    and dense.py call this per call): adapter modules are mutable state - an adapter attached, switched to DoRA or put on lm_head between
    two calls must be seen - and the walk over the module tree is cheap beside a step."""
    training = bool(getattr(model, "training", True))
    if hasattr(model, "named_modules"):
        lora.check_supported(model)
    if is_olmo(model.config) and hasattr(getattr(model, "model", None), "layers"):
        _check_olmo_norms(model)
    try:
        seen = _CHECKED.setdefault(model, set())
    except TypeError:                  # a plain namespace standing in for a model: neither hashable nor weakly referenceable
        return check_supported(model.config, training)
    if training not in seen:
        check_supported(model.config, training)
        seen.add(training)


def _cfg_of(model, longrope_long=False):
    c = model.config
    D = _head_dim(c)
    types = rope_layer_types(c)                  # olmo3: one resolved pair per layer, by the layer's type
    rope = (rope_of(c, long=True) if longrope_long else rope_of(c)) if types is None else [rope_of(c, t) for t in c.layer_types]
    eps = getattr(c, "layer_norm_eps", 1e-5) if is_cohere(c) else getattr(c, "rms_norm_eps", 1e-6)      # Cohere's norm keeps its own field
    return c.num_attention_heads, c.num_key_value_heads, D, float(eps), rope


def _windows_of(model):
    """Sliding window of every decoder layer (0 = full attention), as the HF Qwen2 / Qwen3 configurations define it:
    config.sliding_window where config.layer_types[l] == "sliding_attention"; without layer_types, the rule those config classes
    apply (use_sliding_window and l >= max_window_layers).  A sliding layer without a sliding_window attends in full, as in HF.
    Mistral, Mixtral and Phi-3 (config.model_type) have neither field: every layer slides whenever config.sliding_window is set (HF
    picks the sliding mask for the whole model)."""
    c = model.config
    n = c.num_hidden_layers
    W = getattr(c, "sliding_window", None) or 0
    if getattr(c, "model_type", None) in ("mistral", "mixtral", "phi3"):
        return [int(W)] * n
    types = getattr(c, "layer_types", None)
    if types is not None:
        if len(types) != n:
            raise ValueError(f"config.layer_types has {len(types)} entries for {n} layers")
        bad = [t for t in types if t not in ("full_attention", "sliding_attention")]
        if bad:
            raise ValueError(f"unsupported attention layer type {bad[0]!r} (full_attention / sliding_attention)")
        sliding = [t == "sliding_attention" for t in types]
    else:
        first = getattr(c, "max_window_layers", n)
        sliding = [bool(getattr(c, "use_sliding_window", False)) and l >= (first if first is not None else n) for l in range(n)]
    # HF keeps sliding_window = None when use_sliding_window is off; its attention then gets no window: full attention here too
    return [int(W) if s_ else 0 for s_ in sliding]


def layer_metas(meta, windows, for_window=None):
    """Meta of every layer: `meta` for full layers; for a sliding layer of window W, `for_window(W)` (a packed trie: the windowed
    meta, built once per distinct W - ops.window_meta) or, for a stack-form meta, the same stack form with the window.  A packed
    meta without `for_window` is refused rather than run without the window."""
    out, cache = [], {}
    for W in windows:
        if W <= 0 or meta is None:
            out.append(meta)
            continue
        if W not in cache:
            if for_window is not None:
                cache[W] = for_window(W)
            elif meta.subtree_end is None and meta.runs is None:
                cache[W] = ops.stack_meta(meta.q_offset, W)
            else:
                raise ValueError("a sliding-window layer needs its windowed meta (ops.window_meta); none was given")
        out.append(cache[W])
    return out


def _bias(*mods):
    """The modules' biases concatenated in order (the fused projection GEMMs stack their weights the same way); None when the
    modules have none (HF builds the projections of one group with one flag)."""
    bs = [getattr(m_, "bias", None) for m_ in mods]
    if bs[0] is None:
        return None
    return bs[0] if len(bs) == 1 else torch.cat(bs)


def _project(x, *mods):
    """x through the fused projection of `mods` (q|k|v, gate|up, or one module): ONE base GEMM over the stacked base weights - a module
    that carries a LoRA adapter (lora.resolve) contributes its base_layer's weight and bias - and, where members carry adapters, their
    low-rank terms on the members' column ranges of the fused output (ops.lora_linear: some members only, different ranks, a trainable
    base all work).  Without adapters this is ops.linear, as before.  A group whose bases are quantised (quant.quantize_base) goes
    through ops.quant_linear, which expands the codes per use; shapes and biases are read from the modules, never from a quantised
    module's `weight` (a property that dequantises the whole matrix)."""
    bases, ads = zip(*(lora.resolve(m_) for m_ in mods))
    quantized = [lora.is_quantized(b_) for b_ in bases]
    if any(quantized) and not all(quantized):
        raise ValueError("a fused projection group mixes quantised and plain members: quant.quantize_base(model) quantises all of them")
    bias = _bias(*bases)
    adapters, n0 = [], 0
    for b_, a_ in zip(bases, ads):
        n = lora.base_geometry(b_)[0]
        if a_ is not None:
            adapters.append((n0, n, *a_))
        n0 += n
    if quantized[0]:
        return ops.quant_linear(x, bases, bias, adapters)
    w = bases[0].weight if len(bases) == 1 else ops.stack_rows(*(b_.weight for b_ in bases))
    if not adapters:
        return ops.linear(x, w, bias)
    return ops.lora_linear(x, w, bias, adapters)


def _gemma2_layer_forward(layer, res, delta, cos_sin, attn, Hq, Hkv, D, eps):
    """One Gemma-2 decoder layer in the (residual stream, pending update) convention of _layer_forward: sandwich norms - the attention
    and MLP branch outputs are normalised before they join the residual stream - all with weight offset 1, no q/k norm, no bias, and
    GeGLU.  `attn` carries the layer's scale (query_pre_attn_scalar ** -0.5), soft-cap and window."""
    T = res.shape[0]
    a, m = layer.self_attn, layer.mlp
    res, h = ops.add_rms_norm(res, delta, layer.input_layernorm.weight, eps, 1.0)
    qkv = _project(h, a.q_proj, a.k_proj, a.v_proj).view(T, Hq + 2 * Hkv, D)
    q, k, v = ops.qkv_prep(qkv, None, None, cos_sin, eps, Hq, Hkv)
    o = attn(q, k, v)
    delta = ops.rms_norm(_project(o.reshape(T, Hq * D), a.o_proj), layer.post_attention_layernorm.weight, eps, 1.0)
    res, h = ops.add_rms_norm(res, delta, layer.pre_feedforward_layernorm.weight, eps, 1.0)
    act = ops.geglu_fused(_project(h, m.gate_proj, m.up_proj))
    return res, ops.rms_norm(_project(act, m.down_proj), layer.post_feedforward_layernorm.weight, eps, 1.0)


def _olmo_layer_forward(layer, res, delta, cos_sin, attn, Hq, Hkv, D, eps):
    """One OLMo-2 / OLMo-3 decoder layer in the (residual stream, pending update) convention of _layer_forward: post-norm -
    h = x + norm(attn(x)), y = h + norm(mlp(h)) - with no norm in front of either branch, and q/k norms over the whole projection row
    (ops.qkv_prep_wide).  Each branch reads the raw stream, so the stream is materialised once per branch: ops.rms_norm_add normalises
    the branch output and adds it in one pass, and the layer hands on (y, None)."""
    T = res.shape[0]
    a, m = layer.self_attn, layer.mlp
    x = res if delta is None else res + delta              # (an OLMo layer or the embedding in front never leaves a pending update)
    qkv = _project(x, a.q_proj, a.k_proj, a.v_proj).view(T, Hq + 2 * Hkv, D)
    q, k, v = ops.qkv_prep_wide(qkv, a.q_norm.weight, a.k_norm.weight, cos_sin, eps, Hq, Hkv)
    o = attn(q, k, v)
    h = ops.rms_norm_add(x, _project(o.reshape(T, Hq * D), a.o_proj), layer.post_attention_layernorm.weight, eps)
    act = ops.swiglu_fused(_project(h, m.gate_proj, m.up_proj))
    return ops.rms_norm_add(h, _project(act, m.down_proj), layer.post_feedforward_layernorm.weight, eps), None


def _phi3_layer_forward(layer, res, delta, cos_sin, attn, Hq, Hkv, D, eps):
    """One Phi-3 / Phi-4 decoder layer in the (residual stream, pending update) convention of _layer_forward: pre-norm, with the fused
    modules HF keeps - qkv_proj's output is already q|k|v and gate_up_proj's gate|up, so nothing is stacked.  A table narrower than
    the head (cos_sin [T, R], R < D: Phi-4-mini) rotates the first R elements (ops.qkv_prep_partial); a full one is ops.qkv_prep."""
    T = res.shape[0]
    a, m = layer.self_attn, layer.mlp
    res, h = ops.add_rms_norm(res, delta, layer.input_layernorm.weight, eps)
    qkv = _project(h, a.qkv_proj).view(T, Hq + 2 * Hkv, D)
    if cos_sin.shape[1] < D:
        q, k, v = ops.qkv_prep_partial(qkv, cos_sin, Hq, Hkv, False)
    else:
        q, k, v = ops.qkv_prep(qkv, None, None, cos_sin, eps, Hq, Hkv)
    o = attn(q, k, v)
    res, h = ops.add_rms_norm(res, _project(o.reshape(T, Hq * D), a.o_proj), layer.post_attention_layernorm.weight, eps)
    act = ops.swiglu_fused(_project(h, m.gate_up_proj))
    return res, _project(act, m.down_proj)


def _glm4_layer_forward(layer, res, delta, cos_sin, attn, Hq, Hkv, D, eps):
    """One GLM-4 decoder layer in the (residual stream, pending update) convention of _layer_forward: Gemma-2's sandwich layout - both
    branch outputs are normalised before they join the residual stream - with weight offset 0, biased q/k/v projections, interleaved
    RoPE pairs over the first cos_sin.shape[1] elements of the head, a fused gate_up_proj and SwiGLU."""
    T = res.shape[0]
    a, m = layer.self_attn, layer.mlp
    res, h = ops.add_rms_norm(res, delta, layer.input_layernorm.weight, eps)
    qkv = _project(h, a.q_proj, a.k_proj, a.v_proj).view(T, Hq + 2 * Hkv, D)
    q, k, v = ops.qkv_prep_partial(qkv, cos_sin, Hq, Hkv, True)
    o = attn(q, k, v)
    delta = ops.rms_norm(_project(o.reshape(T, Hq * D), a.o_proj), layer.post_self_attn_layernorm.weight, eps)
    res, h = ops.add_rms_norm(res, delta, layer.post_attention_layernorm.weight, eps)
    act = ops.swiglu_fused(_project(h, m.gate_up_proj))
    return res, ops.rms_norm(_project(act, m.down_proj), layer.post_mlp_layernorm.weight, eps)


def _cohere_layer_forward(layer, res, delta_a, delta_b, cos_sin, attn, Hq, Hkv, D, eps):
    """One Cohere / Cohere2 decoder layer: the parallel block out = x + attn(h) + mlp(h) behind ONE LayerNorm h = LN(x).  The stream
    travels with TWO pending updates - the previous layer's branch outputs - which ops.add_layer_norm joins to it inside the norm's
    pass (x + delta_a + delta_b in fp32, one rounding), so no stand-alone add runs; the layer hands on (x, attn(h), mlp(h)).
    cos_sin [T, D]: interleaved RoPE pairs over the whole head; None: a cohere2 full-attention layer, which does not rotate - q and k
    are the projection's values bit for bit."""
    T = res.shape[0]
    a, m = layer.self_attn, layer.mlp
    res, h = ops.add_layer_norm(res, delta_a, delta_b, layer.input_layernorm.weight, eps)
    qkv = _project(h, a.q_proj, a.k_proj, a.v_proj).view(T, Hq + 2 * Hkv, D)
    q, k, v = ops.qkv_prep_nope(qkv, Hq, Hkv) if cos_sin is None else ops.qkv_prep_partial(qkv, cos_sin, Hq, Hkv, True)
    o = attn(q, k, v)
    act = ops.swiglu_fused(_project(h, m.gate_proj, m.up_proj))
    return res, _project(o.reshape(T, Hq * D), a.o_proj), _project(act, m.down_proj)


def _layer_forward(layer, res, delta, cos_sin, attn, Hq, Hkv, D, eps):
    """One decoder layer over the packed rows.  The hidden state enters as (residual stream, pending update)
    so that each residual add is fused into the RMSNorm that follows it.  hipBLASLt GEMMs through torch;
    everything between them is a HIP kernel of this package."""
    T = res.shape[0]
    a = layer.self_attn
    res, h = ops.add_rms_norm(res, delta, layer.input_layernorm.weight, eps)
    # one projection GEMM for q,k,v (and one for gate,up below): the weights stay separate parameters with
    # their HF names; stacking them is three plain copies whose backward hands out gradient row slices
    qkv = _project(h, a.q_proj, a.k_proj, a.v_proj).view(T, Hq + 2 * Hkv, D)
    qn = getattr(a, "q_norm", None); kn = getattr(a, "k_norm", None)
    q, k, v = ops.qkv_prep(qkv, qn.weight if qn is not None else None, kn.weight if kn is not None else None, cos_sin, eps, Hq, Hkv)
    o = attn(q, k, v)                   # ops.tree_attention over a packed trie, or ops.stack_attention over the KV stack
    attn_out = _project(o.reshape(T, Hq * D), a.o_proj)                                    # LlamaConfig.attention_bias: o_proj too
    res, h = ops.add_rms_norm(res, attn_out, layer.post_attention_layernorm.weight, eps)
    m = layer.mlp
    if hasattr(m, "experts") and hasattr(m, "gate"):       # Qwen3Moe / Mixtral SparseMoeBlock (duck-typed): router + grouped expert GEMMs
        g = m.gate
        norm = getattr(g, "norm_topk_prob", None)
        if norm is None:
            if not hasattr(m, "jitter_noise"):             # MixtralSparseMoeBlock: its router has no flag and always renormalises
                raise AttributeError(f"{type(g).__name__} has no norm_topk_prob and {type(m).__name__} is not a Mixtral block")
            norm = True
        return res, ops.moe_mlp(h, g.weight, m.experts.gate_up_proj, m.experts.down_proj, g.top_k, norm)
    act = ops.swiglu_fused(_project(h, m.gate_proj, m.up_proj))
    return res, _project(act, m.down_proj)                                                # LlamaConfig.mlp_bias


class _ScaleRows(torch.autograd.Function):
    """x * s with s a Python number rounded to x's dtype first (HF Gemma2: hidden_states * tensor(sqrt(hidden_size), dtype=model dtype))."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = float(torch.tensor(s, dtype=x.dtype))
        return x * ctx.s

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def attn_args_of(model):
    """Per-model keyword arguments of ops.tree_attention / ops.stack_attention: Gemma-2's scale and attention soft-cap; {} otherwise
    (scale head_dim ** -0.5, no cap)."""
    if not is_gemma2(model.config):
        return {}
    scale, cap, _ = gemma2_arith(model.config)
    return {"scale": scale, "softcap": cap}


class _LayerRecompute(torch.autograd.Function):
    """Per-layer activation recomputation (for tries whose activations do not fit): the forward runs the layer
    without a graph and keeps only its two inputs — plus, when `keep_attn`, the attention output and lse, so that the
    recomputation in the backward skips the forward attention kernel (a fifth of the attention time at depth).  The
    backward re-runs the layer with a graph and back-propagates through it; parameter gradients accumulate into
    `.grad` directly (nested autograd), input gradients are returned."""

    @staticmethod
    def forward(ctx, fn, keep_attn, res, *deltas):
        # deltas: the pending update of the stream (None behind the embedding or an OLMo layer), or the two of a Cohere layer; the
        # layer returns the stream and as many
        ctx.fn, ctx.has_delta = fn, tuple(d is not None for d in deltas)
        items = []
        with torch.no_grad():
            if keep_attn:
                with ops.AttentionTape("record", items):
                    out = fn(res, *deltas)
            else:
                out = fn(res, *deltas)
        ctx.items = items
        ctx.save_for_backward(res, *(d for d in deltas if d is not None))
        return out

    @staticmethod
    def backward(ctx, g_res, *g_deltas):
        res, *kept = ctx.saved_tensors
        r = res.detach().requires_grad_(True)
        kept = iter(kept)
        ds = [next(kept).detach().requires_grad_(True) if has else None for has in ctx.has_delta]
        with torch.enable_grad():
            if ctx.items:
                with ops.AttentionTape("replay", ctx.items):
                    outs = ctx.fn(r, *ds)
            else:
                outs = ctx.fn(r, *ds)
        ctx.items = None
        live = [(o, g) for o, g in zip(outs, (g_res, *g_deltas)) if o is not None]      # (a layer that leaves no pending update: OLMo)
        torch.autograd.backward(tuple(o for o, _ in live), tuple(g for _, g in live))
        return (None, None, r.grad, *(d.grad if d is not None else None for d in ds))


def packed_hidden_states(model, tokens: torch.Tensor, depth: torch.Tensor, meta, checkpoint_layers: bool = False,
                         attn_keep_bytes: int = 0, attn_of_layer=None, full_layers=0, kept_out=None, embed=None,
                         meta_for_window=None, longrope_long: bool = False) -> torch.Tensor:
    """Final-norm hidden states [T, hidden] of the packed tokens.  `model` is a Qwen3TreeLM or an HF
    Qwen2/Qwen3/Llama/Mistral (and their MoE kin) *ForCausalLM (duck-typed).  `checkpoint_layers`: recompute each layer in the backward, except the first
    `full_layers`, which keep their activations like the plain pass — an int, or a plan `bytes kept by layer 0 -> number of
    layers` that is asked once layer 0 has run in full and its footprint has been measured (the number lands in `kept_out`);
    `attn_keep_bytes`: HBM budget for attention outputs kept across that recomputation (layers are served first to last).
    `attn_of_layer(l)` -> callable (q, k, v) -> o replaces the packed tree attention (the block-wise engine passes the
    stack form bound to layer l's KV stack; `meta` is unused then); `embed(tokens)` replaces the plain embedding lookup (the
    block-wise engine routes the rows' gradients into its fp32 sink instead of a dense [vocab, hidden] gradient per block).
    Sliding-window layers (_windows_of) attend with `meta_for_window(W)` (layer_metas); the stack form gets its window from
    `attn_of_layer`.  `longrope_long`: a longrope model (is_longrope) rotates by its long_factor frequencies in this call."""
    Hq, Hkv, D, eps, rope = _cfg_of(model, longrope_long)
    metas = layer_metas(meta, _windows_of(model), meta_for_window) if attn_of_layer is None else None
    body = model.model
    gemma = is_gemma2(model.config)
    cohere = is_cohere(model.config)
    layer_fwd = (_gemma2_layer_forward if gemma else _olmo_layer_forward if is_olmo(model.config) else _phi3_layer_forward if is_phi3(model.config)
                 else _glm4_layer_forward if is_glm4(model.config) else _cohere_layer_forward if cohere else _layer_forward)
    R = rotary_dim(model.config) if is_phi3(model.config) or is_glm4(model.config) else D          # the table's width: the rotary dimension
    akw = attn_args_of(model)
    res = embed(tokens) if embed is not None else F.embedding(tokens, body.embed_tokens.weight)
    deltas = (None, None) if cohere else (None,)         # the pending update(s) of the stream: a Cohere layer leaves its two branch outputs
    if gemma:            # the normaliser, rounded to the model dtype as HF does; on the embed= path too, so the fp32 sink gets the scaled gradient
        res = _ScaleRows.apply(res, float(model.config.hidden_size) ** 0.5)
    if isinstance(rope, list):           # olmo3: one table per distinct parameter set (rope_of returns one pair object per set)
        tables = {id(r_): ops.rope_cos_sin(depth, D, r_) for r_ in {id(r_): r_ for r_ in rope}.values()}
        cos_sins = [tables[id(r_)] for r_ in rope]
    else:
        cos_sins = [ops.rope_cos_sin(depth, R, rope)] * len(body.layers)
    if cohere and model.config.model_type == "cohere2":                   # NoPE: a full-attention layer gets no table
        cos_sins = [cs if t == "sliding_attention" else None for cs, t in zip(cos_sins, model.config.layer_types)]
    per_layer = tokens.shape[0] * Hq * (D * res.element_size() + 4)             # out + lse of one layer
    n_full = full_layers if isinstance(full_layers, int) else 1
    for li, layer in enumerate(body.layers):
        cos_sin = cos_sins[li]
        attn = attn_of_layer(li) if attn_of_layer is not None else (lambda m_: lambda q, k, v: ops.tree_attention(q, k, v, m_, **akw))(metas[li])
        if li == 0 and callable(full_layers) and checkpoint_layers and torch.is_grad_enabled() and res.is_cuda:
            m0 = torch.cuda.memory_allocated(res.device)
            res, *deltas = layer_fwd(layer, res, *deltas, cos_sin, attn, Hq, Hkv, D, eps)
            n_full = int(full_layers(torch.cuda.memory_allocated(res.device) - m0))
            continue
        # (a layer whose input carries no gradient - the first one behind a frozen embedding, LoRA - runs in full: a recomputed layer
        # whose inputs need no gradient would be cut out of the graph, and its adapters with it)
        if checkpoint_layers and li >= n_full and torch.is_grad_enabled() and (res.requires_grad or any(d is not None and d.requires_grad for d in deltas)):
            keep = attn_of_layer is None and attn_keep_bytes >= per_layer
            if keep:
                attn_keep_bytes -= per_layer
            fn = (lambda layer_, attn_, cs_: lambda r_, *d_: layer_fwd(layer_, r_, *d_, cs_, attn_, Hq, Hkv, D, eps))(layer, attn, cos_sin)
            res, *deltas = _LayerRecompute.apply(fn, keep, res, *deltas)
        else:
            res, *deltas = layer_fwd(layer, res, *deltas, cos_sin, attn, Hq, Hkv, D, eps)
    if kept_out is not None:
        kept_out.append(n_full if checkpoint_layers else len(body.layers))
    if cohere:                           # the last layer's two branch outputs join the stream inside the final norm
        return ops.add_layer_norm(res, *deltas, body.norm.weight, eps)[1]
    return ops.add_rms_norm(res, deltas[0], body.norm.weight, eps, *((1.0,) if gemma else ()))[1]


def head_weight(model) -> torch.Tensor:
    lm = getattr(model, "lm_head", None)
    return lm.weight if lm is not None else model.model.embed_tokens.weight
