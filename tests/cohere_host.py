"""CPU stand-ins for the Cohere ops: HF's own formulas - CohereLayerNorm (mean-centred, the weight multiplied in fp32, one rounding),
the residual join x + delta_a + delta_b, the q|k|v split of a layer without RoPE - and an LM head that honours the temperature the
engine hands it for config.logit_scale (hostmirror's drops unknown keywords: no family before had one).  install(monkeypatch) goes
BEFORE hostmirror.install (family.check_cpu_engine_matches_fixture calls that itself) and after partial_rope_host.install, whose
interleaved rotation and windowed stack attention the Cohere layers use: the head is put in hostmirror's own place, from where
hostmirror.install hands it to the product; tests/hostmirror.py keeps its fixed set."""
import torch

import hostmirror
import partial_rope_host


def plain_layer_norm(x, w, eps):
    """transformers' CohereLayerNorm.forward."""
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = (xf - mean).pow(2).mean(-1, keepdim=True)
    return (w.float() * ((xf - mean) * torch.rsqrt(var + eps))).to(x.dtype)


def _cpu_add_layer_norm(x, delta_a, delta_b, w, eps):
    if delta_a is not None:
        x = x + delta_a                      # CohereDecoderLayer: residual + hidden_states_attention + hidden_states_mlp
    if delta_b is not None:
        x = x + delta_b
    return x, plain_layer_norm(x, w, eps)


def _cpu_qkv_prep_nope(qkv, Hq, Hkv):
    return tuple(qkv.split([Hq, Hkv, Hkv], dim=1))


_plain_lm_head_rows = hostmirror._cpu_lm_head_rows


def _cpu_lm_head_rows(h, W, *args, temperature=1.0, **kw):
    """hostmirror's head on W / temperature: logits (h W^T) / temperature, as the kernels take them."""
    return _plain_lm_head_rows(h, W if temperature == 1.0 else W / temperature, *args, **kw)


def install(monkeypatch):
    from dynamictreeattn_amd import ops
    if hostmirror._cpu_stack_attention is not partial_rope_host._cpu_stack_attention:
        partial_rope_host.install(monkeypatch)
    monkeypatch.setattr(ops, "layer_norm", plain_layer_norm)
    monkeypatch.setattr(ops, "add_layer_norm", _cpu_add_layer_norm)
    monkeypatch.setattr(ops, "qkv_prep_nope", _cpu_qkv_prep_nope)
    if hostmirror._cpu_lm_head_rows is not _cpu_lm_head_rows:
        monkeypatch.setattr(hostmirror, "_cpu_lm_head_rows", _cpu_lm_head_rows)
