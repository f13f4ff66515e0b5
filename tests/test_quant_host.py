"""Quantised frozen base on the host (no GPU): the NF4 code book against its construction and against the C header, the properties of
the host mirror of the two block formats (quant.quantize_host / dequantize_host), and quantize_base / QuantLinear on a CPU stand-in model
(Qwen3TreeLM in bf16 with the device steps replaced by tests/hostmirror.py): module replacement before and after lora.attach, every
refusal by name, the state-dict round trip, the exports against torch expressions, and the engine's loss and adapter gradients against
the run on a model whose base weights ARE the dequantised values."""
import os
import re

import numpy as np
import pytest
import torch

import hostmirror
from dynamictreeattn_amd import lora, quant, synth
from dynamictreeattn_amd.model import Qwen3TreeLM
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
           head_dim=32, rms_norm_eps=1e-6, rope_theta=1000000.0)
DATA = {"kind": "random_tree", "seed": 21, "n_seq": 7, "max_len": 40, "alphabet": 2, "dup": 1}
FMTS = ["nf4", "fp8"]
SEVEN = [f"model.layers.{l}.{p}" for l in range(2) for p in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                                                             "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")]


# ------------------------------------------------------------------------------------------------------------------------ code book
def test_nf4_codebook_follows_its_construction():
    """Eight positive normal quantiles, seven negative ones, zero; sorted and divided by the largest magnitude - in float64 with
    Phi^-1(p) = sqrt(2) erfinv(2p - 1).  The literals agree within 2e-7 (measured: 1.2e-7)."""
    ppf = lambda p: np.sqrt(2.0) * torch.special.erfinv(2 * p - 1).numpy()
    pos = ppf(torch.linspace(0.9677083, 0.5, 9, dtype=torch.float64)[:-1])
    neg = -ppf(torch.linspace(0.9677083, 0.5, 8, dtype=torch.float64)[:-1])
    v = np.sort(np.concatenate([pos, neg, [0.0]]))
    v = v / np.abs(v).max()
    assert len(v) == 16 and len(quant.NF4_CODEBOOK) == 16
    err = np.abs(v - np.array(quant.NF4_CODEBOOK, dtype=np.float64)).max()
    print("construction against the literals:", err)
    assert err <= 2e-7


def test_c_header_table_equals_the_python_copy_bit_for_bit():
    text = open(os.path.join(ROOT, "dynamictreeattn_amd", "csrc", "dta_quant_tables.h")).read()
    body = text[text.index("DTA_NF4_CODEBOOK_BEGIN"):text.index("DTA_NF4_CODEBOOK_END")]
    lits = re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f", body)
    assert len(lits) == 16, lits
    c = np.array([float(x) for x in lits], dtype=np.float32)
    py = np.array(quant.NF4_CODEBOOK, dtype=np.float32)
    assert (c.view(np.uint32) == py.view(np.uint32)).all()
    assert all(float(np.float32(x)) == x for x in quant.NF4_CODEBOOK)              # every literal IS an fp32 value
    mid = quant.midpoints()
    assert mid.dtype == torch.float32 and len(mid) == 15 and bool((mid[1:] > mid[:-1]).all())
    assert int(re.search(r"#define DTA_NF4_BLOCK (\d+)", text).group(1)) == quant.BLOCK["nf4"]
    assert int(re.search(r"#define DTA_FP8_BLOCK (\d+)", text).group(1)) == quant.BLOCK["fp8"]


# ---------------------------------------------------------------------------------------------------------------------- host mirror
def _weight(R, C, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(R, C, generator=g) * torch.exp(2 * torch.randn(R, 1, generator=g))
    w[0, :128] = 0                                                              # an all-zero block in either format
    return w.to(dtype)


@pytest.mark.parametrize("fmt", FMTS)
def test_mirror_error_bound_and_requantisation(fmt):
    B = quant.BLOCK[fmt]
    w = _weight(37, 512, 3)
    q, s = quant.quantize_host(w, fmt)
    assert q.dtype == torch.uint8 and s.dtype == torch.float32 and tuple(s.shape) == (37, 512 // B)
    assert tuple(q.shape) == ((37, 256) if fmt == "nf4" else (37, 512))
    d = quant.dequantize_host(q, s, fmt, torch.float32)
    absmax = w.float().reshape(37, -1, B).abs().amax(-1, keepdim=True)
    err = (d - w.float()).reshape(37, -1, B).abs()
    cb = np.array(quant.NF4_CODEBOOK)
    bound = float(np.diff(cb).max()) / 2 if fmt == "nf4" else 2.0 ** -4
    print(fmt, "worst error / absmax:", float((err / absmax.clamp_min(1e-30)).max()), "bound", bound)
    assert bool((err <= bound * absmax).all())
    assert bool((d[0, :128] == 0).all()) and bool((s[0, :128 // B] == 0).all())
    if fmt == "nf4":
        assert bool((q[0, :64] == 0x77).all())                                   # an all-zero block: code 7
    q2, s2 = quant.quantize_host(d, fmt)
    assert torch.equal(q2, q) and torch.equal(s2, s)


def test_nf4_midpoints_take_the_lower_code_and_nibble_order():
    mid = quant.midpoints()
    x = torch.zeros(1, 64)
    x[0, :15] = mid
    x[0, 15], x[0, 16] = 1.0, -1.0
    x[0, 17:32] = torch.nextafter(mid, torch.full_like(mid, 2.0))
    q, s = quant.quantize_host(x, "nf4")
    codes = torch.stack((q >> 4, q & 15), -1).reshape(-1)
    assert float(s[0, 0]) == 1.0
    assert codes[:15].tolist() == list(range(15)) and codes[15] == 15 and codes[16] == 0
    assert codes[17:32].tolist() == list(range(1, 16))
    assert int(q[0, 0]) == (0 << 4) | 1                                          # element 0 in bits 7..4, element 1 in bits 3..0


# ------------------------------------------------------------------------------------------------------- quantize_base / QuantLinear
def _model(dtype=torch.bfloat16, seed=0):
    return Qwen3TreeLM(dict(CFG)).load_named(mo.init_weights(CFG, seed=seed)).to(dtype)


def _freeze(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("order", ["quantize_then_attach", "attach_then_quantize"])
def test_module_replacement_before_and_after_attach(fmt, order):
    m = _model()
    plain = {k: v.clone() for k, v in m.state_dict().items()}
    if order == "attach_then_quantize":
        lora.attach(m, 4, 8.0, seed=1)
        names = quant.quantize_base(m, fmt)
        assert names == [n + ".base_layer" for n in SEVEN]
    else:
        names = quant.quantize_base(_freeze(m), fmt)
        assert names == SEVEN
        lora.attach(m, 4, 8.0, seed=1)
    lora.check_supported(m)
    for n in SEVEN:
        mod = m.get_submodule(n)
        base = mod.base_layer
        assert isinstance(base, quant.QuantLinear) and lora.carries_adapter(mod)
        assert "weight" not in dict(base.named_parameters()) and set(dict(base.named_buffers())) == {"qweight", "scales"}
        w = plain[n + ".weight"]
        assert (base.out_features, base.in_features, base.fmt, base.block) == (w.shape[0], w.shape[1], fmt, quant.BLOCK[fmt])
        q, s = quant.quantize_host(w, fmt)
        assert torch.equal(base.qweight, q) and torch.equal(base.scales, s)
        assert torch.equal(base.weight, quant.dequantize_host(q, s, fmt, torch.bfloat16)) and base.weight.dtype == torch.bfloat16
        x = torch.randn(3, w.shape[1]).bfloat16()
        assert torch.equal(base(x), torch.nn.functional.linear(x, base.weight))
    # embeddings and norms stay as they were
    assert torch.equal(m.model.embed_tokens.weight, plain["model.embed_tokens.weight"])
    assert lora.rank_elems_per_token(m) == 7 * 4
    lora.detach(m)
    assert isinstance(m.model.layers[0].self_attn.q_proj, quant.QuantLinear)


def test_every_refusal_names_the_module_and_the_field():
    with pytest.raises(ValueError, match=r"q_proj\.weight\.requires_grad.*freeze it or attach adapters first"):
        quant.quantize_base(_model())
    with pytest.raises(ValueError, match=r"fmt = 'int3'"):
        quant.quantize_base(_freeze(_model()), "int3")
    with pytest.raises(ValueError, match=r"q_proj\.weight\.dtype = torch\.float32.*fp32 model"):
        quant.quantize_base(_freeze(_model(torch.float32)))
    small = dict(CFG, hidden_size=64, head_dim=16)
    m = _freeze(Qwen3TreeLM(small).load_named(mo.init_weights(small, seed=0)).bfloat16())
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_proj\.in_features = 64 is not a multiple of the fp8 block of 128"):
        quant.quantize_base(m, "fp8")
    assert not any(isinstance(x, quant.QuantLinear) for x in m.modules())         # refused before anything was replaced
    assert len(quant.quantize_base(m, "nf4")) == 14                                 # 64 is a whole nf4 block
    with pytest.raises(ValueError, match=r"q_proj\.qweight.*already quantised"):
        quant.quantize_base(m, "nf4")
    m = _freeze(_model())
    with torch.no_grad():
        m.model.layers[1].mlp.up_proj.weight[3, 5] = float("inf")
    with pytest.raises(ValueError, match=r"layers\.1\.mlp\.up_proj\.weight holds non-finite"):
        quant.quantize_base(m)
    assert not any(isinstance(x, quant.QuantLinear) for x in m.modules())


@pytest.mark.parametrize("fmt", FMTS)
def test_state_dict_round_trip_and_exports(fmt):
    a = _model(seed=0); lora.attach(a, 4, 8.0, seed=1); quant.quantize_base(a, fmt)
    with torch.no_grad():
        for n, p in a.named_parameters():
            if ".lora_B." in n:
                p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))))
    sd = a.state_dict()
    assert "model.layers.0.self_attn.q_proj.base_layer.qweight" in sd and "model.layers.0.self_attn.q_proj.base_layer.scales" in sd
    assert not any(k.endswith("base_layer.weight") for k in sd)
    b = _model(seed=5); lora.attach(b, 4, 8.0, seed=2); quant.quantize_base(b, fmt)      # quantised the same way, other values
    b.load_state_dict(sd)
    for (k, v), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    plain = quant.dequantized_state_dict(a)
    merged = lora.merged_state_dict(a)
    ref = _model(seed=0)
    assert set(plain) == set(merged) == set(ref.state_dict())
    for n in SEVEN:
        mod = a.get_submodule(n)
        w = quant.dequantize_host(mod.base_layer.qweight, mod.base_layer.scales, fmt, torch.bfloat16)
        assert torch.equal(plain[n + ".weight"], w)
        A, B = mod.lora_A["default"].weight, mod.lora_B["default"].weight
        assert torch.equal(merged[n + ".weight"], (w.float() + 2.0 * (B.float() @ A.float())).to(torch.bfloat16))
    assert torch.equal(plain["model.norm.weight"], ref.state_dict()["model.norm.weight"])
    ref.load_state_dict(plain)                                                     # plain HF keys: a model nobody quantised takes them


def test_scales_stay_fp32_through_a_dtype_cast():
    m = _freeze(_model()); quant.quantize_base(m, "nf4")
    s = m.model.layers[0].mlp.down_proj.scales.clone()
    m.half()
    d = m.model.layers[0].mlp.down_proj
    assert d.scales.dtype == torch.float32 and torch.equal(d.scales, s)
    # the dtype the weight expands to follows the cast: the property, the geometry the adapter checks read, and the module's own forward
    assert d.dtype == torch.float16 and d.weight.dtype == torch.float16 and lora.base_geometry(d)[2] == torch.float16
    assert d(torch.randn(2, d.in_features).half()).dtype == torch.float16
    assert torch.equal(d.weight, quant.dequantize_host(d.qweight, d.scales, "nf4", torch.float16))
    m.to("cpu")                                                                    # a move alone changes nothing
    assert d.dtype == torch.float16 and d.scales.dtype == torch.float32


def test_a_foreign_quantised_module_is_not_taken_for_this_format():
    """GPTQ / AWQ linears also carry `qweight` and `scales`; only a module whose `fmt` is one of quant.BLOCK is routed to ops.quant_linear."""
    foreign = torch.nn.Module()
    foreign.qweight, foreign.scales, foreign.in_features, foreign.out_features = torch.zeros(4, 4, dtype=torch.int32), torch.ones(4), 32, 4
    assert not lora.is_quantized(foreign) and lora.base_geometry(foreign) is None
    foreign.fmt = "gptq"
    assert not lora.is_quantized(foreign)
    assert set(lora.QUANT_FORMATS) == set(quant.BLOCK)
    own = _freeze(_model()); quant.quantize_base(own, "fp8")
    assert lora.is_quantized(own.model.layers[0].self_attn.q_proj)


# ----------------------------------------------------------------------------------------------------------------- stand-in engine
def _engine_backward(m, seqs, mode):
    att = [{"w_logprobs": -1.0 - 0.01 * i, "w_entropy": 0.1 + 0.003 * i} for i in range(len(seqs))]
    t = TokenTrie(seqs, att, device=CPU); t.backward_permute()
    e = TreeTrainingEngine(m.config, CPU, torch.bfloat16, max(map(len, seqs))); e.mode = mode
    loss = e.backward(m, t, mo.default_loss, 16)
    return loss, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("targets", [lora.TARGETS, ("q_proj", "v_proj")], ids=["all7", "qv"])
@pytest.mark.parametrize("mode", ["packed", "stack"])
@pytest.mark.parametrize("fmt", FMTS)
def test_stand_in_engine_equals_the_run_on_the_dequantised_base(fmt, mode, targets, monkeypatch):
    """Model A: quantised base + adapters.  Model B: plain bf16 base weights equal to A's dequantised values, the same adapters.  Host
    tensors take the same torch expressions on the same values: loss and every adapter gradient are equal; and the engine call never reads
    QuantLinear.weight."""
    hostmirror.install(monkeypatch)
    seqs = synth.as_tensors(synth.make_case(DATA))
    a = _model(); quant.quantize_base(_freeze(a), fmt); lora.attach(a, 4, 8.0, target_modules=targets, seed=1)
    b = _model(); b.load_state_dict(quant.dequantized_state_dict(a)); lora.attach(b, 4, 8.0, target_modules=targets, seed=1)
    with torch.no_grad():
        for (n, p), (_, p2) in zip(((n, p) for n, p in a.named_parameters() if ".lora_B." in n), ((n, p) for n, p in b.named_parameters() if ".lora_B." in n)):
            p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n)))); p2.copy_(p)
    reads = []
    prop = quant.QuantLinear.weight
    monkeypatch.setattr(quant.QuantLinear, "weight", property(lambda self: (reads.append(1), prop.fget(self))[1]))
    loss_a, ga = _engine_backward(a, seqs, mode)
    assert not reads
    loss_b, gb = _engine_backward(b, seqs, mode)
    assert ga and set(ga) == set(gb) == {n for n, p in a.named_parameters() if p.requires_grad}
    assert loss_a == loss_b
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert any(float(g.abs().max()) > 0 for n, g in ga.items() if ".lora_A." in n)
