"""LoRA adapters: the cases behind tests/golden/engine_lora.pt (scripts/make_golden_lora.py: the REFERENCE's dense per-sequence path
over unmodified tiny HF models whose projections are wrapped by `RefLora` below - a test-side restatement of the adapter layout, not the
product's module, with its attribute and parameter names - base frozen, fp32, CPU, eager attention), the checks of the fixture, and the
CPU checks of dynamictreeattn_amd.lora: attach (names, shapes, init statistics, what is frozen), merged_state_dict against float64,
detach, every refusal by message, the data-parallel bucket plan, and the product module's forward against the restatement bit for bit.

Cases (geometries, data and base weights of test_llama_family_fixture.py; A, B ~ N(0, AB_STD), B non-zero - with PEFT's zero B every
dA is zero and a ratio means nothing):
* llama3_all7: all seven targets, r = 6 (not a multiple of 8), alpha = 12, fp32 adapters; head_dim 64, untied head.
* mistral_r16: all seven targets, r = 16, bf16 adapters (values drawn in fp32 and rounded to bf16, so that both dtypes hold the same
  numbers); every layer sliding.
* llama3_bias_qv: q_proj and v_proj only, ranks 8 and 4 through rank_pattern (scalings 2 and 4), on the biased Llama.
* qwen3_tied: Qwen3ForCausalLM (q/k-norm, tied head), all seven targets, r = 8.
* mixtral_attn: attention-only adapters, experts and router frozen.
Every record also holds `fwd_dense_off`, the logprobs with the adapters disabled: max |fwd_dense - fwd_dense_off| >= MIN_GAP (0.4, 5x
the bf16 forward tolerance) - a run that ignores the adapters cannot pass.  tests/test_gpu_engine_lora.py runs the product engine."""
import math
import os

import pytest
import torch
import torch.nn as nn

import family
import test_llama_family_fixture as fx
from dynamictreeattn_amd import lora, synth
from family import gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden_lora.py read it here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(GOLD, "engine_lora.pt")
MIN_GAP = fx.MIN_GAP
AB_STD = 0.1
ALL7 = lora.TARGETS
QWEN3 = dict(vocab_size=256, hidden_size=16, intermediate_size=32, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2,
             head_dim=64, rms_norm_eps=1e-6, tie_word_embeddings=True)
# case -> (base model, targets, r, alpha, rank_pattern, adapter dtype in the 16-bit run, seed of A / B)
CASES = {"llama3_all7": ("llama3", ALL7, 6, 12.0, None, torch.float32, 31),
         "mistral_r16": ("mistral", ALL7, 16, 32.0, None, torch.bfloat16, 32),
         "llama3_bias_qv": ("llama3_bias", ("q_proj", "v_proj"), 8, 16.0, {"v_proj": 4}, torch.float32, 33),
         "qwen3_tied": ("qwen3", ALL7, 8, 16.0, None, torch.float32, 34),
         "mixtral_attn": ("mixtral", ("q_proj", "k_proj", "v_proj", "o_proj"), 8, 16.0, None, torch.float32, 35)}


class RefLora(nn.Module):
    """The adapter layout restated: y = base(x) + scaling * B(A(x))."""

    def __init__(self, base, r, alpha):
        super().__init__()
        self.base_layer = base
        self.lora_A = nn.ModuleDict({"default": nn.Linear(base.in_features, r, bias=False)})
        self.lora_B = nn.ModuleDict({"default": nn.Linear(r, base.out_features, bias=False)})
        self.scaling, self.disable_adapters = {"default": alpha / r}, False

    def forward(self, x):
        y = self.base_layer(x)
        return y if self.disable_adapters else y + self.lora_B["default"](self.lora_A["default"](x)) * self.scaling["default"]


def base_model(case, attn="eager"):
    """The unmodified transformers model under `case` with its seeded weights (fp32, train mode)."""
    name = CASES[case][0]
    if name != "qwen3":
        return fx.hf_model(name, attn=attn)
    import transformers
    c = transformers.Qwen3Config(**QWEN3, max_position_embeddings=256, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    c._attn_implementation = attn
    m = transformers.Qwen3ForCausalLM(c)
    return family.load_weights(m, fx.weights(m, 26))


def seqs_of(case):
    name = CASES[case][0]
    return synth.make_case(fx.LLAMA_DATA) if name == "qwen3" else fx.seqs_of(name)


def _rank(case, full_name):
    _, _, r, _, pattern, _, _ = CASES[case]
    for k, v in (pattern or {}).items():
        if full_name.endswith("." + k):
            return v
    return r


def adapter_values(case, model):
    """Seeded A / B values by parameter name, in layer and target order; rounded to bf16 where the case's adapters are bf16."""
    _, targets, _, _, _, dt, seed = CASES[case]
    g = torch.Generator().manual_seed(seed)
    out = {}
    for li, layer in enumerate(model.model.layers):
        for parent, names in lora._GROUPS:
            p = getattr(layer, parent)
            for t in names:
                m = getattr(p, t, None)
                if t not in targets or m is None:
                    continue
                base = getattr(m, "base_layer", m)
                if getattr(getattr(base, "weight", None), "dim", lambda: 0)() != 2:
                    continue
                full = f"model.layers.{li}.{parent}.{t}"
                r = _rank(case, full)
                for key, shape in ((".lora_A.default.weight", (r, base.weight.shape[1])), (".lora_B.default.weight", (base.weight.shape[0], r))):
                    v = AB_STD * torch.randn(shape, generator=g)
                    out[full + key] = v.to(dt).float() if dt != torch.float32 else v
    return out


def wrap_ref(case, model, off=False):
    """`model` with the case's projections wrapped in RefLora, the seeded adapter values loaded, the base frozen."""
    _, targets, _, alpha, _, _, _ = CASES[case]
    vals = adapter_values(case, model)
    for li, layer in enumerate(model.model.layers):
        for parent, names in lora._GROUPS:
            p = getattr(layer, parent)
            for t in names:
                full = f"model.layers.{li}.{parent}.{t}"
                if full + ".lora_A.default.weight" in vals:
                    w = RefLora(getattr(p, t), _rank(case, full), alpha)
                    w.disable_adapters = off
                    setattr(p, t, w)
    for prm in model.parameters():
        prm.requires_grad_(False)
    with torch.no_grad():
        for n, prm in model.named_parameters():
            if n in vals:
                prm.copy_(vals[n]); prm.requires_grad_(True)
    return model


def attach_product(case, model, adapter_dtype=torch.float32):
    """`model` with the case's adapters built by the product's lora.attach and the seeded values loaded."""
    _, targets, r, alpha, pattern, _, _ = CASES[case]
    vals = adapter_values(case, model)
    params = lora.attach(model, r, alpha, targets, dtype=adapter_dtype, rank_pattern=pattern, seed=0)
    lora.load_adapter_state_dict(model, vals)
    return params


def gold(case):
    return torch.load(FIXTURE, weights_only=True)[case]


# ---------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_names_shapes_and_feature_gap(case):
    pytest.importorskip("transformers")
    g = gold(case)
    grads = gold_grads(g)
    model = base_model(case)
    params = attach_product(case, model)
    named = {n: p for n, p in model.named_parameters() if p.requires_grad}
    assert {n: tuple(p.shape) for n, p in named.items()} == {n: tuple(v.shape) for n, v in grads.items()}
    assert len(params) == len(named) and all(".lora_A." in n or ".lora_B." in n for n in named)
    seqs = seqs_of(case)
    assert len(g["fwd_dense"]) == len(g["fwd_dense_off"]) == len(seqs)
    for lp, off, s in zip(g["fwd_dense"], g["fwd_dense_off"], seqs):
        assert lp.shape == off.shape == (len(s) - 1,) and lp.dtype == torch.float32
    gap = max(float((a - b).abs().max()) for a, b in zip(g["fwd_dense"], g["fwd_dense_off"]))
    assert gap >= MIN_GAP, gap
    assert all(v > 0 for v in g["grad_norms"].values())
    assert abs(g["bwd_dense_loss"] - g["bwd_dense_loss_off"]) > 1e-5 * abs(g["bwd_dense_loss"])


def test_fixture_cases_and_size():
    assert set(torch.load(FIXTURE, weights_only=True)) == set(CASES)
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(GOLD, "engine_llama3.pt"))
    g = gold_grads(gold("llama3_bias_qv"))
    assert g["model.layers.0.self_attn.q_proj.lora_A.default.weight"].shape[0] == 8
    assert g["model.layers.0.self_attn.v_proj.lora_A.default.weight"].shape[0] == 4
    assert not any("k_proj" in n or "mlp" in n for n in g)
    assert not any("mlp" in n for n in gold_grads(gold("mixtral_attn")))
    assert gold_grads(gold("llama3_all7"))["model.layers.2.mlp.down_proj.lora_B.default.weight"].shape == (16, 6)


# ---------------------------------------------------------------------------------------------------------------- lora.attach & co
def test_attach_names_shapes_init_and_frozen():
    pytest.importorskip("transformers")
    m = fx.hf_model("llama3")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    params = lora.attach(m, 6, 12.0, seed=5)
    named = dict(m.named_parameters())
    L = m.config.num_hidden_layers
    assert len(params) == 2 * 7 * L
    for n, p in before.items():                                          # every base parameter keeps its value under PEFT's name, frozen
        k = n
        for t in lora.TARGETS:
            k = k.replace(f".{t}.weight", f".{t}.base_layer.weight")
        assert torch.equal(named[k], p) and not named[k].requires_grad, n
    trainable = {n for n, p in named.items() if p.requires_grad}
    assert trainable == {f"model.layers.{l}.{g}.{t}.lora_{ab}.default.weight" for l in range(L) for g, ts in lora._GROUPS for t in ts for ab in "AB"}
    q = m.model.layers[0].self_attn.q_proj
    A, B = q.lora_A["default"].weight, q.lora_B["default"].weight
    assert A.shape == (6, 16) and B.shape == (256, 6) and A.dtype == B.dtype == torch.float32 and q.scaling["default"] == 2.0
    assert all(float(named[n].detach().abs().max()) == 0.0 for n in trainable if ".lora_B." in n)
    # Kaiming-uniform with a = sqrt(5): U(-1/sqrt(in), 1/sqrt(in)) - bound and spread over all A matrices with in = 16
    vals = torch.cat([named[n].reshape(-1) for n in trainable if ".lora_A." in n and named[n].shape[1] == 16])
    bound = 1 / math.sqrt(16)
    assert float(vals.abs().max()) <= bound and float(vals.abs().max()) > 0.9 * bound
    assert abs(float(vals.std()) - bound / math.sqrt(3)) < 0.1 * bound and abs(float(vals.mean())) < 0.05 * bound
    assert q.weight is q.base_layer.weight                               # PEFT's `weight` property: the BASE weight
    m2 = fx.hf_model("llama3"); lora.attach(m2, 6, 12.0, seed=5)         # seeded: reproducible
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))
    with pytest.raises(ValueError, match="target_modules"):
        lora.attach(fx.hf_model("llama3"), 4, 8.0, target_modules=("lm_head",))
    with pytest.raises(ValueError, match="r = 300"):
        lora.attach(fx.hf_model("llama3"), 300, 8.0)


def test_attach_rank_pattern_and_mixtral_experts_stay_plain():
    pytest.importorskip("transformers")
    m = base_model("llama3_bias_qv"); attach_product("llama3_bias_qv", m)
    a = m.model.layers[1].self_attn
    assert a.q_proj.lora_A["default"].weight.shape[0] == 8 and a.v_proj.lora_A["default"].weight.shape[0] == 4
    assert a.q_proj.scaling["default"] == 2.0 and a.v_proj.scaling["default"] == 4.0
    assert not lora.carries_adapter(a.k_proj) and not lora.carries_adapter(m.model.layers[1].mlp.down_proj)
    assert a.q_proj.bias is a.q_proj.base_layer.bias and a.q_proj.bias is not None
    x = base_model("mixtral_attn"); lora.attach(x, 8, 16.0)              # all seven asked: the expert MLP has none of them
    assert sum(lora.carries_adapter(m_) for m_ in x.modules()) == 4 * x.config.num_hidden_layers
    assert not any(p.requires_grad for n, p in x.named_parameters() if ".mlp." in n)
    lora.check_supported(x)


@pytest.mark.parametrize("case", ["llama3_all7", "llama3_bias_qv", "qwen3_tied"])
def test_product_module_forward_equals_the_restatement_bit_for_bit(case):
    pytest.importorskip("transformers")
    a, b = wrap_ref(case, base_model(case)), base_model(case)
    attach_product(case, b)
    ids = torch.tensor(seqs_of(case)[0][:48])[None]
    with torch.no_grad():
        la, lb = a(input_ids=ids, use_cache=False).logits, b(input_ids=ids, use_cache=False).logits
    assert torch.equal(la, lb)
    assert set(dict(a.named_parameters())) == set(dict(b.named_parameters()))
    for mod in b.modules():
        if lora.carries_adapter(mod):
            mod.disable_adapters = True
    with torch.no_grad():
        off = b(input_ids=ids, use_cache=False).logits
        plain = base_model(case)(input_ids=ids, use_cache=False).logits
    assert torch.equal(off, plain) and not torch.equal(off, lb)


def test_state_dict_helpers_merge_and_detach():
    pytest.importorskip("transformers")
    case = "llama3_bias_qv"
    m = base_model(case).to(torch.bfloat16)
    attach_product(case, m)                                              # fp32 adapters over a bf16 base
    sd = lora.adapter_state_dict(m)
    assert set(sd) == set(adapter_values(case, base_model(case))) and all(v.dtype == torch.float32 for v in sd.values())
    plain = base_model(case).to(torch.bfloat16)
    merged = lora.merged_state_dict(m)
    assert set(merged) == set(plain.state_dict())
    worst = 0.0
    for k, w in plain.state_dict().items():
        if k + "" in merged and k.replace(".weight", ".lora_A.default.weight") in sd:
            A, B = sd[k.replace(".weight", ".lora_A.default.weight")].double(), sd[k.replace(".weight", ".lora_B.default.weight")].double()
            s = 4.0 if "v_proj" in k else 2.0
            exact = w.double() + s * (B @ A)
            assert merged[k].dtype == torch.bfloat16
            # one rounding of the exact sum: half a bf16 spacing, at most 2^-8 relative (the fp32 formation adds 2^-24)
            assert torch.all((merged[k].double() - exact).abs() <= 2.0 ** -8 * exact.abs() + 1e-30), k
            worst = max(worst, float((merged[k].double() - w.double()).abs().max()))
        else:
            assert torch.equal(merged[k], w), k
    assert worst > 0.05                                                  # the adapters moved the merged weights
    sd2 = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    lora.load_adapter_state_dict(m, sd2)
    assert all(torch.equal(v, sd2[k]) for k, v in lora.adapter_state_dict(m).items())
    with pytest.raises(KeyError):
        lora.load_adapter_state_dict(m, {k: v for k, v in list(sd.items())[1:]})
    lora.detach(m)
    assert not any(lora.carries_adapter(m_) for m_ in m.modules()) and set(m.state_dict()) == set(plain.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), plain.state_dict().values()))


def test_dp_bucket_plan_holds_the_adapters_only():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import dp
    m = base_model("llama3_all7")
    params = attach_product("llama3_all7", m)
    buckets = dp._buckets(list(m.parameters()), 1 << 20)
    got = [p for b in buckets for p in b]
    assert {id(p) for p in got} == {id(p) for p in params} and len(got) == len(params)
    assert sum(p.numel() for p in got) < sum(p.numel() for p in m.parameters()) // 3


# ---------------------------------------------------------------------------------------------------------------- refusals
def _attached():
    m = fx.hf_model("llama3")
    lora.attach(m, 4, 8.0)
    return m, m.model.layers[1].self_attn.q_proj


def test_check_supported_accepts_attached_models_and_plain_ones():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.model import ensure_supported
    for case in CASES:
        m = base_model(case)
        ensure_supported(m)
        attach_product(case, m)
        ensure_supported(m)
        ensure_supported(wrap_ref(case, base_model(case)))


def test_refusals_name_the_module_and_the_field():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.model import ensure_supported
    m, q = _attached()
    q.use_dora = {"default": True}
    with pytest.raises(ValueError, match=r"layers\.1\.self_attn\.q_proj\.use_dora"):
        ensure_supported(m)
    m, q = _attached()
    q.lora_dropout = nn.ModuleDict({"default": nn.Dropout(0.1)})
    with pytest.raises(ValueError, match=r"q_proj\.lora_dropout"):
        ensure_supported(m)
    m.eval(); ensure_supported(m)                                        # in eval mode dropout is the identity
    m, q = _attached()
    q.lora_A["other"], q.lora_B["other"] = nn.Linear(16, 4, bias=False), nn.Linear(4, 256, bias=False)
    q.scaling["other"] = 1.0
    lora.check_supported(m)                                              # a second adapter that is not active is fine
    q.active_adapters = ["default", "other"]
    with pytest.raises(ValueError, match=r"q_proj\.active_adapters"):
        lora.check_supported(m)
    with pytest.raises(ValueError, match="active_adapters"):
        lora.resolve(q)
    m, q = _attached()
    q.fan_in_fan_out = True
    with pytest.raises(ValueError, match=r"q_proj\.fan_in_fan_out"):
        lora.check_supported(m)
    m, q = _attached()
    q.lora_B["default"] = nn.Linear(4, 256, bias=True)
    with pytest.raises(ValueError, match=r"q_proj\.lora_bias"):
        lora.check_supported(m)
    m, q = _attached()
    q.lora_A["default"].to(torch.float16)                                # fp32 model: neither fp32 nor the model dtype
    with pytest.raises(ValueError, match=r"q_proj\.lora_A.*dtype"):
        lora.check_supported(m)
    m, q = _attached()
    q.lora_A["default"], q.lora_B["default"] = nn.Linear(16, 257, bias=False), nn.Linear(257, 256, bias=False)
    with pytest.raises(ValueError, match=r"q_proj\.lora_A.*r = 257"):
        lora.check_supported(m)


@pytest.mark.parametrize("where", ["lm_head", "embed_tokens", "gate", "experts"])
def test_adapters_off_the_seven_projections_are_refused(where):
    pytest.importorskip("transformers")
    m = base_model("mixtral_attn")
    if where == "lm_head":
        m.lm_head = RefLora(m.lm_head, 4, 8.0)
    elif where == "embed_tokens":
        e = m.model.embed_tokens
        e.lora_embedding_A = nn.ParameterDict({"default": nn.Parameter(torch.zeros(4, 512))})
    elif where == "gate":
        g = m.model.layers[0].mlp.gate
        holder = nn.Module()
        holder.base_layer, holder.lora_A, holder.lora_B, holder.scaling = g, nn.ModuleDict(), nn.ModuleDict(), {}
        holder.weight, holder.top_k = g.weight, getattr(g, "top_k", 2)
        m.model.layers[0].mlp.gate = holder
    else:
        x = m.model.layers[0].mlp.experts
        x.base_layer, x.lora_A, x.lora_B, x.scaling = nn.Identity(), nn.ModuleDict(), nn.ModuleDict(), {}
    with pytest.raises(ValueError, match=where):
        lora.check_supported(m)


def test_a_change_after_the_first_call_is_checked_again_and_attach_refuses_a_second_time():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.model import ensure_supported
    m, q = _attached()
    ensure_supported(m)
    q.use_dora = {"default": True}                                       # the same number of adapted projections as before
    with pytest.raises(ValueError, match=r"q_proj\.use_dora"):
        ensure_supported(m)
    q.use_dora = {"default": False}
    ensure_supported(m)
    m.lm_head = RefLora(m.lm_head, 4, 8.0)                               # an adapter the decoder layers do not count
    with pytest.raises(ValueError, match="lm_head"):
        ensure_supported(m)
    m, q = _attached()
    with pytest.raises(ValueError, match="already carries adapters"):    # a second attach would freeze the first one's adapters
        lora.attach(m, 4, 8.0, target_modules=("q_proj",))
    assert all(p.requires_grad for n, p in m.named_parameters() if ".lora_" in n)
    lora.detach(m)
    assert len(lora.attach(m, 4, 8.0, target_modules=("q_proj",))) == 2 * m.config.num_hidden_layers


def test_merged_and_disabled_adapters_mean_the_base_path():
    pytest.importorskip("transformers")
    m, q = _attached()
    assert lora.resolve(q)[1] is not None and lora.resolve(q)[0] is q.base_layer
    q.disable_adapters = True
    assert lora.resolve(q) == (q.base_layer, None)
    q.disable_adapters, q.merged = False, True
    assert lora.resolve(q) == (q.base_layer, None)
    q.use_dora = {"default": True}                                       # nothing of a merged adapter is computed: nothing to refuse
    lora.check_supported(m)
    plain = m.model.layers[0].mlp
    lora.detach(m)
    assert lora.resolve(plain.up_proj) == (plain.up_proj, None)


# ---------------------------------------------------------------------------------------------------------------- the engine on the CPU
@pytest.mark.parametrize("case", ["llama3_all7", "llama3_bias_qv", "qwen3_tied"])
def test_lora_engine_on_cpu_matches_the_reference_fixture(case, monkeypatch):
    """The product engine with its device steps replaced by the CPU stand-ins of tests/hostmirror.py (fp32: the adapter terms are torch
    expressions there) reproduces the reference's logprobs, loss and every adapter gradient, and gives no frozen parameter a gradient."""
    pytest.importorskip("transformers")
    hf = base_model(case)
    attach_product(case, hf)
    family.check_cpu_engine_matches_fixture(hf, synth.as_tensors(seqs_of(case)), gold(case), monkeypatch)
