"""OLMo-2 / OLMo-3: the tiny configurations behind tests/golden/engine_olmo.pt (scripts/make_golden_olmo.py: the REFERENCE's dense
per-sequence path over unmodified transformers Olmo2ForCausalLM / Olmo3ForCausalLM models in fp32 on the CPU, eager attention), the
checks of the fixture, of the model layer's configuration rules and of the new C entries' refusals, the float64 reference of the two
OLMo row kernels (tests/olmo_ref64.py) against torch autograd and against an emulation of the kernels' roundings, and the engine on the
CPU against the fixture.

* olmo2:      Olmo2ForCausalLM, 4 layers, 4 / 2 heads, head_dim 64 passed explicitly (hidden 32), untied head: q_norm over 256 and
              k_norm over 128 elements, post-norm layers.
* olmo2_d128: the same with 2 / 1 heads and head_dim 128.
* olmo3:      Olmo3ForCausalLM at head_dim 64, sliding_window 24 on layers 0 and 2 (explicit layer_types), rope_parameters nested per
              layer type: sliding layers on the default table, full layers on YaRN (factor 4, original_max_position_embeddings 64, an
              explicit attention_factor).

Every record also holds HF's logprobs with ONE feature removed - fwd_dense_off_wide_norm (q_norm / k_norm applied per head with the
first head_dim weights: what the per-head kernel would compute), and for olmo3 fwd_dense_off_window (a window wider than every
sequence) and fwd_dense_off_yarn (the full layers on the default table) - and the fixture must keep each
max |fwd_dense - fwd_dense_off_*| >= 0.4 (MIN_GAP of tests/test_llama_family_fixture.py).  The post-norm layout cannot be removed by
configuration; it has no record.  tests/test_gpu_engine_olmo.py runs the product engine on these cases."""
import ctypes
import math
import os

import pytest
import torch

import family
import hostmirror
import olmo_ref64 as OR
import rowops_ref64 as R
from dynamictreeattn_amd import synth
from dynamictreeattn_amd.model import _windows_of, check_supported, ensure_supported, is_olmo, make_config, rope_of
from family import _m, att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden_olmo.py read them here)
from hostmirror import _cs, plain_wide  # noqa: F401  (HF's formula: the autograd reference here and the CPU stand-in there)
from test_llama_family_fixture import LLAMA, MIN_GAP

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILE = "engine_olmo.pt"
WINDOW = 24
STD, NORM_STD = 0.1, 0.1           # matrices N(0, STD); post-branch norm weights 1 + N(0, NORM_STD)
QK_NORM_STD = 0.3                  # q_norm / k_norm weights 1 + N(0, QK_NORM_STD): the heads' weights differ, so the per-head mistake shows
CASE_STD = {}
# The weight seeds (CASES) are picked, not arbitrary: at hidden 32 the median gradient ratio of HF's OWN bf16 run of these post-norm
# models against its fp32 run moves between 0.020 and 0.041 with the draw (seeds 40 .. 89 tried; STD 0.06 .. 0.2 does not move it), and
# the GPU tests apply 0.0255.  These three draws put HF itself at 0.0233 / 0.0199 / 0.0215 with logprob errors of 0.034 / 0.029 / 0.039
# (bound 0.08) and feature gaps of 0.8 or more (scripts/make_golden_olmo.py prints all of it).
OLMO2 = dict(vocab_size=256, hidden_size=32, intermediate_size=64, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2,
             head_dim=64, rms_norm_eps=1e-6, tie_word_embeddings=False, max_position_embeddings=256, pad_token_id=None, eos_token_id=None,
             rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
OLMO2_D128 = dict(OLMO2, num_attention_heads=2, num_key_value_heads=1, head_dim=128)
DEFAULT_ROPE = {"rope_type": "default", "rope_theta": 10000.0}
YARN_ROPE = {"rope_type": "yarn", "rope_theta": 10000.0, "factor": 4.0, "original_max_position_embeddings": 64, "attention_factor": 1.0625}
LAYER_TYPES = ["sliding_attention", "full_attention", "sliding_attention", "full_attention"]
OLMO3 = dict(OLMO2, sliding_window=WINDOW, layer_types=LAYER_TYPES,
             rope_parameters={"sliding_attention": DEFAULT_ROPE, "full_attention": YARN_ROPE})
DATA = {"kind": "tau2", "seed": 6, "V": 256, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 128}
# case -> (record name, HF class stem, geometry, data, weight seed)
CASES = {"olmo2": ("olmo2", "Olmo2", OLMO2, DATA, 53), "olmo2_d128": ("olmo2_d128", "Olmo2", OLMO2_D128, DATA, 61),
         "olmo3": ("olmo3", "Olmo3", OLMO3, DATA, 53)}
# feature removed -> the configuration change that removes it ("wide_norm" is not a configuration: hf_model swaps the norm modules)
OFF = {"wide_norm": {}, "window": dict(sliding_window=4096),
       "yarn": dict(rope_parameters={"sliding_attention": DEFAULT_ROPE, "full_attention": DEFAULT_ROPE})}


def offs_of(case):
    return ["wide_norm"] + (["window", "yarn"] if case == "olmo3" else [])


def hf_config(case, off=None, attn="eager", **change):
    """The case's Olmo2Config / Olmo3Config; `off`: one of OFF (that feature removed); further fields through `change`."""
    import copy
    import transformers
    kw = copy.deepcopy(CASES[case][2])
    kw.update(copy.deepcopy(OFF[off]) if off else {})
    kw.update(change)
    c = getattr(transformers, CASES[case][1] + "Config")(**kw)
    c._attn_implementation = attn
    return c


def weights(model, seed, std=STD):
    """Seeded fp32 weights for every parameter of `model`, by name in named_parameters order: q_norm / k_norm 1 + N(0, QK_NORM_STD),
    the other norms 1 + N(0, NORM_STD), every matrix N(0, std)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        if n.endswith(("q_norm.weight", "k_norm.weight")):
            out[n] = 1.0 + QK_NORM_STD * torch.randn(p.shape, generator=g)
        elif n.endswith(("norm.weight", "layernorm.weight")):
            out[n] = 1.0 + NORM_STD * torch.randn(p.shape, generator=g)
        else:
            out[n] = std * torch.randn(p.shape, generator=g)
    return out


class PerHeadNorm(torch.nn.Module):
    """The mistake a per-head kernel makes with a projection-wide weight: RMSNorm over each head of head_dim with the FIRST head_dim
    weights.  Stands in for q_norm / k_norm in the `wide_norm` off-record only; the parameter keeps its name and shape."""

    def __init__(self, norm, head_dim):
        super().__init__()
        self.weight, self.eps, self.D = norm.weight, norm.variance_epsilon, head_dim

    def forward(self, x):
        xf = x.float().unflatten(-1, (-1, self.D))
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)
        return (self.weight[: self.D] * xf).flatten(-2).to(x.dtype)


def hf_model(case, off=None, attn="eager", **change):
    """The unmodified transformers model of `case` with the seeded weights (fp32, train mode); off == "wide_norm": its q_norm / k_norm
    modules replaced by PerHeadNorm over the same parameters."""
    import transformers
    m = getattr(transformers, CASES[case][1] + "ForCausalLM")(hf_config(case, off, attn, **change))
    family.load_weights(m, weights(m, CASES[case][4], CASE_STD.get(case, STD)))
    if off == "wide_norm":
        for layer in m.model.layers:
            a = layer.self_attn
            a.q_norm, a.k_norm = PerHeadNorm(a.q_norm, a.head_dim), PerHeadNorm(a.k_norm, a.head_dim)
    return m.float().train()


def llama_control(case):
    """Llama-shaped wiring of the same sizes (pre-norm layers, no q/k norm, default RoPE, no window) with weights from the same helper:
    the control of the fp32 GPU test - what the engine's gradients deviate by on a model of this size without any of OLMo's features."""
    import transformers
    geo = {k: v for k, v in CASES[case][2].items() if k not in ("sliding_window", "layer_types", "rope_parameters")}
    c = transformers.LlamaConfig(**geo, rope_parameters=dict(DEFAULT_ROPE))
    c._attn_implementation = "eager"
    m = transformers.LlamaForCausalLM(c)
    return family.load_weights(m, weights(m, CASES[case][4], CASE_STD.get(case, STD)))


def seqs_of(case):
    return synth.make_case(CASES[case][3])


def gold(case):
    return torch.load(os.path.join(GOLD, FILE), weights_only=True)[CASES[case][0]]


# ---------------------------------------------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("case", list(CASES))
def test_fixture_names_shapes_and_feature_gaps(case):
    pytest.importorskip("transformers")
    g = gold(case)
    grads = gold_grads(g)
    model = hf_model(case)
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == {n: tuple(v.shape) for n, v in grads.items()}
    assert "lm_head.weight" in grads                                       # untied head
    c = model.config
    assert grads["model.layers.0.self_attn.q_norm.weight"].shape == (c.num_attention_heads * c.head_dim,)
    assert grads["model.layers.3.self_attn.k_norm.weight"].shape == (c.num_key_value_heads * c.head_dim,)
    assert "model.layers.0.post_feedforward_layernorm.weight" in grads and "model.layers.0.input_layernorm.weight" not in grads
    if case == "olmo2":
        assert sum(p.numel() for p in model.parameters()) == 141088
    seqs = seqs_of(case)
    assert len(seqs) == 12 and max(map(len, seqs)) > 3 * WINDOW
    assert len(g["fwd_dense"]) == len(seqs)
    assert {k for k in g if k.startswith("fwd_dense_off_")} == {"fwd_dense_off_" + o for o in offs_of(case)}
    for off in offs_of(case):
        other = g["fwd_dense_off_" + off]
        assert len(other) == len(seqs)
        for lp, o, s in zip(g["fwd_dense"], other, seqs):
            assert lp.shape == o.shape == (len(s) - 1,) and lp.dtype == torch.float32
        gap = max(float((a - b).abs().max()) for a, b in zip(g["fwd_dense"], other))
        assert gap >= MIN_GAP, (off, gap)          # a run that ignores the feature cannot pass the bf16 forward bound (0.08)
    assert all(v > 0 for v in g["grad_norms"].values())
    assert os.path.getsize(os.path.join(GOLD, FILE)) < (1 << 20)


# ---------------------------------------------------------------------------------------------------------------- configuration rules
@pytest.mark.parametrize("case", list(CASES))
def test_check_supported_accepts_olmo(case):
    pytest.importorskip("transformers")
    c = hf_config(case)
    assert is_olmo(c) and c.model_type == ("olmo3" if case == "olmo3" else "olmo2")
    check_supported(c)
    for off in offs_of(case):
        check_supported(hf_config(case, off))
    check_supported(hf_config(case, attention_bias=True))                    # biases work as they do for Llama
    ensure_supported(hf_model(case))                                          # the q_norm / k_norm lengths of the model object


def test_is_olmo_is_keyed_on_the_model_type_alone():
    assert not is_olmo(make_config(dict(LLAMA))) and not is_olmo(make_config(dict(LLAMA, model_type="olmo")))
    assert is_olmo(make_config(dict(LLAMA, model_type="olmo2"))) and is_olmo(make_config(dict(LLAMA, model_type="olmo3")))
    with pytest.raises(ValueError, match="olmo"):                            # OLMo-1 stays refused by name
        check_supported(make_config(dict(LLAMA, model_type="olmo", rope_parameters=dict(DEFAULT_ROPE))))


def test_windows_and_rope_tables_per_layer_type():
    """olmo3: windows from layer_types; one resolved (inv_freq, attention_factor) per layer type, bit-equal to the buffers of HF's
    Olmo3RotaryEmbedding; two layer types with equal parameters share one pair (one table)."""
    pytest.importorskip("transformers")
    m = hf_model("olmo3")
    c = m.config
    assert _windows_of(_m(c)) == [WINDOW, 0, WINDOW, 0]
    assert _windows_of(_m(hf_config("olmo2"))) == [0, 0, 0, 0]
    rot = m.model.rotary_emb
    for lt in ("sliding_attention", "full_attention"):
        inv, factor = rope_of(c, lt)
        assert torch.equal(inv, getattr(rot, lt + "_inv_freq")) and float(factor) == float(getattr(rot, lt + "_attention_scaling"))
    assert float(rope_of(c, "full_attention")[1]) == YARN_ROPE["attention_factor"]
    assert not torch.equal(rope_of(c, "full_attention")[0], rope_of(c, "sliding_attention")[0])
    same = hf_config("olmo3", "yarn")
    assert rope_of(same, "full_attention") is rope_of(same, "sliding_attention")
    with pytest.raises(ValueError, match="nested"):
        rope_of(c)                                                           # a nested configuration: the layer type must be named


@pytest.mark.parametrize("field,change", [
    ("head_dim", dict(head_dim=96)),
    ("hidden_act", dict(hidden_act="gelu")),
    ("num_attention_heads", dict(num_attention_heads=72, head_dim=128)),      # Hq * D = 9216 > 8192
    ("num_key_value_heads", dict(num_attention_heads=64, num_key_value_heads=136, head_dim=64)),
])
@pytest.mark.parametrize("case", ["olmo2", "olmo3"])
def test_check_supported_refuses_olmo_and_names_the_field(case, field, change):
    pytest.importorskip("transformers")
    c = hf_config(case)
    geo = {k: v for k, v in CASES[case][2].items()}
    d = make_config(dict(geo, model_type=c.model_type, hidden_act="silu"))     # a plain namespace works the same way
    check_supported(c); check_supported(d)
    for k, v in change.items():
        setattr(c, k, v); setattr(d, k, v)
    for cfg in (c, d):
        with pytest.raises(ValueError, match=field):
            check_supported(cfg)


def test_nested_rope_parameters_rules():
    pytest.importorskip("transformers")
    nested = {"sliding_attention": dict(DEFAULT_ROPE), "full_attention": dict(YARN_ROPE)}
    # keys that are not the layer types: refused, naming the field
    for bad in ({"sliding_attention": dict(DEFAULT_ROPE)}, dict(nested, chunked_attention=dict(DEFAULT_ROPE)), dict(DEFAULT_ROPE),
                dict(DEFAULT_ROPE, **nested)):
        d = make_config(dict(OLMO3, model_type="olmo3", rope_parameters=bad))
        with pytest.raises(ValueError, match="rope_parameters"):
            check_supported(d)
    # every sub-dict passes the type and partial-rotary checks
    d = make_config(dict(OLMO3, model_type="olmo3", rope_parameters=dict(nested, full_attention={"rope_type": "longrope", "rope_theta": 1e4})))
    with pytest.raises(ValueError, match="rope_type"):
        check_supported(d)
    d = make_config(dict(OLMO3, model_type="olmo3", rope_parameters=dict(nested, full_attention=dict(YARN_ROPE, partial_rotary_factor=0.5))))
    with pytest.raises(ValueError, match="partial_rotary_factor"):
        check_supported(d)
    # a nested dict on any other model type stays refused
    for mt in (None, "llama", "olmo2", "qwen3"):
        kw = dict(OLMO3, rope_parameters=nested)
        if mt is not None:
            kw["model_type"] = mt
        with pytest.raises(ValueError, match="nested"):
            check_supported(make_config(kw))


def test_ensure_supported_checks_the_norm_weight_lengths():
    pytest.importorskip("transformers")
    m = hf_model("olmo2")
    ensure_supported(m)
    a = m.model.layers[1].self_attn
    a.q_norm.weight = torch.nn.Parameter(torch.ones(a.head_dim))             # a per-head weight: another model's arithmetic
    with pytest.raises(ValueError, match=r"layers\.1\.self_attn\.q_norm"):
        ensure_supported(m)


def test_olmo_footprint_counts_what_the_layer_keeps():
    pytest.importorskip("transformers")
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    c = hf_config("olmo2")
    e = TreeTrainingEngine(c, torch.device("cpu"), torch.float32, 128)
    plain = make_config({k: v for k, v in c.to_dict().items() if k != "model_type"})
    mk = lambda cfg: type("M", (), {"config": cfg, "named_modules": lambda self: iter(())})()
    # two streams and two branch outputs in place of two streams and two pre-branch norm outputs: the same count (the docstring)
    assert e._per_token_layer_bytes(mk(c)) == e._per_token_layer_bytes(mk(plain))


# ---------------------------------------------------------------------------------------------------------------- C entries
def test_new_entries_refuse_bad_arguments_without_a_gpu():
    """Refused calls only (a refusal returns before any HIP call), in the documented order: DTA_EINVAL -1, DTA_EUNSUPPORTED -2,
    DTA_EALIGN -3.  One 64-byte aligned host buffer stands for every pointer.  (NH * D is a multiple of head_dim: the rows just over
    8192 are 129 * 64 = 8256 and 65 * 128 = 8320; dta_rmsnorm_bwd's own 8200 is the H of rms_norm_add's backward.)"""
    from dynamictreeattn_amd import _lib
    lib = _lib.lib()
    raw = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(raw) + 63) & ~63
    nan = float("nan")

    def fwd(x=p, w=p, cs=p, y=p, rstd=p, T=4, NH=4, D=64, st=None, eps=1e-6, dtype=0):
        return lib.dta_wide_qk_norm_rope_fwd(x, w, cs, y, rstd, T, NH, D, NH * D if st is None else st, eps, dtype, None)

    def bwd(x=p, w=p, cs=p, dy=p, rstd=p, dx=p, part=None, T=4, NH=4, D=64, st=None, dy_h=None, dtype=0):
        n = NH * D if st is None else st
        return lib.dta_wide_qk_norm_rope_bwd(x, w, cs, dy, rstd, dx, part, T, NH, D, n, n, D if dy_h is None else dy_h, n, dtype, None)

    def add(y=p, w=p, res=p, out=p, yn=None, rstd=p, R_=4, H=64, eps=1e-6, dtype=0):
        return lib.dta_rmsnorm_add_fwd(y, w, res, out, yn, rstd, R_, H, eps, dtype, None)

    for f in (fwd, bwd):
        assert f(x=None) == -1 and f(w=None) == -1 and f(cs=None) == -1 and f(rstd=None) == -1 and f(T=0) == -1 and f(NH=0) == -1
        assert f(NH=129, D=64) == -2 and f(NH=65, D=128) == -2               # NH * D > 8192
        assert f(D=96) == -2 and f(dtype=7) == -2
        assert f(x=p + 2) == -3 and f(w=p + 2) == -3 and f(st=4 * 64 + 4) == -3
        assert f(st=4 * 64 - 8) == -1                                         # a token stride below NH * D
        # the order: a null pointer goes before the dtype, the dtype before the alignment
        assert f(x=None, dtype=7) == -1 and f(x=p + 2, dtype=7) == -2 and f(x=p + 2, D=96) == -2
        assert f(NH=64, D=128) != -2 and f(NH=128, D=64) != -2               # both ways to 8192 are supported
    assert fwd(y=None) == -1 and fwd(eps=nan) == -1 and fwd(y=p + 2) == -3
    assert bwd(dy=None) == -1 and bwd(dx=None) == -1 and bwd(dy=p + 2) == -3 and bwd(dx=p + 2) == -3 and bwd(dy_h=60) == -3
    assert lib.dta_wide_qk_norm_rope_bwd_blocks(1) == 1 and lib.dta_wide_qk_norm_rope_bwd_blocks(37) == 10
    assert lib.dta_wide_qk_norm_rope_bwd_blocks(1 << 20) == 2048
    assert add(y=None) == -1 and add(w=None) == -1 and add(res=None) == -1 and add(out=None) == -1 and add(rstd=None) == -1
    assert add(R_=0) == -1 and add(H=0) == -1 and add(eps=nan) == -1
    assert add(dtype=7) == -2 and add(H=60) == -2 and add(y=None, dtype=7) == -1
    assert add(y=p + 2) == -3 and add(res=p + 2) == -3 and add(out=p + 2) == -3 and add(yn=p + 2) == -3 and add(y=p + 2, H=60) == -2
    assert lib.dta_rmsnorm_bwd(p, p, p, None, p, p, None, 4, 8200, 0.0, 0, None) == -2      # the backward of rms_norm_add: H <= 8192


# ---------------------------------------------------------------------------------------------------------------- float64 reference
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def wide_case(T, NH, D, dtype, seed):
    """(x [T, NH, D], w [NH * D], cos_sin, dy) on rowops_ref64.rows: token scales log-spaced, an all-zero token, a single-element one."""
    from dynamictreeattn_amd import ops
    x = R.rows(T, NH * D, dtype, seed).view(T, NH, D)
    w = R.norm_weight(NH * D, dtype, seed + 1, False)
    depth = torch.randint(0, 16384, (T,), generator=torch.Generator().manual_seed(seed + 2))
    return x, w, ops.rope_cos_sin(depth, D, 1e4), R.randn((T, NH, D), dtype, seed + 3)


def emu_wide_fwd(x, w, cs, eps, dtype):
    """The kernel's documented arithmetic in torch fp32: r over the whole row, a = cast(w x r) (one rounding), y = cast(a c + b s)."""
    xf = x.float()
    T, NH, D = xf.shape
    cos, sin = _cs(cs, D)
    r = torch.rsqrt((xf * xf).sum((1, 2)) / (NH * D) + eps)
    a = (w.float().view(1, NH, D) * (xf * r[:, None, None])).to(dtype).float()
    b = torch.cat([-a[..., D // 2:], a[..., :D // 2]], -1)
    return (a * cos + b * sin).to(dtype), r


def emu_wide_bwd(x, w, cs, dy, rstd, dtype, head_mean=False):
    """(dx, dw); head_mean: the projection term taken per head instead of over the whole row (a corruption)."""
    g = dy.float()
    T, NH, D = g.shape
    cos, sin = _cs(cs, D)
    da = g * cos + torch.cat([g[..., D // 2:], -g[..., :D // 2]], -1) * sin
    r, wf = rstd[:, None, None], w.float().view(1, NH, D)
    t = x.float() * r
    dot = (da * wf * t).mean(-1, keepdim=True) if head_mean else (da * wf * t).sum((1, 2), keepdim=True) / (NH * D)
    return (r * (da * wf - t * dot)).to(dtype), (da * t).sum(0).reshape(-1).to(dtype)


def emu_norm_add(y, w, res, eps, dtype):
    yf = y.float()
    r = torch.rsqrt((yf * yf).sum(-1) / yf.shape[1] + eps)
    yn = (w.float() * (yf * r[:, None])).to(dtype)
    return yn, (res.float() + yn.float()).to(dtype), r


@pytest.mark.parametrize("T,NH,D", [(5, 3, 64), (4, 2, 128), (6, 1, 64)])
def test_wide_reference_matches_autograd(T, NH, D):
    x, w, cs, dy = wide_case(T, NH, D, F32, 10 + NH)
    eps = float(torch.tensor(1e-6, dtype=F32))
    xa, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = plain_wide(xa, wa, cs.double(), eps)
    dx, dw = torch.autograd.grad(y, (xa, wa), dy.double())
    fwd, bwd = OR.wide_fwd_ref(x, w, cs, 1e-6, F32), OR.wide_bwd_ref(x, w, cs, dy, 1e-6, F32)
    for name, got, want in (("y", fwd["y"][0], y.detach()), ("dx", bwd["dx"][0], dx), ("dw", bwd["dw"][0], dw)):
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-13), (name, float((got - want).abs().max()))
    assert all(bool((b >= 0).all()) and bool(torch.isfinite(b).all()) for _, b in list(fwd.values()) + list(bwd.values()))


@pytest.mark.parametrize("R_,H", [(5, 32), (4, 2048)])
def test_norm_add_reference_matches_autograd(R_, H):
    y, res, w = R.rows(R_, H, F32, 3), R.randn((R_, H), F32, 4), R.norm_weight(H, F32, 5, False)
    eps = float(torch.tensor(1e-6, dtype=F32))
    ya, wa, ra = (t.double().requires_grad_(True) for t in (y, w, res))
    out = ra + wa * (ya * torch.rsqrt(ya.pow(2).mean(-1, keepdim=True) + eps))
    g = R.randn((R_, H), F32, 6)
    dy, dw, dres = torch.autograd.grad(out, (ya, wa, ra), g.double())
    ref = OR.norm_add_ref(y, w, res, 1e-6, F32)
    assert torch.allclose(ref["out"][0], out.detach(), rtol=1e-11, atol=1e-13)
    assert torch.equal(dres, g.double())                                       # d res = d out passes through
    bwd = R.rmsnorm_bwd_ref(y, w, g, None, 1e-6, 0.0, F32)                     # the backward the operator uses: the existing reference
    assert torch.allclose(bwd["dx"][0], dy, rtol=1e-11, atol=1e-13) and torch.allclose(bwd["dw"][0], dw, rtol=1e-11, atol=1e-13)


WIDE_SHAPES = [(64, 1), (64, 3), (64, 4), (128, 1), (128, 5), (128, 12), (64, 33), (128, 40), (128, 64), (64, 128)]


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D,NH", WIDE_SHAPES)
def test_wide_emulation_stays_inside_every_bound(D, NH, dtype):
    T = 5
    x, w, cs, dy = wide_case(T, NH, D, dtype, NH + D)
    eps = 1e-6
    y, rstd = emu_wide_fwd(x, w, cs, eps, dtype)
    R.check_all("emu_wide", {"y": y, "rstd": rstd}, OR.wide_fwd_ref(x, w, cs, eps, dtype))
    dx, dw = emu_wide_bwd(x, w, cs, dy, rstd, dtype)
    R.check_all("emu_wide", {"dx": dx, "dw": dw}, OR.wide_bwd_ref(x, w, cs, dy, eps, dtype))


@pytest.mark.parametrize("dtype", [BF, F16])
def test_wide_corruptions_are_rejected(dtype):
    """What the per-head kernel would compute - the norm per head with the first D weights, and its backward's per-head projection -
    is outside the bounds: they tell the two arithmetics apart."""
    T, NH, D = 6, 4, 64
    x, w, cs, dy = wide_case(T, NH, D, dtype, 7)
    fwd, bwd = OR.wide_fwd_ref(x, w, cs, 1e-6, dtype), OR.wide_bwd_ref(x, w, cs, dy, 1e-6, dtype)
    y, rstd = emu_wide_fwd(x, w, cs, 1e-6, dtype)
    import test_rowops_ref64 as TR
    per_head, _ = TR.emu_qk_fwd(x, w[:D], cs, 1e-6, dtype)
    with pytest.raises(AssertionError, match="over the bound"):
        R.check("y", per_head, *fwd["y"])
    dx_bad, _ = emu_wide_bwd(x, w, cs, dy, rstd, dtype, head_mean=True)
    with pytest.raises(AssertionError, match="over the bound"):
        R.check("dx", dx_bad, *bwd["dx"])
    y_bad = y.clone(); y_bad[1] = (y_bad[1].float() * 1.02).to(dtype)
    with pytest.raises(AssertionError, match="over the bound"):
        R.check("y", y_bad, *fwd["y"])


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("R_,H", [(1, 32), (5, 2048), (3, 5120), (3, 16384)])
def test_norm_add_emulation_stays_inside_every_bound(R_, H, dtype):
    y, res, w = R.rows(R_, H, dtype, H), R.randn((R_, H), dtype, H + 1), R.norm_weight(H, dtype, H + 2, False)
    yn, out, rstd = emu_norm_add(y, w, res, 1e-6, dtype)
    ref = OR.norm_add_ref(y, w, res, 1e-6, dtype)
    R.check_all("emu_norm_add", {"yn": yn, "out": out, "rstd": rstd}, ref)
    bad = (res.float() + 1.02 * yn.float()).to(dtype)                        # the branch joined at the wrong weight
    with pytest.raises(AssertionError, match="over the bound"):
        R.check("out", bad, *ref["out"])


# ---------------------------------------------------------------------------------------------------------------- the engine on the CPU
@pytest.mark.parametrize("case", list(CASES))
def test_olmo_engine_on_cpu_matches_the_reference_fixture(case, monkeypatch):
    """The product engine with its device steps replaced by CPU stand-ins (fp32) reproduces the reference's dense logprobs, loss and
    every gradient: the layer wiring (post-norm branches, projection-wide q/k norms, per-layer windows, one RoPE table per layer type)
    is host-side plumbing around the kernels."""
    pytest.importorskip("transformers")
    g = gold(case)
    named = family.check_cpu_engine_matches_fixture(hf_model(case), synth.as_tensors(seqs_of(case)), g, monkeypatch)
    assert set(named) == set(gold_grads(g))


def test_olmo3_on_the_sliding_table_misses_the_fixture(monkeypatch):
    """The per-layer table is not inert: with the full layers forced onto the sliding layers' table the CPU engine is off the fixture
    by the recorded YaRN gap, and equals the fwd_dense_off_yarn record."""
    pytest.importorskip("transformers")
    from dynamictreeattn_amd import model as M
    from dynamictreeattn_amd.token_trie import TokenTrie
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
    hostmirror.install(monkeypatch)
    real = M.rope_of
    monkeypatch.setattr(M, "rope_of", lambda c, layer_type=None: real(c, "sliding_attention" if layer_type else None))
    cpu = torch.device("cpu")
    hf = hf_model("olmo3")
    g = gold("olmo3")
    seqs = synth.as_tensors(seqs_of("olmo3"))
    t = TokenTrie(seqs, device=cpu); t.forward_permute()
    out = TreeTrainingEngine(hf.config, cpu, torch.float32, max(map(len, seqs)), forward_only=True).forward(hf, t)
    assert max(float((a - b).abs().max()) for a, b in zip(out, g["fwd_dense"])) >= MIN_GAP
    assert max(float((a - b).abs().max()) for a, b in zip(out, g["fwd_dense_off_yarn"])) < 1e-4
