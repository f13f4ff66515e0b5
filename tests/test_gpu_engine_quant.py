"""A quantised frozen base through the engine on the GPU (quant.quantize_base, ops.quant_linear).

Model A: a tiny unmodified transformers model with `quantize_base` + `lora.attach(seed=...)`.  Model B: the same geometry with plain
16-bit base weights equal to A's dequantised values (quant.dequantized_state_dict) and the same adapters.  The same trie and the same
PolicyLoss go through engine.backward on both.  B takes the path the engine had before quantisation (stack_rows / transposed-weight
caches, ops.linear / ops.lora_linear), A expands its codes per use - the two runs issue the same GEMMs on the same operand values, so the
loss and every adapter gradient are compared with `torch.equal`.

The criterion is loosened in one case only: if A and B differ AND B differs from a clone of B at other addresses too (the GEMM library
picks by operand address), A may deviate from B by no more than B deviates from its clone, per tensor.  `_compare` prints which
criterion a case was held to.

Cases, fp8 and nf4: Qwen3 geometry (hidden 256, 4 layers, 4 / 2 heads of 64, intermediate 512, vocab 512) on a forked trie of a few
hundred rows and on one of more than 4400 packed rows (the transposed dgrad orientation); Qwen2 geometry (q/k/v biases); Phi-3
geometry (fused qkv_proj / gate_up_proj); adapters on the attention projections only with the MLP quantised and adapter-free; f16; the
forced recomputation grade; engine.mode = "stack" with blocks of 64 rows; tree_forward log-probs.  QuantLinear.weight is not read during
an engine call.  Memory on an 8-layer model: at rest and in use (bounds derived in the tests' docstrings)."""
import copy

import numpy as np
import pytest
import torch

import family
from dynamictreeattn_amd import lora, ops, quant
from dynamictreeattn_amd.losses import PolicyLoss
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMTS = ["nf4", "fp8"]
LOSS = PolicyLoss(clip_low=0.2, clip_high=0.2, entropy_coef=0.01)
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")


def _hf(kind, layers=4, inter=512):
    import transformers as tf
    kw = dict(vocab_size=512, hidden_size=256, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=4, num_key_value_heads=2,
              max_position_embeddings=1024, tie_word_embeddings=True, rms_norm_eps=1e-6, pad_token_id=None, eos_token_id=None, bos_token_id=None,
              rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    if kind == "qwen3":
        c, cls = tf.Qwen3Config(head_dim=64, **kw), tf.Qwen3ForCausalLM
    elif kind == "qwen2":
        c, cls = tf.Qwen2Config(**kw), tf.Qwen2ForCausalLM
    else:
        c, cls = tf.Phi3Config(**kw), tf.Phi3ForCausalLM
    c._attn_implementation = "eager"
    m = cls(c)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g) if n.endswith("norm.weight") else 0.05 * torch.randn(p.shape, generator=g))
    return m.train()


def _pair(kind, fmt, dtype=torch.bfloat16, targets=lora.TARGETS, layers=4, inter=512):
    """(A, B): A quantised with adapters, B plain with A's dequantised base values and the same adapters (lora_B filled: a zero B gives
    zero lora_A gradients)."""
    base = _hf(kind, layers, inter).to(dtype)
    a = copy.deepcopy(base).to(DEV)
    lora.attach(a, 8, 16.0, target_modules=[t for t in targets], seed=3)
    names = quant.quantize_base(a, fmt)
    assert names and all(n.startswith("model.layers.") for n in names)
    b = base.to(DEV)
    missing, unexpected = b.load_state_dict(quant.dequantized_state_dict(a), strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    lora.attach(b, 8, 16.0, target_modules=[t for t in targets], seed=3)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    with torch.no_grad():
        for n, p in pa.items():
            if ".lora_B." in n:
                p.copy_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))))
            if p.requires_grad:
                pb[n].copy_(p)
    return a, b


def _seqs(rows):
    """A forked trie: a 40-token prompt, three groups behind it, rollouts of 60 - 200 tokens; `rows` packed rows at least."""
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, 512, 40).tolist()
    groups = [prompt + rng.integers(0, 512, 20).tolist() for _ in range(3)]
    seqs, total, i = [], 100, 0
    while total < rows:
        n = 60 + (37 * i) % 140
        seqs.append(groups[i % 3] + rng.integers(0, 512, n).tolist()); total += n; i += 1
    seqs.append(list(seqs[1]))                                                     # a duplicate
    return [torch.tensor(s, dtype=torch.int64) for s in seqs]


def _atts(seqs):
    rng = np.random.default_rng(9)
    return [{"advantages": torch.from_numpy(rng.normal(0.5, 0.7, len(s) - 1)).float(), "loss_mask": torch.from_numpy(rng.random(len(s) - 1) < 0.8)}
            for s in seqs]


def _backward(m, seqs, dtype=torch.bfloat16, mode="packed", monkeypatch=None, recompute=False):
    m.zero_grad(set_to_none=True)
    t = TokenTrie(seqs, _atts(seqs), device=torch.device(DEV)); t.backward_permute()
    e = TreeTrainingEngine(m.config, DEV, dtype, 512)
    e.mode = mode
    if recompute:
        e.checkpoint_layers = True
    if mode == "stack":
        monkeypatch.setattr(e, "_stack_block_rows", lambda *a: 64)
    loss = e.backward(m, t, LOSS, 64 if mode == "stack" else 2048)
    torch.cuda.synchronize()
    return loss, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, e


def _compare(label, run_a, run_b, clone_b):
    """loss and gradients of A against B: bitwise, unless B against its clone at other addresses differs as well - then A within B's own
    deviation per tensor."""
    (la, ga), (lb, gb) = run_a(), run_b()
    assert set(ga) == set(gb) and ga, (sorted(set(ga) ^ set(gb))[:4])
    same = la == lb and all(torch.equal(ga[n], gb[n]) for n in ga)
    if same:
        print(f"{label}: bitwise equal ({len(ga)} gradients)")
        return
    lc, gc = clone_b()
    dev_clone = {n: float((gb[n].float() - gc[n].float()).abs().max()) for n in gb}
    dev_a = {n: float((ga[n].float() - gb[n].float()).abs().max()) for n in gb}
    worst = max(dev_a, key=dev_a.get)
    print(f"{label}: A differs from B (loss {la!r} / {lb!r}; worst {worst}: {dev_a[worst]:.3e}); B against its clone: loss {lc!r}, "
          f"worst {max(dev_clone.values()):.3e}")
    assert lc != lb or any(v > 0 for v in dev_clone.values()), f"{label}: A differs from B while B equals its clone bit for bit"
    assert abs(la - lb) <= abs(lc - lb), (la, lb, lc)
    bad = {n: (dev_a[n], dev_clone[n]) for n in gb if dev_a[n] > dev_clone[n]}
    assert not bad, bad


def _check_backward(label, kind, fmt, rows, monkeypatch, dtype=torch.bfloat16, targets=lora.TARGETS, mode="packed", recompute=False, last=None):
    pytest.importorskip("transformers")
    a, b = _pair(kind, fmt, dtype, targets)
    seqs = _seqs(rows)
    adapters = {n for n, p in a.named_parameters() if p.requires_grad}

    def run(m):
        loss, g, e = _backward(m, seqs, dtype, mode, monkeypatch, recompute)
        if last is not None:
            assert e.last_mode.startswith(last), e.last_mode
        return loss, g
    _compare(label, lambda: run(a), lambda: run(b), lambda: run(copy.deepcopy(b)))
    assert {n for n, p in a.named_parameters() if p.grad is not None} == adapters
    assert any(float(p.grad.abs().max()) > 0 for n, p in a.named_parameters() if ".lora_A." in n)


@pytest.mark.parametrize("fmt", FMTS)
def test_qwen3_forked_trie(fmt, monkeypatch):
    _check_backward(f"qwen3/{fmt}/small", "qwen3", fmt, 300, monkeypatch, last="packed")


@pytest.mark.parametrize("fmt", FMTS)
def test_qwen3_transposed_dgrad_orientation(fmt, monkeypatch):
    """More than 4400 packed rows: _dgrad takes the transposed copy, QuantOperand.dgrad the transposed expansion."""
    seqs = _seqs(4400)
    t = TokenTrie(seqs, device=torch.device(DEV))
    assert t.n_tokens >= 4400
    calls = []
    real = ops.dequant_blockwise
    monkeypatch.setattr(ops, "dequant_blockwise", lambda q, s, f, out, transposed=False: (calls.append(bool(transposed)), real(q, s, f, out, transposed))[1])
    _check_backward(f"qwen3/{fmt}/large", "qwen3", fmt, 4400, monkeypatch, last="packed")
    assert any(calls) and not all(calls)


@pytest.mark.parametrize("fmt", FMTS)
def test_qwen2_biases(fmt, monkeypatch):
    _check_backward(f"qwen2/{fmt}", "qwen2", fmt, 300, monkeypatch)


@pytest.mark.parametrize("fmt", FMTS)
def test_phi3_fused_projections(fmt, monkeypatch):
    pytest.importorskip("transformers")
    a, _ = _pair("phi3", fmt)
    att = a.model.layers[0].self_attn
    assert isinstance(att.qkv_proj, quant.QuantLinear) and isinstance(a.model.layers[0].mlp.gate_up_proj, quant.QuantLinear)
    assert isinstance(att.o_proj.base_layer, quant.QuantLinear)
    _check_backward(f"phi3/{fmt}", "phi3", fmt, 300, monkeypatch)


@pytest.mark.parametrize("fmt", FMTS)
def test_attention_adapters_only_with_a_quantised_mlp(fmt, monkeypatch):
    pytest.importorskip("transformers")
    a, _ = _pair("qwen3", fmt, targets=ATTN)
    assert isinstance(a.model.layers[0].mlp.down_proj, quant.QuantLinear) and isinstance(a.model.layers[0].self_attn.q_proj.base_layer, quant.QuantLinear)
    _check_backward(f"qwen3/{fmt}/attention adapters", "qwen3", fmt, 300, monkeypatch, targets=ATTN)


@pytest.mark.parametrize("fmt", FMTS)
def test_f16(fmt, monkeypatch):
    _check_backward(f"qwen3/{fmt}/f16", "qwen3", fmt, 300, monkeypatch, dtype=torch.float16)


@pytest.mark.parametrize("fmt", FMTS)
def test_forced_recomputation(fmt, monkeypatch):
    _check_backward(f"qwen3/{fmt}/recompute", "qwen3", fmt, 300, monkeypatch, recompute=True, last="packed+recompute")


@pytest.mark.parametrize("fmt", FMTS)
def test_blockwise_walk(fmt, monkeypatch):
    _check_backward(f"qwen3/{fmt}/stack", "qwen3", fmt, 300, monkeypatch, mode="stack", last="stack")


@pytest.mark.parametrize("fmt", FMTS)
def test_tree_forward_logprobs_and_no_read_of_the_weight_property(fmt, monkeypatch):
    pytest.importorskip("transformers")
    a, b = _pair("qwen3", fmt)
    seqs = _seqs(300)
    reads = []
    prop = quant.QuantLinear.weight
    monkeypatch.setattr(quant.QuantLinear, "weight", property(lambda self: (reads.append(1), prop.fget(self))[1]))
    outs = []
    for m in (a, b):
        t = TokenTrie(seqs, device=torch.device(DEV)); t.forward_permute()
        outs.append(TreeTrainingEngine(m.config, DEV, torch.bfloat16, 512, forward_only=True).forward(m, t))
    _backward(a, seqs)
    assert not reads, f"QuantLinear.weight was read {len(reads)} times during engine calls"
    same = all(torch.equal(x, y) for x, y in zip(*outs))
    if not same:                                                                   # the module docstring's one exception, for the forward
        t = TokenTrie(seqs, device=torch.device(DEV)); t.forward_permute()
        c = copy.deepcopy(b)
        out_c = TreeTrainingEngine(c.config, DEV, torch.bfloat16, 512, forward_only=True).forward(c, t)
        dev_c = max(float((y - z).abs().max()) for y, z in zip(outs[1], out_c))
        dev_a = max(float((x - y).abs().max()) for x, y in zip(*outs))
        print(f"forward/{fmt}: A against B {dev_a:.3e}, B against its clone {dev_c:.3e}")
        assert dev_c > 0 and dev_a <= dev_c
    assert len(outs[0]) == len(seqs) and all(bool(torch.isfinite(x).all()) for x in outs[0])


@pytest.mark.parametrize("fmt", FMTS)
def test_dgrad_of_a_group_whose_member_rows_are_no_multiple_of_8(fmt, monkeypatch):
    """q|k|v with 12 + 20 + 32 rows at 4096 packed rows: the stacked total (64) would take the transposed orientation, but a member's
    column range of the transposed operand would start off 16 bytes.  QuantOperand.dgrad takes the row-major expansion then - no
    DTA_EALIGN in the backward - and gives dy · W of the dequantised stack; a group of 16 + 16 + 32 rows takes the transposed one."""
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(4096, 64, generator=g).to(torch.bfloat16).to(DEV)
    for rows, want_transposed in (((12, 20, 32), False), ((16, 16, 32), True)):
        mods = [quant.QuantLinear.from_weight((0.05 * torch.randn(r, 128, generator=g)).to(torch.bfloat16).to(DEV), None, fmt) for r in rows]
        op = ops.QuantOperand(mods, torch.bfloat16)
        w = torch.cat([m.weight for m in mods])
        assert torch.equal(op.matrix(False), w)
        seen = []
        real = ops.dequant_blockwise
        monkeypatch.setattr(ops, "dequant_blockwise", lambda q, s, f, out, transposed=False: (seen.append(bool(transposed)), real(q, s, f, out, transposed))[1])
        dx = op.dgrad(dy)
        monkeypatch.setattr(ops, "dequant_blockwise", real)
        assert seen == [want_transposed] * 3, (rows, seen)
        ref = dy @ ops.transpose_2d(w).t() if want_transposed else dy @ w
        assert torch.equal(dx, ref), rows


# ------------------------------------------------------------------------------------------------------------------------------ memory
def _projection_bytes16(m):
    return sum(2 * x.in_features * x.out_features for x in m.modules() if isinstance(x, quant.QuantLinear))


@pytest.mark.parametrize("fmt", FMTS)
def test_memory_at_rest_and_in_use(fmt, monkeypatch):
    """8 layers, hidden 256, intermediate 1024.
    At rest: quantize_base frees the projections' 16-bit bytes P and allocates P * bits / 16 (codes + one fp32 scale per block: 4.5 bits
    per element for nf4, 8.25 for fp8): memory_allocated falls by at least P * (1 - bits / 16), less 1 % for allocator rounding.
    In use: A's peak above its resting level during engine.backward is at most B's plus twice the 16-bit bytes of the largest fused
    group - at most one transient expanded operand per orientation is alive at a time, everything else A allocates B allocates too, and
    B's own peak already holds its cached stacked and transposed copies.  An A that saved the expanded operand per layer would exceed
    the bound by about the whole base."""
    pytest.importorskip("transformers")
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = _hf("qwen3", layers=8, inter=1024).to(torch.bfloat16)
    a = copy.deepcopy(base).to(DEV)
    for p in a.parameters():
        p.requires_grad_(False)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    quant.quantize_base(a, fmt)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    P = _projection_bytes16(a)
    want = P * (1 - quant.BITS_PER_ELEMENT[fmt] / 16)
    print(f"{fmt}: projections {P} bytes at 16 bits; memory_allocated fell by {before - after} (required: {0.99 * want:.0f})")
    assert P == 8 * 2 * (256 * (256 + 128 + 128) + 256 * 256 + 3 * 256 * 1024)
    assert before - after >= 0.99 * want
    lora.attach(a, 8, 16.0, seed=3)
    b = base.to(DEV)
    b.load_state_dict(quant.dequantized_state_dict(a), strict=False)
    lora.attach(b, 8, 16.0, seed=3)
    seqs = _seqs(300)
    above = {}
    for name, m in (("B", b), ("A", a)):
        _backward(m, seqs)                                                         # warm: library workspaces, the allocator's pools
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        rest = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _backward(m, seqs)
        above[name] = torch.cuda.max_memory_allocated() - rest
        m.zero_grad(set_to_none=True)
    group = 2 * (2 * 1024) * 256                                                   # gate|up: [2 * 1024, 256] at 16 bits
    print(f"{fmt}: peak above rest A {above['A']}, B {above['B']}, bound B + {2 * group}; the whole base is {P}")
    assert above["A"] <= above["B"] + 2 * group
