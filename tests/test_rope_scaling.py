"""RoPE parameters from the configuration: the host-side restatement (ops.rope_inv_freq, model.rope_of) against transformers' own
ROPE_INIT_FUNCTIONS bit for bit, the cos/sin table (ops.rope_cos_sin) against LlamaRotaryEmbedding on positions 0..16383, and the
default table against the formula the table was built from before scaled types existed."""
import pytest
import torch

from dynamictreeattn_amd import ops
from dynamictreeattn_amd.model import make_config, rope_of

LLAMA31 = {"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
           "original_max_position_embeddings": 8192}
LLAMA32 = dict(LLAMA31, factor=32.0)
QWEN3_YARN = {"rope_type": "yarn", "rope_theta": 1000000.0, "factor": 4.0, "original_max_position_embeddings": 32768}
GRID = [("llama3.1", LLAMA31, 131072), ("llama3.2", LLAMA32, 131072), ("qwen3-yarn", QWEN3_YARN, 131072),
        ("yarn-knobs", dict(QWEN3_YARN, beta_fast=16, beta_slow=2, mscale=1.0, mscale_all_dim=0.707, truncate=False), 131072),
        ("yarn-attention-factor", dict(QWEN3_YARN, attention_factor=1.25), 131072),
        ("yarn-implicit-factor", dict(QWEN3_YARN, factor=None), 65536),
        ("tiny-llama3", dict(LLAMA31, rope_theta=10000.0, original_max_position_embeddings=32), 256),
        ("linear2", {"rope_type": "linear", "rope_theta": 10000.0, "factor": 2.0}, 8192),
        ("linear4", {"rope_type": "linear", "rope_theta": 1000000.0, "factor": 4.0}, 8192)]


def _hf_config(rp, D, max_pos):
    import transformers
    return transformers.LlamaConfig(vocab_size=32, hidden_size=2 * D, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                    num_key_value_heads=1, head_dim=D, max_position_embeddings=max_pos, rope_parameters=dict(rp))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name,rp,max_pos", GRID, ids=[g[0] for g in GRID])
def test_inv_freq_and_attention_factor_equal_transformers(name, rp, max_pos, D):
    pytest.importorskip("transformers")
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    c = _hf_config(rp, D, max_pos)
    ref_inv, ref_factor = ROPE_INIT_FUNCTIONS[rp["rope_type"]](c, "cpu")
    inv, factor = rope_of(c)
    assert inv.dtype == torch.float32 and inv.shape == (D // 2,) and torch.equal(inv, ref_inv)
    assert float(factor) == float(ref_factor)
    # the same dict through make_config (Qwen3TreeLM) and through the pre-5.x field names (rope_scaling + rope_theta)
    plain = {k: v for k, v in rp.items() if v is not None}
    mine = make_config(dict(vocab_size=32, hidden_size=2 * D, num_attention_heads=2, num_key_value_heads=1, head_dim=D,
                            max_position_embeddings=max_pos, rope_parameters=plain))
    assert torch.equal(rope_of(mine)[0], ref_inv) and float(rope_of(mine)[1]) == float(ref_factor)
    old = make_config(dict(vocab_size=32, hidden_size=2 * D, num_attention_heads=2, num_key_value_heads=1, head_dim=D,
                           max_position_embeddings=max_pos, rope_theta=plain["rope_theta"],
                           rope_scaling={("type" if k == "rope_type" else k): v for k, v in plain.items() if k != "rope_theta"}))
    assert torch.equal(rope_of(old)[0], ref_inv) and float(rope_of(old)[1]) == float(ref_factor)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name,rp,max_pos", GRID[:3] + GRID[7:8], ids=[g[0] for g in GRID[:3] + GRID[7:8]])
def test_cos_sin_table_equals_llama_rotary_embedding(name, rp, max_pos, D):
    """Positions 0..16383 on the CPU, bit for bit: the half-table is cos[..., :D/2] (HF concatenates the frequencies with themselves)."""
    pytest.importorskip("transformers")
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    c = _hf_config(rp, D, max_pos)
    pos = torch.arange(16384)
    cos, sin = LlamaRotaryEmbedding(c)(torch.zeros(1, dtype=torch.float32), pos[None])
    table = ops.rope_cos_sin(pos.to(torch.int32), D, rope_of(c))
    assert table.dtype == torch.float32 and table.shape == (16384, D)
    assert torch.equal(table[:, :D // 2], cos[0, :, :D // 2]) and torch.equal(table[:, D // 2:], sin[0, :, :D // 2])


@pytest.mark.parametrize("D,theta", [(64, 1e6), (128, 1e6), (128, 1e4), (64, 5e5)])
def test_default_table_is_the_bytes_of_the_plain_theta_table(D, theta):
    depth = torch.cat([torch.arange(0, 600), torch.tensor([4095, 16383])]).to(torch.int32)
    inv = 1.0 / (float(theta) ** (torch.arange(0, D, 2, dtype=torch.int64).to(torch.float32) / D))       # the formula written out
    ang = depth.float()[:, None] * inv[None, :]
    want = torch.cat([ang.cos(), ang.sin()], dim=-1).contiguous()
    for c in (make_config(dict(hidden_size=2 * D, num_attention_heads=2, head_dim=D, rope_theta=theta)),
              make_config(dict(hidden_size=2 * D, num_attention_heads=2, head_dim=D, rope_parameters={"rope_type": "default", "rope_theta": theta})),
              make_config(dict(hidden_size=2 * D, num_attention_heads=2, head_dim=D, rope_theta=theta, rope_scaling=None))):
        assert torch.equal(ops.rope_cos_sin(depth, D, rope_of(c)), want)
    assert torch.equal(ops.rope_cos_sin(depth, D, theta), want)                                            # the plain-theta call


def test_tables_are_cached_by_value_not_by_theta():
    D, depth = 64, torch.arange(256, dtype=torch.int32)
    plain = ops.rope_cos_sin(depth, D, 10000.0)
    scaled = ops.rope_cos_sin(depth, D, ops.rope_inv_freq(D, {"rope_type": "linear", "rope_theta": 10000.0, "factor": 4.0}))
    assert not torch.equal(plain, scaled)
    assert torch.equal(ops.rope_cos_sin(depth, D, 10000.0), plain)
    yarn = ops.rope_inv_freq(D, {"rope_type": "yarn", "rope_theta": 10000.0, "factor": 4.0, "original_max_position_embeddings": 32})
    assert yarn[1] > 1.0 and float(ops.rope_cos_sin(depth, D, yarn)[0, 0]) == pytest.approx(yarn[1])     # cos(0) * attention_factor


def test_unknown_rope_type_is_refused():
    with pytest.raises(ValueError, match="rope_type"):
        ops.rope_inv_freq(64, {"rope_type": "dynamic", "rope_theta": 1e4, "factor": 2.0})
