"""Qwen3-MoE: the tiny configuration behind tests/golden/engine_qwen3_moe.pt (scripts/make_golden.py qwen3_moe: the REFERENCE's dense
per-sequence path over an HF Qwen3MoeForCausalLM in fp32 on the CPU, with HF's per-expert loop, config._experts_implementation = "eager")
and the checks of the fixture.  Layer 0 is dense (mlp_only_layers = [0]); layers 1 and 2 route every token to 2 of 8 experts whose
intermediate size, 48, is no multiple of the GEMM tile.  The fixture also records every (token, MoE layer)'s top-k experts and routing
margin (k-th minus (k+1)-th router probability): the smallest margin is far above fp32 rounding, so the product must route exactly
alike.  tests/test_gpu_engine_moe.py runs the product engine on it."""
import os

import torch

import family
from dynamictreeattn_amd import synth
from family import att, gold_grads  # noqa: F401  (re-exported: the GPU tests and scripts/make_golden.py read them here)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIXTURE = os.path.join(GOLD, "engine_qwen3_moe.pt")
QWEN3_MOE = dict(vocab_size=512, hidden_size=32, intermediate_size=64, moe_intermediate_size=48, num_experts=8, num_experts_per_tok=2,
                 norm_topk_prob=True, decoder_sparse_step=1, mlp_only_layers=[0], num_hidden_layers=3, num_attention_heads=4,
                 num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-6, rope_theta=1000000.0)
QWEN3_MOE_DATA = {"kind": "tau2", "seed": 7, "V": 512, "G": 3, "sys_len": 30, "turns": 4, "lo": 8, "hi": 20, "cap": 100}
WEIGHT_SEED = 5
ROUTER_STD = 0.5          # router rows drawn wider than the rest: well-separated top-k probabilities
MIN_MARGIN = 1e-5
MOE_LAYERS = (1, 2)


def hf_config(cfg=QWEN3_MOE, attn="eager"):
    import transformers
    c = transformers.Qwen3MoeConfig(
        vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
        moe_intermediate_size=cfg["moe_intermediate_size"], num_experts=cfg["num_experts"], num_experts_per_tok=cfg["num_experts_per_tok"],
        norm_topk_prob=cfg["norm_topk_prob"], decoder_sparse_step=cfg["decoder_sparse_step"], mlp_only_layers=list(cfg["mlp_only_layers"]),
        num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
        num_key_value_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], tie_word_embeddings=cfg.get("tie_word_embeddings", True),
        max_position_embeddings=40960, rms_norm_eps=cfg["rms_norm_eps"], output_router_logits=False,
        rope_parameters={"rope_type": "default", "rope_theta": cfg["rope_theta"]})
    c._attn_implementation = attn
    c._experts_implementation = "eager"
    return c


def moe_weights(model, seed=WEIGHT_SEED, router_std=ROUTER_STD, device="cpu"):
    """Seeded weights for every parameter of `model` (by name, in named_parameters order): norms 1 + N(0, 0.1), router rows N(0, router_std),
    everything else N(0, 0.02) - the same values whatever transformers' own initialisation does (drawn on `device`)."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        if n.endswith("norm.weight"):
            v = 1.0 + 0.1 * torch.randn(p.shape, generator=g, device=device)
        elif n.endswith("mlp.gate.weight"):
            v = router_std * torch.randn(p.shape, generator=g, device=device)
        else:
            v = 0.02 * torch.randn(p.shape, generator=g, device=device)
        out[n] = v
    return out


def hf_qwen3_moe(cfg=QWEN3_MOE, seed=WEIGHT_SEED):
    """transformers.Qwen3MoeForCausalLM of `cfg` with the seeded weights (fp32, train mode)."""
    import transformers
    m = transformers.Qwen3MoeForCausalLM(hf_config(cfg))
    return family.load_weights(m, moe_weights(m, seed))


def gold():
    return torch.load(FIXTURE, weights_only=True)


def test_qwen3_moe_fixture_names_shapes_and_routing_margins():
    g = gold()
    grads = gold_grads(g)
    E, k, H, I, L = (QWEN3_MOE[n] for n in ("num_experts", "num_experts_per_tok", "hidden_size", "moe_intermediate_size", "num_hidden_layers"))
    assert set(g) >= {"fwd_dense", "bwd_dense_loss", "bwd_dense_grads_fp16_scaled", "grad_norms", "topk_ids", "margins"}
    for l in MOE_LAYERS:
        p = f"model.layers.{l}.mlp."
        assert grads[p + "gate.weight"].shape == (E, H)
        assert grads[p + "experts.gate_up_proj"].shape == (E, 2 * I, H) and grads[p + "experts.down_proj"].shape == (E, H, I)
        assert p + "gate_proj.weight" not in grads
    assert grads["model.layers.0.mlp.gate_proj.weight"].shape == (QWEN3_MOE["intermediate_size"], H)
    assert len(grads) == 2 + 11 * L              # embed + final norm; per layer 6 attention + 2 norms + 3 MLP (dense or router + experts)
    seqs = synth.make_case(QWEN3_MOE_DATA)
    assert len(g["fwd_dense"]) == len(seqs) == len(g["topk_ids"]) == len(g["margins"])
    for lp, s, ids, mg in zip(g["fwd_dense"], seqs, g["topk_ids"], g["margins"]):
        assert lp.shape == (len(s) - 1,) and lp.dtype == torch.float32
        assert ids.shape == (len(MOE_LAYERS), len(s), k) and mg.shape == (len(MOE_LAYERS), len(s))
        assert int(ids.min()) >= 0 and int(ids.max()) < E
    assert 60 <= max(map(len, seqs)) <= 100
    every = torch.cat([m.flatten() for m in g["margins"]])
    assert float(every.min()) >= MIN_MARGIN, float(every.min())
    used = torch.cat([i.flatten() for i in g["topk_ids"]]).bincount(minlength=E)
    assert int((used > 0).sum()) == E                                    # every expert is used somewhere
    assert all(v > 0 for v in g["grad_norms"].values())
    assert os.path.getsize(FIXTURE) < 500_000


def test_qwen3_tree_lm_moe_layers_match_hf_names_and_shapes():
    """Qwen3TreeLM with the MoE configuration: HF's parameter names and shapes (layer 0 dense by mlp_only_layers), and the engine's
    activation estimate counts the experts' rows of an MoE layer instead of intermediate_size."""
    from dynamictreeattn_amd.model import Qwen3TreeLM, is_moe_layer, make_config
    from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine, _mlp_elems_per_token
    import transformers
    hf = transformers.Qwen3MoeForCausalLM(hf_config())
    mine = Qwen3TreeLM(QWEN3_MOE)
    assert {n: tuple(p.shape) for n, p in mine.named_parameters()} == {n: tuple(p.shape) for n, p in hf.named_parameters()}
    c = make_config(QWEN3_MOE)
    assert [is_moe_layer(c, l) for l in range(3)] == [False, True, True]
    assert [is_moe_layer(hf.config, l) for l in range(3)] == [type(l.mlp).__name__ == "Qwen3MoeSparseMoeBlock" for l in hf.model.layers]
    k, H, I, E = (QWEN3_MOE[n] for n in ("num_experts_per_tok", "hidden_size", "moe_intermediate_size", "num_experts"))
    assert _mlp_elems_per_token(c, 1) == k * (3 * I + H) + 2 * E and _mlp_elems_per_token(c, 0) == 4 * QWEN3_MOE["intermediate_size"]
    big = make_config(synth.QWEN3_30B_A3B)
    e = TreeTrainingEngine(big, "cpu", torch.bfloat16, 16384)
    D, Hq, Hkv = big.head_dim, big.num_attention_heads, big.num_key_value_heads
    per = 2 * (10 * big.hidden_size + 8 * (3 * 768 + 2048) + 2 * 128 + 4 * (Hq + Hkv) * D)
    assert e._per_token_layer_bytes(type("M", (), {"config": big})()) == per
