"""tests/partial_rope_ref64.py on the CPU: an honest fp32 emulation of the partial RoPE kernels' arithmetic stays inside the float64
bounds in bf16, f16 and fp32 storage - both pairings, both directions, the products summed plainly or through an fma - and each of
four deliberate errors falls outside them: the other pairing, a rotary dimension off by 16, a rotated pass-through region, and the
forward's sign of sin in the backward."""
import pytest
import torch

import partial_rope_ref64 as PR
import rowops_ref64 as R
from dynamictreeattn_amd import ops

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
HALF_SPLIT = [(64, 16), (64, 48), (64, 64), (128, 32), (128, 96), (128, 112), (128, 128)]
INTERLEAVED = [(64, 8), (64, 32), (64, 64), (128, 64), (128, 120), (128, 128)]
CASES = [(0, D, r) for D, r in HALF_SPLIT] + [(1, D, r) for D, r in INTERLEAVED]


def _inputs(T, NH, D, rot, dtype, seed):
    x = R.rows(T, NH * D, dtype, seed).view(T, NH, D)
    depth = torch.randint(1, 131072, (T,), generator=torch.Generator().manual_seed(seed + 2))
    return x, ops.rope_cos_sin(depth, rot, 1e4), R.randn((T, NH, D), dtype, seed + 3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing,D,rot", CASES)
def test_honest_emulation_is_inside_the_bounds(pairing, D, rot, dtype):
    worst = {}
    for T, NH in ((1, 1), (5, 3), (37, 4)):
        x, cs, dy = _inputs(T, NH, D, rot, dtype, T + NH + D + rot)
        for fused in (False, True):
            y = PR.emulate(x, cs, pairing, 1.0, fused)
            dx = PR.emulate(dy, cs, pairing, -1.0, fused)
            for k, v in {**R.check_all("rope_partial_emu", {"y": y}, PR.fwd_ref(x, cs, pairing, dtype)),
                         **R.check_all("rope_partial_emu", {"dx": dx}, PR.bwd_ref(dy, cs, pairing, dtype))}.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert torch.equal(y[..., rot:], x[..., rot:]) and torch.equal(dx[..., rot:], dy[..., rot:])
    print(f"\nWORST emulation pairing={pairing} D={D} R={rot} {dtype}: {worst}")


def test_the_two_pairings_are_hf_formulas():
    """The float64 restatement equals HF's apply_rotary_pos_emb of Phi-3 (pairing 0) and GLM-4 (pairing 1), stated independently in
    tests/partial_rope_host.py, to float64 rounding."""
    import partial_rope_host as PH
    for pairing, D, rot in CASES:
        x, cs, _ = _inputs(5, 3, D, rot, torch.float32, 11)
        ref = PR.fwd_ref(x, cs, pairing, torch.float32)["y"][0]
        hf = PH.plain_partial(x.double(), cs.double(), bool(pairing))
        assert float((ref - hf).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairing,D,rot", [(0, 128, 96), (0, 64, 48), (1, 128, 64), (1, 64, 32)])
def test_deliberate_errors_fall_outside_the_bounds(pairing, D, rot, dtype):
    x, cs, dy = _inputs(37, 3, D, rot, dtype, 5)
    fwd, bwd = PR.fwd_ref(x, cs, pairing, dtype), PR.bwd_ref(dy, cs, pairing, dtype)
    R.check_all("rope_partial_emu", {"y": PR.emulate(x, cs, pairing)}, fwd)                    # the honest one passes
    wrong = {"the other pairing": PR.emulate(x, cs, 1 - pairing),
             "a rotated pass-through region": PR.emulate(x, cs, pairing, rotate_all=True)}
    for off in (-16, 16):                                                      # the same table values over a region 16 shorter / longer
        h = (rot + off) // 2
        c, s = cs[:, :rot // 2], cs[:, rot // 2:]
        if off > 0:
            c, s = torch.cat([c, c[:, :8]], -1), torch.cat([s, s[:, :8]], -1)
        wrong[f"R off by {off}"] = PR.emulate(x, torch.cat([c[:, :h], s[:, :h]], -1).contiguous(), pairing)
    for what, y in wrong.items():
        with pytest.raises(AssertionError, match="over the bound"):
            R.check_all("rope_partial_wrong", {"y": y}, fwd, what)
    with pytest.raises(AssertionError, match="over the bound"):
        R.check_all("rope_partial_wrong", {"dx": PR.emulate(dy, cs, pairing, 1.0)}, bwd, "the forward's sign of sin in the backward")
