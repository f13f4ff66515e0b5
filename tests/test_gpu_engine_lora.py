"""LoRA adapters through the engine on the GPU: UNMODIFIED transformers models with adapters (tests/test_lora_fixture.py: all seven
targets at r = 6 on Llama-3, r = 16 in bf16 on Mistral, q_proj + v_proj with ranks 8 and 4 on the biased Llama, Qwen3 with q/k-norm
and tied head, Mixtral with attention-only adapters), the protocol of tests/family.py:

* fp32, packed mode and the block-wise stack walk, against HF's own eager forward / backward in float64 on the card over the same
  wrapped model (the test-side RefLora): logprobs within 1e-4, loss within 1e-5, every adapter gradient within max(1e-4, 1.5 x
  control) and 1e-3, where the control is the worst ratio of the same engine on the merged model (plain trainable weights W + s B A, no
  adapters: the path the engine had before adapters) against HF in float64; and the adapters-off loss is not the reference's.
* bf16 against tests/golden/engine_lora.pt (logprobs 0.08 / 0.015, loss 1 %, REF_BF16_BOUND / REF_BF16_MEDIAN).
* the parameters with a gradient are exactly the adapters, every frozen .grad is None - packed, packed+recompute, stack.
* tree equals dense on the device; engine.forward equals the engine on the merged model; a trainable base AND adapters get both
  gradient sets; a frozen head forms no [V, hidden] product; two ranks sum to the single-process adapter gradients."""
import os
import sys

import numpy as np
import pytest
import torch

import family
import test_llama_family_fixture as fx
import test_lora_fixture as lx
from dynamictreeattn_amd import dense, lora, ops, synth
from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo
from test_gpu_engine import REF_BF16_BOUND, REF_BF16_MEDIAN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [("packed", 2048), ("stack", 16)]


def _seqs(case):
    return synth.as_tensors(lx.seqs_of(case))


def _against_hf64(mine, ref64, seqs, mode, monkeypatch):
    """family.fp32_against_hf64 with the wrapped float64 model as the reference -> (logprob error, loss, reference loss, {name:
    ratio} over the parameters HF gave a gradient); the engine gave exactly those a gradient, every frozen .grad is None."""
    return family.fp32_against_hf64(mine, seqs, family.att(len(seqs)), mode, monkeypatch, ref64=ref64)[:4]


def _merged_plain(case, attached):
    """The plain transformers model holding merged_state_dict(attached): every weight trainable, no adapters."""
    plain = lx.base_model(case)
    missing, unexpected = plain.load_state_dict(lora.merged_state_dict(attached), strict=False)
    assert not unexpected and all("rotary" in k or k == "lm_head.weight" for k in missing), (missing, unexpected)
    return plain.float().train()


@pytest.mark.parametrize("mode", ["packed", "stack"])
@pytest.mark.parametrize("case", list(lx.CASES))
def test_fp32_against_hf_eager_in_float64(case, mode, monkeypatch):
    pytest.importorskip("transformers")
    seqs = _seqs(case)
    mine = lx.base_model(case); lx.attach_product(case, mine)
    plain = _merged_plain(case, mine)
    ref = lx.wrap_ref(case, lx.base_model(case)).double().to(DEV).train()
    lp_err, loss, loss_r, ratios = _against_hf64(mine.to(DEV), ref, seqs, mode, monkeypatch)
    assert set(ratios) == set(lx.gold_grads(lx.gold(case)))                    # the adapter parameters, nothing else
    print(f"{case}/{mode}: logprob err {lp_err:.2e}, loss rel {abs(loss - loss_r) / abs(loss_r):.2e}, worst ratio "
          f"{max(ratios.items(), key=lambda kv: kv[1])}")
    assert lp_err < 1e-4
    assert abs(loss - loss_r) <= 1e-5 * abs(loss_r)
    assert abs(lx.gold(case)["bwd_dense_loss_off"] - loss_r) > 1e-5 * abs(loss_r)      # adapters off: another loss - not an inert case
    _, _, _, control = _against_hf64(plain, None, seqs, mode, monkeypatch)
    worst_c = max(control.values())
    bad = {n: r for n, r in ratios.items() if r > max(1e-4, 1.5 * worst_c)}
    print(f"{case}/{mode}: control worst {worst_c:.2e}; above the rule: {bad}")
    assert not bad, bad
    assert max(ratios.values()) <= 1e-3


def _bf16_model(case, trainable_base=False):
    m = lx.base_model(case).to(torch.bfloat16)
    lx.attach_product(case, m, adapter_dtype=lx.CASES[case][5])
    if trainable_base:
        for p in m.parameters():
            p.requires_grad_(True)
    return m.to(DEV).train()


def _bf16_backward(hf, seqs, mode, bs, monkeypatch, recompute=False):
    _, loss, e = family.run_engine(hf, seqs, family.att(len(seqs)), torch.bfloat16, mode, bs, monkeypatch, forward=False,
                                   **({"checkpoint_layers": True} if recompute else {}))
    return loss, e.last_mode


@pytest.mark.parametrize("mode,bs", MODES)
@pytest.mark.parametrize("case", list(lx.CASES))
def test_bf16_against_the_reference_fixture(case, mode, bs, monkeypatch):
    pytest.importorskip("transformers")
    g = lx.gold(case)
    named = family.check_bf16_against_fixture(_bf16_model(case), _seqs(case), g, mode, bs, monkeypatch, label=case)
    assert all(named[n].grad.dtype == named[n].dtype == lx.CASES[case][5] for n in lx.gold_grads(g))


@pytest.mark.parametrize("mode", ["packed", "packed+recompute", "stack"])
@pytest.mark.parametrize("case", list(lx.CASES))
def test_only_the_adapters_get_gradients(case, mode, monkeypatch):
    pytest.importorskip("transformers")
    hf = _bf16_model(case)
    adapters = {n for n, p in hf.named_parameters() if p.requires_grad}
    assert adapters == set(lx.gold_grads(lx.gold(case)))
    loss, last = _bf16_backward(hf, _seqs(case), mode.split("+")[0], 16 if mode == "stack" else 2048, monkeypatch, recompute="recompute" in mode)
    assert last.startswith(mode), last
    got = {n for n, p in hf.named_parameters() if p.grad is not None}
    assert got == adapters, (sorted(got - adapters)[:4], sorted(adapters - got)[:4])
    assert all(p.grad is None for n, p in hf.named_parameters() if n not in adapters)            # frozen: None, not zeros
    gold_grads = lx.gold_grads(lx.gold(case))
    named = dict(hf.named_parameters())
    ratios = {n: mo.grad_ratio(gold_grads[n], named[n].grad.float().cpu()) for n in gold_grads}
    assert abs(loss - lx.gold(case)["bwd_dense_loss"]) < 1e-2 * abs(loss)
    assert max(ratios.values()) <= REF_BF16_BOUND and float(np.median(list(ratios.values()))) <= REF_BF16_MEDIAN


def test_tree_equals_dense_on_the_device():
    """dense.backward (one pass per sequence, the stack form) against engine.backward (one packed pass), fp32, all seven targets."""
    pytest.importorskip("transformers")
    case = "llama3_all7"
    seqs = _seqs(case)
    a = lx.base_model(case); lx.attach_product(case, a); a = a.to(DEV)
    b = lx.base_model(case); lx.attach_product(case, b); b = b.to(DEV)
    ratios = family.check_tree_equals_dense(a, b, seqs, forward=False)
    assert len(ratios) == 42 and all(p.grad is None for p in a.parameters() if not p.requires_grad)
    fwd_d = dense.forward(a, seqs)                                            # dense.py sees the adapters too
    for x, y in zip(fwd_d, lx.gold(case)["fwd_dense"]):
        assert float((x.cpu() - y).abs().max()) < 1e-4


@pytest.mark.parametrize("case", ["llama3_bias_qv", "qwen3_tied"])
def test_forward_equals_the_engine_on_the_merged_model(case):
    pytest.importorskip("transformers")
    seqs = _seqs(case)
    mine = lx.base_model(case); lx.attach_product(case, mine)
    plain = _merged_plain(case, mine).to(DEV)
    mine = mine.to(DEV)
    outs = []
    for m in (mine, plain):
        t = TokenTrie(seqs); t.forward_permute()
        outs.append(TreeTrainingEngine(m.config, DEV, torch.float32, max(map(len, seqs)), forward_only=True).forward(m, t))
    err = max(float((a - b).abs().max()) for a, b in zip(*outs))
    off = max(float((a.cpu() - b).abs().max()) for a, b in zip(outs[0], lx.gold(case)["fwd_dense_off"]))
    print(f"{case}: adapters vs merged {err:.2e}; vs adapters off {off:.3f}")
    assert err < 1e-4 and off >= lx.MIN_GAP


def test_trainable_base_and_adapters_get_both_gradient_sets(monkeypatch):
    pytest.importorskip("transformers")
    case = "llama3_bias_qv"                       # a group where only some members carry an adapter, over a base with biases
    seqs = _seqs(case)
    mine = lx.base_model(case); lx.attach_product(case, mine)
    ref = lx.wrap_ref(case, lx.base_model(case))
    for m in (mine, ref):
        for p in m.parameters():
            p.requires_grad_(True)
    lp_err, loss, loss_r, ratios = _against_hf64(mine.to(DEV), ref.double().to(DEV).train(), seqs, "packed", monkeypatch)
    assert set(ratios) == set(dict(mine.named_parameters())) and len(ratios) > 12
    assert lp_err < 1e-4 and abs(loss - loss_r) <= 1e-5 * abs(loss_r) and max(ratios.values()) <= 1e-3, max(ratios.items(), key=lambda kv: kv[1])
    hf = _bf16_model(case, trainable_base=True)   # bf16: the HIP adapter kernels beside the base weight-gradient GEMMs
    loss16, _ = _bf16_backward(hf, seqs, "packed", 2048, monkeypatch)
    named = dict(hf.named_parameters())
    assert all(p.grad is not None for p in named.values())
    gold_grads = lx.gold_grads(lx.gold(case))     # the adapter gradients do not depend on whether the base trains
    r16 = {n: mo.grad_ratio(gold_grads[n], named[n].grad.float().cpu()) for n in gold_grads}
    assert abs(loss16 - loss_r) < 1e-2 * abs(loss_r) and max(r16.values()) <= REF_BF16_BOUND
    ref_named = dict(ref.named_parameters())
    rb = {n: mo.grad_ratio(ref_named[n].grad.float().cpu(), p.grad.float().cpu()) for n, p in named.items() if n not in gold_grads}
    assert max(rb.values()) <= REF_BF16_BOUND, max(rb.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("keep", [True, False], ids=["kept", "chunked"])
def test_frozen_head_forms_no_vocab_by_hidden_product(keep, monkeypatch):
    """ops.lm_head_rows with a head weight that needs no gradient: no [V, hidden] result of torch.mm / addmm during backward (the weight
    gradient GEMM and its buffer are skipped); with a trainable head there is at least one.  dh is the same either way."""
    T, V, H = 300, 512, 64
    g = torch.Generator(device=DEV).manual_seed(3)
    h0 = torch.randn((T, H), generator=g, device=DEV).to(torch.bfloat16)
    W0 = (0.1 * torch.randn((V, H), generator=g, device=DEV)).to(torch.bfloat16)
    nxt = torch.randint(0, V, (T,), generator=g, device=DEV)
    empty = torch.zeros(0, dtype=torch.long, device=DEV)
    seen = []
    real_mm, real_addmm = torch.mm, torch.addmm

    def counted(fn):
        def wrapper(*a, **k):
            out = fn(*a, **k)
            seen.append(tuple(out.shape))
            return out
        return wrapper
    results = {}
    for trainable in (False, True):
        h, W = h0.clone().requires_grad_(True), W0.clone().requires_grad_(trainable)
        lp, _, ent = ops.lm_head_rows(h, W, nxt, None, empty, empty, [0] * 8, True, 128, keep_bytes=(1 << 40) if keep else 0)
        seen.clear()
        monkeypatch.setattr(torch, "mm", counted(real_mm)); monkeypatch.setattr(torch, "addmm", counted(real_addmm))
        (lp.sum() + 0.1 * ent.sum()).backward()
        monkeypatch.setattr(torch, "mm", real_mm); monkeypatch.setattr(torch, "addmm", real_addmm)
        n_vh = sum(1 for s in seen if s == (V, H))
        assert len(seen) > 0 and (n_vh >= 1 if trainable else n_vh == 0), (trainable, seen)
        assert (W.grad is not None) == trainable
        results[trainable] = h.grad.clone()
    assert torch.equal(results[False], results[True])


# ---------------------------------------------------------------------------------------------------------------- two ranks
def _dp_worker(rank, world, port, outdir):
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
    import torch.distributed as dist
    from dynamictreeattn_amd import dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    case = "llama3_all7"
    model = _bf16_model(case)
    seqs = _seqs(case); att = fx.att(len(seqs))
    red = dp.GradReducer(model.parameters(), bucket_bytes=4000)
    n_adapter = sum(1 for p in model.parameters() if p.requires_grad)
    assert len(red.buckets) > 3 and sum(len(b) for b in red.buckets) == n_adapter                # the buckets hold the adapters only
    ids = dp.my_bin(seqs, rank, world, "backward", 2048)
    t = TokenTrie([seqs[i] for i in ids], [att[i] for i in ids], device=torch.device(DEV))
    if ids:
        t.backward_permute()
    red.zero_grad(); red.start()
    loss = TreeTrainingEngine(model.config, DEV, torch.bfloat16, 256).backward(model, t, mo.default_loss, 2048)
    red.finish()
    torch.cuda.synchronize()
    lt = torch.tensor([loss], dtype=torch.float64, device=DEV); dist.all_reduce(lt)
    torch.save({"loss": float(lt), "ids": sorted(ids),
                "grads": {n: p.grad.float().cpu() for n, p in model.named_parameters() if p.grad is not None}}, os.path.join(outdir, f"rank{rank}.pt"))
    red.close()
    dist.destroy_process_group()


def test_two_ranks_sum_to_the_single_process_adapter_gradients(tmp_path, monkeypatch):
    pytest.importorskip("transformers")
    import test_gpu_multirank as mr
    mr._run(_dp_worker, 2, (mr._free_port(), str(tmp_path)))
    res = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"), weights_only=True) for r in range(2)]
    case = "llama3_all7"
    hf = _bf16_model(case)
    seqs = _seqs(case)
    loss, _ = _bf16_backward(hf, seqs, "packed", 2048, monkeypatch)
    full = {n: p.grad.float().cpu() for n, p in hf.named_parameters() if p.grad is not None}
    assert sorted(res[0]["ids"] + res[1]["ids"]) == list(range(len(seqs))) and res[0]["ids"] and res[1]["ids"]
    assert abs(res[0]["loss"] - loss) < 1e-2 * abs(loss)
    for r in res:
        assert set(r["grads"]) == set(full) == set(lx.gold_grads(lx.gold(case)))
        worst = max(mo.grad_ratio(full[n], r["grads"][n]) for n in full)
        assert worst <= REF_BF16_BOUND, worst
    assert all(torch.equal(res[0]["grads"][n], res[1]["grads"][n]) for n in full)                # both ranks hold the same sums
