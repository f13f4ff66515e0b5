"""The protocol every model family's tests share: the small fixture helpers, HF's own dense run, the engine runner, and the four
checks - the engine on the CPU stand-ins against the fixture, bf16 against the fixture, tree equals dense, and recomputation with kept
attention outputs.  The family files (test_*_fixture.py, test_gpu_engine_*.py) hold the configurations, weights, control models and
every assertion that is their own; a bound that differs between families is an argument here, never a default that hides it."""
import numpy as np
import torch

from dynamictreeattn_amd.token_trie import TokenTrie
from dynamictreeattn_amd.tree_training_engine import TreeTrainingEngine
from oracle import model_oracle as mo

DEV = "cuda:0"
CPU = torch.device("cpu")


def att(n):
    return [{"w_logprobs": -1.0 - 0.01 * i, "w_entropy": 0.1 + 0.003 * i} for i in range(n)]


def gold_grads(g, key="bwd_dense_grads_fp16_scaled"):
    return {n: q.float() * s_ for n, (q, s_) in g[key].items()}


def load_weights(model, w):
    """Copies the weights dict `w` (by parameter name) into `model`; -> the model in fp32, train mode."""
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(w[n])
    return model.float().train()


def _m(c):
    return type("M", (), {"config": c})()


def hf_dense(model, seqs, att, device=DEV):
    """HF's own eager forward / backward per sequence (the reference's dense.py arithmetic: logprobs[:len-1], entropy[:len] - at the
    fixtures' weight scale the entropy varies along a sequence, so its last row counts): logprobs, loss sum; grads in .grad."""
    lps, total = [], 0.0
    for s, a in zip(seqs, att):
        ids = s.to(device)[None]
        logits = model(input_ids=ids, use_cache=False).logits[0]
        lsm = torch.log_softmax(logits if logits.dtype == torch.float64 else logits.float(), -1)
        lp, ent = lsm[:-1].gather(-1, ids[0, 1:, None])[:, 0], -(lsm.exp() * lsm).sum(-1)
        loss = mo.default_loss(lp, ent, a)
        loss.backward()
        total += float(loss.detach())
        lps.append(lp.detach().float().cpu())
    return lps, total


def run_engine(model, seqs, att, dtype, mode, bs, monkeypatch, device=DEV, forward=True, recompute=None, full_layers=0, **engine_attrs):
    """-> (per-sequence logprobs on the host or None, loss, engine) of the engine on `model`; gradients in .grad.  mode None: the
    engine's own choice; stack: blocks of `bs` rows; recompute (a kept fraction of the attention outputs): every layer but the first
    `full_layers` is recomputed in the backward; engine_attrs: attributes set on the backward engine."""
    maxlen = max(map(len, seqs))
    out = None
    if forward:
        t = TokenTrie(seqs, device=torch.device(device)); t.forward_permute()
        out = [o.cpu() for o in TreeTrainingEngine(model.config, device, dtype, maxlen, forward_only=True).forward(model, t)]
    t = TokenTrie(seqs, att, device=torch.device(device)); t.backward_permute()
    e = TreeTrainingEngine(model.config, device, dtype, maxlen)
    if mode is not None:
        e.mode = mode
    for k, v in engine_attrs.items():
        setattr(e, k, v)
    if recompute is not None:
        e.attn_keep_fraction = recompute
        monkeypatch.setattr(e, "_should_checkpoint", lambda model, T: True)
        monkeypatch.setattr(e, "_full_layers", lambda model, T, f=full_layers: f)
    if mode == "stack":
        monkeypatch.setattr(e, "_stack_block_rows", lambda *a, b=bs: b)
    loss = e.backward(model, t, mo.default_loss, bs)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return out, loss, e


def fp32_against_hf64(model32, seqs, att, mode, monkeypatch, ref64=None):
    """The engine in fp32 on `model32` against HF eager in float64 (`ref64`, or a float64 copy of the same class on the same state
    dict), both on the card, stack blocks of 16 rows: (logprob error, loss, reference loss, {name: gradient ratio}, (the names the
    engine gave a gradient, the reference's trainable names)).  The two name sets are equal (asserted here: no frozen parameter has a
    gradient, every trainable one has), and the engine ran in `mode`."""
    if ref64 is None:
        ref64 = type(model32)(model32.config).double().to(DEV).train()
        ref64.load_state_dict({k: v.double() for k, v in model32.state_dict().items()})
    mine = model32.to(DEV)
    lps, loss_r = hf_dense(ref64, seqs, att)
    out, loss, e = run_engine(mine, seqs, att, torch.float32, mode, 16, monkeypatch)
    assert e.last_mode.startswith(mode), e.last_mode
    lp_err = max(float((a - b).abs().max()) for a, b in zip(out, lps))
    rg = {n: p.grad for n, p in ref64.named_parameters() if p.requires_grad}
    named = dict(mine.named_parameters())
    got = {n for n, p in named.items() if p.grad is not None}
    assert got == set(rg), (sorted(got - set(rg))[:4], sorted(set(rg) - got)[:4])
    return lp_err, loss, loss_r, {n: mo.grad_ratio(g.float(), named[n].grad) for n, g in rg.items()}, (got, set(rg))


# ---------------------------------------------------------------------------------------------------------------- the four checks
def check_cpu_engine_matches_fixture(hf, seqs, g, monkeypatch, fwd_key="fwd_dense", loss_key="bwd_dense_loss",
                                     grads_key="bwd_dense_grads_fp16_scaled", mode="packed", atol=1e-4, loss_rtol=1e-4, norm_rtol=None):
    """The product engine with its device steps replaced by the CPU stand-ins of tests/hostmirror.py (fp32) reproduces the fixture:
    forward logprobs within `atol`, loss within `loss_rtol`, the parameters with a gradient are exactly the fixture's, every gradient
    ratio <= 1e-3 (fp16-packed golden: 5e-4 per element) and, with `norm_rtol`, every gradient norm within it."""
    import hostmirror
    hostmirror.install(monkeypatch)
    out, loss, _ = run_engine(hf, seqs, att(len(seqs)), torch.float32, mode, 2048, monkeypatch, device=CPU)
    for a, b in zip(out, g[fwd_key]):
        assert torch.allclose(a, b, atol=atol), float((a - b).abs().max())
    assert abs(loss - g[loss_key]) < loss_rtol * abs(loss)
    named = dict(hf.named_parameters())
    grads = gold_grads(g, grads_key)
    assert {n for n, p in named.items() if p.grad is not None} == set(grads)
    for n, gg in grads.items():
        assert mo.grad_ratio(gg, named[n].grad) <= 1e-3, n
        if norm_rtol is not None:
            assert abs(float(named[n].grad.norm()) - g["grad_norms"][n]) <= norm_rtol * g["grad_norms"][n] + 1e-9, n
    return named


def check_bf16_against_fixture(hf, seqs, g, mode, bs, monkeypatch, label=""):
    """bf16 on the card against the fixture the reference computed: logprobs 0.08 max / 0.015 mean over all positions, loss 1 %, the
    parameters with a gradient are exactly the fixture's, REF_BF16_BOUND / REF_BF16_MEDIAN on the gradient ratios; -> the parameters."""
    from test_gpu_engine import REF_BF16_BOUND, REF_BF16_MEDIAN
    grads = gold_grads(g)
    out, loss, e = run_engine(hf, seqs, att(len(seqs)), torch.bfloat16, mode, bs, monkeypatch)
    assert e.last_mode.startswith(mode), e.last_mode
    err = torch.cat([(a - b).abs() for a, b in zip(out, g["fwd_dense"])])
    named = dict(hf.named_parameters())
    assert {n for n, p in named.items() if p.grad is not None} == set(grads)
    ratios = {n: mo.grad_ratio(grads[n], named[n].grad.float().cpu()) for n in grads}
    print(f"{label}/{mode}: logprob err max {float(err.max()):.4f} mean {float(err.mean()):.4f}, loss rel "
          f"{abs(loss - g['bwd_dense_loss']) / abs(loss):.2e}, ratio max {max(ratios.values()):.4f} median {float(np.median(list(ratios.values()))):.4f}")
    assert float(err.max()) < 0.08 and float(err.mean()) < 0.015
    assert abs(loss - g["bwd_dense_loss"]) < 1e-2 * abs(loss)
    assert max(ratios.values()) <= REF_BF16_BOUND, max(ratios.items(), key=lambda kv: kv[1])
    assert float(np.median(list(ratios.values()))) <= REF_BF16_MEDIAN
    return named


def check_tree_equals_dense(a, b, seqs, forward=True):
    """dense.backward on `a` (one pass per sequence, the stack form) against engine.backward on `b` (one packed pass), two copies of
    one model on the card in fp32: loss within 1e-5, every trainable parameter's gradient ratio <= 1e-4 and, with `forward`, the dense
    forward within 1e-4 of the packed forward; -> the ratios."""
    from dynamictreeattn_amd import dense
    loss_d = dense.backward(a, seqs, att(len(seqs)), mo.default_loss)
    _, loss_t, _ = run_engine(b, seqs, att(len(seqs)), torch.float32, "packed", 2048, None, forward=False)
    assert abs(loss_t - loss_d) <= 1e-5 * abs(loss_d)
    gd = dict(a.named_parameters())
    ratios = {n: mo.grad_ratio(gd[n].grad, p.grad) for n, p in b.named_parameters() if p.requires_grad}
    assert max(ratios.values()) <= 1e-4, max(ratios.items(), key=lambda kv: kv[1])
    if forward:
        fwd = dense.forward(b, seqs)
        t = TokenTrie(seqs); t.forward_permute()
        out = TreeTrainingEngine(b.config, DEV, torch.float32, max(map(len, seqs)), forward_only=True).forward(b, t)
        assert max(float((x - y).abs().max()) for x, y in zip(fwd, out)) < 1e-4
    return ratios


def check_recompute_is_bitwise(hf, seqs, monkeypatch):
    """checkpoint_layers = True: every layer is recomputed in the backward; with kept attention outputs the recomputation replays them
    (the forward attention kernel runs once per layer, L launches; without them 2 L) - loss and gradients are those of the plain
    packed pass, bit for bit."""
    from dynamictreeattn_amd import ops
    L = hf.config.num_hidden_layers
    ref = None
    for ckpt, frac, launches in ((False, 0.25, L), (True, 0.25, L), (True, 0.0, 2 * L)):
        hf.zero_grad(set_to_none=True)
        tm = ops.KernelTimer(); ops.KernelTimer.active = tm
        try:
            _, loss, e = run_engine(hf, seqs, att(len(seqs)), torch.bfloat16, "packed", 2048, monkeypatch, forward=False,
                                    checkpoint_layers=ckpt, attn_keep_fraction=frac)
        finally:
            ops.KernelTimer.active = None
        assert tm.totals_ms()["fwd"][1] == launches, (ckpt, frac, tm.totals_ms()["fwd"][1])
        g = {n: p.grad.clone() for n, p in hf.named_parameters()}
        if ref is None:
            ref = (loss, g)
        else:
            assert loss == ref[0] and all(torch.equal(g[n], ref[1][n]) for n in g), (ckpt, frac)
