"""Sliding-window tree attention, host side: the per-token lower key bound win_lo (packing.window_lo_host) against a brute-force
ancestor walk, the windowed query-tile run plan (packing.plan_qtile_runs_window) and dK/dV query ends against the visibility rule
depth[t] - depth[s] < W over ancestors, and the per-layer windows read from Qwen2 / Qwen3 configurations (model._windows_of)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import hostmirror
from dynamictreeattn_amd import model as M
from dynamictreeattn_amd import packing

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
WINDOWS = [1, 2, 63, 64, 65, 130, 10 ** 6]


def _plans():
    cases = json.load(open(os.path.join(GOLDEN, "trie_cases.json")))["cases"]
    out = []
    for c in cases:
        lens, lcp = c["ref"].get("lens"), c["ref"].get("lcp_lens")
        if lens is None:
            continue
        out.append(packing.plan_segments(lens, lcp))
    rng = np.random.default_rng(5)
    for n in range(12):                                   # random tries: sorted random sequences over a small alphabet
        seqs = sorted(tuple(rng.integers(0, 3, size=int(rng.integers(1, 400)))) for _ in range(int(rng.integers(1, 9))))
        lens = [len(s) for s in seqs]
        lcp = []
        for a, b in zip(seqs, seqs[1:]):
            k = 0
            while k < min(len(a), len(b)) and a[k] == b[k]:
                k += 1
            lcp.append(k)
        out.append(packing.plan_segments(lens, lcp))
    out.append(packing.pad_plan(out[-1], 256))
    return out


PLANS = _plans()


def _brute(plan, W):
    _, depth, parent, se = hostmirror.expand_plan_host(plan)
    a = np.maximum(depth.astype(np.int64) - W + 1, 0)
    wl = np.arange(plan.T, dtype=np.int64)
    live = np.flatnonzero(depth[wl] > a)
    while live.size:                                      # every token steps to its parent until it reaches the target depth
        wl[live] = parent[wl[live]]
        live = live[depth[wl[live]] > a[live]]
    return depth, se, wl


def _visible(depth, se, W):
    T = depth.shape[0]
    s = np.arange(T)
    t = s[:, None]
    return (s[None, :] <= t) & (t < se[None, :]) & ((depth[:, None] - depth[None, :]) < W)      # [t, s]


def test_plans_were_read():
    assert len(PLANS) >= 10 and any(p.T > 300 for p in PLANS)


@pytest.mark.parametrize("W", WINDOWS)
def test_window_lo_matches_ancestor_walk(W):
    for plan in PLANS:
        if plan.T == 0:
            continue
        _, _, wl = _brute(plan, W)
        np.testing.assert_array_equal(packing.window_lo_host(plan, W), wl)


@pytest.mark.parametrize("W", WINDOWS)
def test_windowed_runs_cover_exactly_what_is_visible(W):
    for plan in PLANS:
        if plan.T == 0 or plan.T > 1500:
            continue
        depth, se, wl = _brute(plan, W)
        vis = _visible(depth, se, W)
        # the window rule equals the win_lo bound over ancestors
        anc = (np.arange(plan.T)[None, :] <= np.arange(plan.T)[:, None]) & (np.arange(plan.T)[:, None] < se[None, :])
        np.testing.assert_array_equal(vis, anc & (np.arange(plan.T)[None, :] >= wl[:, None]))
        rp, runs = packing.plan_qtile_runs_window(plan, wl.astype(np.int32))
        nqt = (plan.T + packing.QTILE - 1) // packing.QTILE
        assert rp.shape[0] == nqt + 1
        for qt in range(nqt):
            q0, q1 = qt * packing.QTILE, min(plan.T, (qt + 1) * packing.QTILE)
            listed = np.zeros(plan.T, bool)
            for b, e, m, _ in runs[rp[qt]:rp[qt + 1]]:
                assert b < e
                listed[b:e] = True
                if m == 0:                                # maskless: every key visible to every row of the tile
                    assert vis[q0:q1, b:e].all(), (W, qt, b, e)
            need = vis[q0:q1].any(0)
            assert not (need & ~listed).any(), (W, qt)    # every visible pair covered
            # nothing below the lowest window bound of the tile is listed: no key tile outside every row's window
            lo_min = int(wl[q0:q1].min())
            assert not listed[:lo_min].any()
            # a listed key is an ancestor inside the window of at least one row, up to the diagonal block's own rows
            anc_any = (anc[q0:q1] & (np.arange(plan.T)[None, :] >= wl[q0:q1, None])).any(0)
            assert not (listed[:q0] & ~anc_any[:q0] & ~anc[q0:q1, :q0].any(0)).any(), (W, qt)


def test_windowed_runs_drop_out_of_window_key_tiles():
    """A deep chain: a query tile visits O(W) keys, not its whole root path."""
    plan = packing.plan_segments([4096], [])
    W = 200
    wl = packing.window_lo_host(plan, W)
    rp, runs = packing.plan_qtile_runs_window(plan, wl)
    for qt in range(plan.T // packing.QTILE):
        keys = sum(int(e - b) for b, e, _, _ in runs[rp[qt]:rp[qt + 1]])
        assert keys <= W + packing.QTILE
    rp0, runs0 = packing.plan_qtile_runs(plan)
    assert sum(int(e - b) for b, e, _, _ in runs) * 5 < sum(int(e - b) for b, e, _, _ in runs0)


def test_wide_window_plan_equals_unwindowed_plan():
    for plan in PLANS:
        if plan.T == 0:
            continue
        W = packing.max_depth(plan) + 1
        wl = packing.window_lo_host(plan, W)
        rp, runs = packing.plan_qtile_runs_window(plan, wl)
        rp0, runs0 = packing.plan_qtile_runs(plan)
        np.testing.assert_array_equal(rp, rp0)
        np.testing.assert_array_equal(runs, runs0)
        kq = packing.ktile_qend_host(plan)
        np.testing.assert_array_equal(packing.ktile_qend_window(kq, wl), kq)


@pytest.mark.parametrize("W", WINDOWS)
def test_windowed_ktile_qend_bounds_every_visible_row(W):
    for plan in PLANS:
        if plan.T == 0 or plan.T > 1500:
            continue
        depth, se, wl = _brute(plan, W)
        vis = _visible(depth, se, W)
        kq = packing.ktile_qend_window(packing.ktile_qend_host(plan), wl)
        assert (kq <= packing.ktile_qend_host(plan)).all()
        for j in range(kq.shape[0]):
            k0, k1 = j * packing.KTILE, min(plan.T, (j + 1) * packing.KTILE)
            rows = np.flatnonzero(vis[:, k0:k1].any(1))
            if rows.size:
                assert rows.max() < kq[j]
        units, splits, _ = packing.plan_dkv_units(kq, plan.T, plan.T, 0, 2, min_tiles=1)
        assert units.shape[1] == 4


def test_window_lo_rejects_no_window():
    with pytest.raises(ValueError):
        packing.window_lo_host(PLANS[0], 0)


# ------------------------------------------------------------------------------------------------ configurations
def _model(**cfg):
    return SimpleNamespace(config=SimpleNamespace(**cfg))


def test_windows_from_use_sliding_window_rule():
    m = _model(num_hidden_layers=4, use_sliding_window=True, max_window_layers=1, sliding_window=24)
    assert M._windows_of(m) == [0, 24, 24, 24]
    m = _model(num_hidden_layers=3, use_sliding_window=False, max_window_layers=1, sliding_window=24)
    assert M._windows_of(m) == [0, 0, 0]
    assert M._windows_of(_model(num_hidden_layers=2)) == [0, 0]


def test_windows_from_layer_types():
    m = _model(num_hidden_layers=3, layer_types=["sliding_attention", "full_attention", "sliding_attention"], sliding_window=7)
    assert M._windows_of(m) == [7, 0, 7]
    with pytest.raises(ValueError):
        M._windows_of(_model(num_hidden_layers=2, layer_types=["chunked_attention", "full_attention"], sliding_window=7))
    # HF: a sliding layer whose config has no sliding_window attends in full
    assert M._windows_of(_model(num_hidden_layers=1, layer_types=["sliding_attention"], sliding_window=None)) == [0]


def test_windows_from_hf_configs():
    tr = pytest.importorskip("transformers")
    c2 = tr.Qwen2Config(num_hidden_layers=3, use_sliding_window=True, max_window_layers=1, sliding_window=24,
                        hidden_size=64, intermediate_size=64, num_attention_heads=2, num_key_value_heads=1, vocab_size=32)
    assert M._windows_of(SimpleNamespace(config=c2)) == [0, 24, 24]
    c3 = tr.Qwen3Config(num_hidden_layers=2, use_sliding_window=True, layer_types=["full_attention", "sliding_attention"], sliding_window=16,
                        hidden_size=64, intermediate_size=64, num_attention_heads=2, num_key_value_heads=1, head_dim=64, vocab_size=32)
    assert M._windows_of(SimpleNamespace(config=c3)) == [0, 16]
    m = M.Qwen3TreeLM(M.make_config(dict(vocab_size=32, hidden_size=64, intermediate_size=64, num_hidden_layers=2,
                                         num_attention_heads=2, num_key_value_heads=1, head_dim=64,
                                         use_sliding_window=True, max_window_layers=1, sliding_window=5)))
    assert M._windows_of(m) == [0, 5]


def test_layer_metas_refuse_a_packed_meta_without_windowed_form():
    from dynamictreeattn_amd import ops
    packed = ops.TreeAttnMeta(T=4, subtree_end=object(), run_ptr=None, runs=None, ktile_qend=None)
    with pytest.raises(ValueError):
        M.layer_metas(packed, [0, 8])
    built = []
    metas = M.layer_metas(packed, [0, 8, 8, 3], lambda W: built.append(W) or W)
    assert metas == [packed, 8, 8, 3] and built == [8, 3]          # once per distinct window
    st = M.layer_metas(ops.stack_meta(5), [0, 9])
    assert st[0].window == 0 and st[1].window == 9 and st[1].q_offset == 5
