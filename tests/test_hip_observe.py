"""TIGE.observe on the GPU: a model that starts from a graph over the first 37 events and the first 38 edge-table rows and
is fed the rest of the stream through `observe` against a twin with equal weights that had the full graph and the full
table from the start and streams the same batches with `stream_step`.  Everything is compared bit for bit: embeddings,
state, recommendations.  On build() of tests/test_hip_rank.py (d = 16, K = 10, E = 200)."""
import numpy as np
import pytest
import torch

from test_hip_rank import assert_same_state, batch, build, dev, state_of

pytestmark = pytest.mark.gpu

E0 = 37
BATCHES = [(37, 101), (101, 102), (102, 200)]   # ragged: 64 events, one event, 98 events


def install_seq_restarter(model):
    from www2023tiger_amd.model.restarters import SeqRestarter
    torch.manual_seed(123)
    rst = SeqRestarter(raw_feat_getter=model.raw_feat_getter, graph=model.graph, hist_len=7, n_head=2, dropout=0.0).to(dev())
    rst.eval()
    rst.model_struct_fn, rst.rng_fn = model.model_struct, model.dropout_rng
    model.restarter_fn = rst


def twins(*, strategy='recent_edges', L=1, forms=(), seq=False):
    """A: the full graph and table.  B: the graph over the first E0 events, the first E0 + 1 table rows.  Equal weights
    (build() seeds every initialiser); both have streamed events [0, E0)."""
    from www2023tiger_amd.data.graph import Graph
    A, _, st = build(16, 16, 10, L=L, strategy=strategy)
    B, _, _ = build(16, 16, 10, L=L, strategy=strategy)
    for (ka, va), (kb, vb) in zip(A.state_dict().items(), B.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    B.graph = Graph.from_arrays(*(st[k][:E0] for k in ('src', 'dst', 'ts', 'eids')), strategy=strategy, seed=0,
                                max_node_id=st['n_nodes'] - 1, device=dev())
    B.raw_feat_getter.efeats = B.raw_feat_getter.efeats[:E0 + 1].clone()
    B.invalidate_struct()
    for m in (A, B):
        if seq:
            install_seq_restarter(m)
        if 'fused' in forms:
            m.fuse_attention()
        if 'eager' in forms:
            m.eager_updates()
        m.stream_step(*batch(st, 0, E0))
    assert_same_state(state_of(A), state_of(B))
    return A, B, st


def feed(A, B, st, lo, hi, **kw):
    src, dst, neg, ts, eids = batch(st, lo, hi)
    a = A.stream_step(src, dst, neg, ts, eids)
    ha = a.h[:2 * (hi - lo)].clone()
    b = B.observe(src, dst, ts, eids, efeats=st['efeats'][lo + 1:hi + 1], neg=neg, **kw)
    assert torch.equal(b.h[:2 * (hi - lo)], ha), f'h of batch [{lo}, {hi})'
    assert_same_state(state_of(A), state_of(B))
    return a, b


@pytest.mark.parametrize('variant', ['plain', 'recent_nodes', 'two-layers', 'fused+eager'])
def test_observing_the_stream_equals_having_had_the_full_graph(variant):
    kw = {'plain': {}, 'recent_nodes': dict(strategy='recent_nodes'), 'two-layers': dict(L=2),
          'fused+eager': dict(forms=('fused', 'eager'))}[variant]
    A, B, st = twins(**kw)
    g0, table0 = B.graph, B.raw_feat_getter.efeats
    for lo, hi in BATCHES:
        parent = B.graph
        feed(A, B, st, lo, hi)
        assert B.graph is not parent and B.restarter_fn.graph is B.graph
        assert B.graph.tcsr.num_entry == 2 * hi and parent.tcsr.num_entry == 2 * lo   # the parent is what it was
    assert g0.tcsr.num_entry == 2 * E0 and table0.shape[0] == E0 + 1
    fg = B.raw_feat_getter
    assert fg.efeats.shape[0] == 201 and torch.equal(fg.efeats, A.raw_feat_getter.efeats)
    assert fg.efeats.data_ptr() == fg._ef_store.data_ptr()   # a leading view of its backing storage
    for a, b in zip(B.graph._tensors(), A.graph._tensors()):
        assert torch.equal(a, b)


def test_the_sequence_restarter_reads_its_histories_from_the_extended_graph():
    A, B, st = twins(seq=True)
    for lo, hi in BATCHES:
        feed(A, B, st, lo, hi)
        nodes = torch.unique(torch.from_numpy(np.concatenate([st['src'][lo:hi], st['dst'][lo:hi]]))).to(dev())
        t = torch.full((nodes.numel(),), float(st['ts'][hi - 1]), device=dev())
        A.restart(nodes, t)
        B.restart(nodes, t)
        assert_same_state(state_of(A), state_of(B))
    # and the histories did come from the new edges: the stale graph gives other rows
    stale = B.restarter_fn.graph
    B.restarter_fn.graph = twins_graph_prefix(st)
    h_stale = B.restarter_fn(nodes, t)[0]
    B.restarter_fn.graph = stale
    assert not torch.equal(h_stale, B.restarter_fn(nodes, t)[0])


def twins_graph_prefix(st):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*(st[k][:E0] for k in ('src', 'dst', 'ts', 'eids')), strategy='recent_edges', seed=0,
                             max_node_id=st['n_nodes'] - 1, device=dev())


def test_recommend_sees_the_new_edges_after_observe_and_not_before():
    A, B, st = twins()
    lo, hi = BATCHES[0]
    q = torch.from_numpy(st['src'][hi:hi + 40]).to(dev())
    t = torch.full((40,), float(st['ts'][hi]), dtype=torch.float64, device=dev())   # A's later events are not before t
    cand = torch.arange(61, 76, device=dev())   # the items
    g_before = B.graph
    before = B.recommend(q, t, cand, 5, exclude_seen=True)
    feed(A, B, st, lo, hi)
    want = A.recommend(q, t, cand, 5, exclude_seen=True)
    got = B.recommend(q, t, cand, 5, exclude_seen=True)
    for a, b, nm in zip(got, want, ('ids', 'scores', 'n_valid')):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), nm
    assert not torch.equal(before[0], got[0])   # the call before observe: another state and another graph
    # the graph alone: the same state on the parent graph, which is still valid, excludes fewer items and ranks otherwise
    stale = B.recommend(q, t, cand, 5, exclude_seen=True, graph=g_before)
    assert bool((stale[0] != got[0]).any(1).any())
    assert int(stale[2].sum()) > int(got[2].sum())
    sa = A.rank_scores(q, q, t, cand)
    sb = B.rank_scores(q, q, t, cand)
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32))


def test_observe_defaults_and_device_inputs():
    """neg defaults to dst; device tensors give what host arrays give; want_prev is handed on"""
    A, B, st = twins()
    lo, hi = BATCHES[0]
    src, dst, _, ts, eids = batch(st, lo, hi)
    a = A.stream_step(src, dst, dst, ts, eids, want_prev=True)
    t = lambda x, dt: torch.as_tensor(x).to(dev(), dt)
    b = B.observe(t(src, torch.int64), t(dst, torch.int64), t(ts, torch.float64), t(eids, torch.int64),
                  efeats=t(st['efeats'][lo + 1:hi + 1], torch.float32), want_prev=True)
    assert torch.equal(a.h[:3 * (hi - lo)], b.h[:3 * (hi - lo)])
    assert_same_state(state_of(A), state_of(B))


def test_refusals_come_before_anything_runs():
    A, B, st = twins()
    lo, hi = BATCHES[0]
    src, dst, _, ts, eids = batch(st, lo, hi)
    rows = st['efeats'][lo + 1:hi + 1]
    s0, g0, table0 = state_of(B), B.graph, B.raw_feat_getter.efeats

    def untouched():
        assert_same_state(state_of(B), s0)
        assert B.graph is g0 and B.raw_feat_getter.efeats is table0
    B.train()
    with pytest.raises(RuntimeError, match='eval'):
        B.observe(src, dst, ts, eids, efeats=rows)
    B.eval()
    untouched()
    B._row_of = torch.zeros(B.n_nodes, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError, match='partitioned'):
        B.observe(src, dst, ts, eids, efeats=rows)
    B._row_of = None
    untouched()
    with pytest.raises(ValueError, match='no row of the edge table'):   # without their rows the eids lie past the table
        B.observe(src, dst, ts, eids)
    bad = eids.copy()
    bad[5] = E0 + 1 + len(eids)
    with pytest.raises(ValueError, match='no row of the edge table'):
        B.observe(src, dst, ts, bad, efeats=rows)
    with pytest.raises(ValueError, match='efeats'):
        B.observe(src, dst, ts, eids, efeats=rows[:-1])
    with pytest.raises(ValueError, match='before the latest event'):   # what Graph.extended refuses
        B.observe(src, dst, ts - 1e6, eids, efeats=rows)
    with pytest.raises(ValueError, match='node ids'):
        B.observe(np.full_like(src, B.n_nodes), dst, ts, eids, efeats=rows)
    untouched()
    feed(A, B, st, lo, hi)   # and the model still follows its twin


def test_append_edge_rows_grows_geometrically_and_reports_a_moved_table():
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    rs = np.random.RandomState(0)
    rows = torch.from_numpy(rs.standard_normal((300, 8)).astype(np.float32))
    fg = NumericalFeature(None, rows[:10], dim=8).to(dev())
    moved = [fg.append_edge_rows(rows[lo:hi]) for lo, hi in ((10, 11), (11, 20), (20, 21), (21, 150), (150, 300))]
    assert moved == [True, False, True, True, True]
    assert torch.equal(fg.efeats.cpu(), rows) and fg.n_edges == 300
    assert not fg.append_edge_rows(rows[:0]) and fg.efeats.shape[0] == 300
    assert NumericalFeature(None, None, dim=8).append_edge_rows(rows[:3]) is False   # no edge table: nothing to do
    pinned = NumericalFeature(None, rows[:10], dim=8, register_buffer=False)
    with pytest.raises(NotImplementedError, match='pinned'):
        pinned.append_edge_rows(rows[10:12])
