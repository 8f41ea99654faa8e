"""TIGE.forget on the GPU.  Twin models with equal weights observe the same ragged batches; one of them forgets all but
every node's last M entries after every batch.  With one layer, `recent_edges`, n_neighbors = M and a sequence restarter
with hist_len <= M nothing that is dropped is ever read: embeddings and the full state stay equal bit for bit while the
forgetting twin's graph stays small.  A horizon changes what `recommend(..., exclude_seen=True)` excludes - exactly as a
graph built over the filtered stream does.  On twins() of tests/test_hip_observe.py (d = 16, K = 10, E = 200)."""
import numpy as np
import pytest
import torch

from test_hip_observe import BATCHES, E0, twins
from test_hip_rank import assert_same_state, batch, dev, state_of

pytestmark = pytest.mark.gpu

M = 10   # = n_neighbors of twins(); the sequence restarter reads 7 <= M


def observe(model, st, lo, hi):
    src, dst, neg, ts, eids = batch(st, lo, hi)
    buf = model.observe(src, dst, ts, eids, efeats=st['efeats'][lo + 1:hi + 1], neg=neg)
    return buf.h[:3 * (hi - lo)].clone()


def test_a_twin_that_forgets_all_but_the_last_m_entries_stays_bit_identical():
    _, B, st = twins(seq=True, forms=('fused',))   # observes only
    _, F, _ = twins(seq=True, forms=('fused',))    # observes and forgets
    assert B.n_neighbors == M and B.restarter_fn.hist_len <= M
    dropped = 0
    for lo, hi in BATCHES:   # 64 events, one event, 98 events
        hb, hf = observe(B, st, lo, hi), observe(F, st, lo, hi)
        assert torch.equal(hb.view(torch.int32), hf.view(torch.int32)), f'h of batch [{lo}, {hi})'
        assert_same_state(state_of(B), state_of(F))
        parent = F.graph
        g = F.forget(keep_last=M)
        assert g is F.graph is F.restarter_fn.graph is F.temporal_embedding_fn.graph and g is not parent
        assert parent.tcsr.num_entry == 2 * hi - dropped   # the parent is what it was
        dropped += parent.tcsr.num_entry - g.tcsr.num_entry
        assert g.tcsr.num_entry <= M * g.num_node
        assert int(torch.diff(g._tensors()[0]).max()) <= M
        assert_same_state(state_of(B), state_of(F))   # forget touches no memory, mailbox or table
        # the sequence restarter reads its histories from the trimmed graph: the same rows
        nodes = torch.unique(torch.from_numpy(np.concatenate([st['src'][lo:hi], st['dst'][lo:hi]]))).to(dev())
        t = torch.full((nodes.numel(),), float(st['ts'][hi - 1]), device=dev())
        B.restart(nodes, t)
        F.restart(nodes, t)
        assert_same_state(state_of(B), state_of(F))
    assert dropped > 0 and F.graph.tcsr.num_entry == B.graph.tcsr.num_entry - dropped   # something was forgotten
    assert torch.equal(F.raw_feat_getter.efeats, B.raw_feat_getter.efeats)   # the edge table keeps its rows


def test_recommend_after_a_horizon_excludes_what_was_seen_inside_the_window():
    from www2023tiger_amd.data.graph import Graph
    A, B, st = twins()
    for lo, hi in BATCHES[:2]:
        a = batch(st, lo, hi)
        A.stream_step(*a)
        observe(B, st, lo, hi)
    hi = BATCHES[1][1]
    assert_same_state(state_of(A), state_of(B))
    t_cut = float(st['ts'][hi // 2])
    q = torch.from_numpy(st['src'][hi:hi + 40]).to(dev())
    t = torch.full((40,), float(st['ts'][hi]), dtype=torch.float64, device=dev())
    cand = torch.arange(61, 76, device=dev())   # the items
    unforgotten = B.recommend(q, t, cand, 5, exclude_seen=True)
    s0 = state_of(B)
    g = B.forget(before=t_cut)
    assert_same_state(state_of(B), s0)
    keep = st['ts'][:hi] >= t_cut
    assert g.tcsr.num_entry == 2 * int(keep.sum()) < 2 * hi
    A.graph = Graph.from_arrays(*(st[k][:hi][keep] for k in ('src', 'dst', 'ts', 'eids')), strategy='recent_edges', seed=0,
                                max_node_id=st['n_nodes'] - 1, device=dev())
    for a, b in zip(B.graph._tensors(), A.graph._tensors()):
        assert torch.equal(a, b)
    want = A.recommend(q, t, cand, 5, exclude_seen=True)
    got = B.recommend(q, t, cand, 5, exclude_seen=True)
    for a, b, nm in zip(got, want, ('ids', 'scores', 'n_valid')):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), nm
    assert bool((unforgotten[0] != got[0]).any(1).any())   # "seen" now means "seen inside the window"
    # the model goes on observing on the trimmed graph
    lo, hi2 = BATCHES[2]
    observe(B, st, lo, hi2)
    assert B.graph.tcsr.num_entry == g.tcsr.num_entry + 2 * (hi2 - lo)


def test_refusals_come_before_anything_runs():
    _, B, st = twins()
    s0, g0 = state_of(B), B.graph
    B._row_of = torch.zeros(B.n_nodes, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError, match='partitioned'):
        B.forget(keep_last=3)
    B._row_of = None
    with pytest.raises(ValueError, match='NaN'):
        B.forget(before=float('nan'))
    with pytest.raises(ValueError, match='negative'):
        B.forget(keep_last=-2)
    assert B.graph is g0 and B.graph.tcsr.num_entry == 2 * E0
    assert_same_state(state_of(B), s0)


def test_the_online_example_answers_the_same_when_it_forgets_what_it_never_reads(tmp_path):
    """examples/recommend.run_online(keep_last=M) with M >= max(n_neighbors, hist_len) on toy JODIE files answers exactly
    what the online replay that never forgets answers; entries are dropped on the way"""
    import os
    import sys
    from _util import load
    from test_input_side import write_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'examples'))
    import link_prediction as lp
    import recommend as rc
    z0 = load('input_side')
    z = {k: z0[k] for k in ('src', 'dst', 'ts')}
    z['labels'] = np.zeros(len(z['src']), dtype=np.int64)
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    never, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, offline=False, **kw)
    online, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keep_last=6, verbose=False, offline=False, **kw)
    forgot = online.pop('forgot')
    assert online == never and online['n_events'] > 0 and online['hit_rate'] > 0
    assert len(forgot) == -(-online['n_events'] // 100) and sum(d for _, d in forgot) > 0
    windowed, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, window=float(np.ptp(z['ts'])) / 20, exclude_seen=True,
                                verbose=False, offline=False, **kw)
    assert windowed['n_events'] == online['n_events'] and sum(d for _, d in windowed['forgot']) > 0
