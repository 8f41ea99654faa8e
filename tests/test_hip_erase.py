"""TIGE.erase on the GPU, on build() of tests/test_hip_rank.py at the d = 8 golden checkpoint shapes (d = d_e = 8, K = 10,
one layer, `recent_edges`, 75 nodes, 200 events).  A model that starts from a graph over the first 37 events observes the
rest of the stream in ragged batches (the edge table holds every row from the start, as examples/recommend.py --online has
it), then nodes are erased and events retracted.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from _erase_ref import filtered
from test_hip_observe import BATCHES, E0
from test_hip_rank import assert_same_state, batch, build, dev, state_of

pytestmark = pytest.mark.gpu

KEYS = ('src', 'dst', 'ts', 'eids')
PER_NODE = ('left_vals', 'left_ts', 'left_active', 'right_vals', 'right_ts', 'right_active', 'msg_vals', 'msg_ts')


def graph_over(st, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, strategy='recent_edges', seed=0, max_node_id=st['n_nodes'] - 1, device=dev(), **kw)


def served(upto=200):
    """a model over the first E0 events that has streamed them and observed the stream up to event `upto`"""
    m, _, st = build(8, 8, 10)
    m.graph = graph_over(st, tuple(st[k][:E0] for k in KEYS))
    m.invalidate_struct()
    m.stream_step(*batch(st, 0, E0))
    for lo, hi in BATCHES:
        if lo < upto:
            observe(m, st, lo, min(hi, upto))
    return m, st


def observe(m, st, lo, hi):
    src, dst, neg, ts, eids = batch(st, lo, hi)
    return m.observe(src, dst, ts, eids, neg=neg)


def events_of(st, upto=200):
    return tuple(np.ascontiguousarray(st[k][:upto]) for k in KEYS)


def erased_nodes(st, upto=200):
    """three users and two items with history, one node that never occurs, one id twice; never 0"""
    src, dst = st['src'][:upto], st['dst'][:upto]
    u, cu = np.unique(src, return_counts=True)
    i, ci = np.unique(dst, return_counts=True)
    never = np.setdiff1d(np.arange(1, st['n_nodes']), np.concatenate([st['src'], st['dst']]))
    S = np.concatenate([u[np.argsort(-cu)][:3], i[np.argsort(-ci)][:2], never[:1]])
    assert 0 not in S and len(np.unique(S)) == len(S)
    return np.concatenate([S, S[:1]]).astype(np.int64)


def bits_of(words, ids):
    ids = torch.as_tensor(ids).to(words.device)
    return (words[ids >> 6] >> (ids & 63)) & 1


def same_graph(g, ref, what=''):
    for a, b, nm in zip(g._tensors(), ref._tensors(), ('indptr', 'ts', 'nbr', 'eid')):
        assert a.dtype == b.dtype and torch.equal(a, b), f'{what} {nm}'


def same_out(a, b, what):
    for x, y, nm in zip(a, b, ('ids', 'scores', 'n_valid')):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), f'{what} {nm}'


def test_erased_nodes_leave_the_graph_and_their_state_rows_are_those_of_a_reset_model():
    m, st = served()
    S = erased_nodes(st)
    before, parent = state_of(m), m.graph
    p_arrays = [t.clone() for t in parent._tensors()]
    five = torch.from_numpy(S[:5]).to(dev())
    assert bool(bits_of(before['has_msg'], five).any()) and bool((before['msg_vals'][five] != 0).any())
    assert bool((before['left_vals'][five] != 0).any()) or bool((before['right_vals'][five] != 0).any())
    g = m.erase(nodes=S)
    assert g is m.graph is m.restarter_fn.graph is m.temporal_embedding_fn.graph and g is not parent
    assert g.serial != parent.serial and g.num_node == parent.num_node
    ev = events_of(st)
    same_graph(g, graph_over(st, filtered(ev, S)), 'erase(nodes)')
    for a, b in zip(parent._tensors(), p_arrays):
        assert torch.equal(a, b), 'the parent graph is what it was'
    indptr = g._tensors()[0].cpu().numpy()
    assert not np.diff(indptr)[S].any() and not np.isin(g._tensors()[2].cpu().numpy(), S).any()
    # the rows of S: those of a freshly reset model
    fresh, _, _ = build(8, 8, 10)
    fresh.reset()
    after, zero = state_of(m), state_of(fresh)
    ids = torch.from_numpy(S).to(dev())
    for k in PER_NODE:
        assert torch.equal(after[k][ids], zero[k][ids]), k
    assert not bool(bits_of(after['has_msg'], S).any()) and not bool(bits_of(zero['has_msg'], S).any())
    # every other row of every state tensor: bit-identical to its value before the call
    others = torch.ones(m.n_nodes, dtype=torch.bool, device=dev())
    others[ids] = False
    for k in PER_NODE:
        a, b = after[k][others], before[k][others]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b), k
    rest = torch.arange(m.n_nodes, device=dev())[others]
    assert torch.equal(bits_of(after['has_msg'], rest), bits_of(before['has_msg'], rest))
    assert bool(bits_of(after['has_msg'], rest).any())
    spare = torch.arange(m.n_nodes, after['has_msg'].numel() * 64, device=dev())   # (bits past n_nodes)
    assert not bool(bits_of(after['has_msg'], spare).any())


def test_recommendations_after_an_erase_equal_a_model_given_the_state_and_the_filtered_graph():
    m, st = served()
    S = erased_nodes(st)
    m.erase(nodes=S)
    twin, _, _ = build(8, 8, 10)
    L, R, M = twin.left_memory, twin.right_memory, twin.msg_store
    s = state_of(m)
    for dst_t, k in ((L.vals, 'left_vals'), (L.update_ts, 'left_ts'), (L.active_mask, 'left_active'), (R.vals, 'right_vals'),
                     (R.update_ts, 'right_ts'), (R.active_mask, 'right_active'), (M.node_msg_vals, 'msg_vals'),
                     (M.node_msg_ts, 'msg_ts'), (M.has_msg_bits, 'has_msg')):
        dst_t.copy_(s[k])
    twin.graph = graph_over(st, filtered(events_of(st), S))
    twin.invalidate_struct()
    twin.invalidate_pending()
    q = torch.from_numpy(np.concatenate([st['src'][100:140], S[:3]])).to(dev())
    t = torch.full((q.numel(),), float(st['ts'][-1]) + 1.0, dtype=torch.float64, device=dev())
    cand = torch.arange(61, 76, device=dev())   # the items
    got = m.recommend(q, t, cand, 5, exclude_seen=True)
    same_out(got, twin.recommend(q, t, cand, 5, exclude_seen=True), 'recommend')
    # an erased user has seen nothing: no item is excluded (n_valid counts the candidates left to rank)
    assert int(got[2][-3:].min()) == cand.numel() > int(got[2][:40].min())
    a, b = m.recommend_walk(q, t, 5, C=16), twin.recommend_walk(q, t, 5, C=16)
    same_out(a[:3], b[:3], 'recommend_walk')
    for k in ('ids', 'counts', 'n_valid'):
        assert torch.equal(a[3][k], b[3][k]), f'recommend_walk cand {k}'
    assert int(a[3]['n_valid'].sum()) > 0 and not np.isin(a[3]['ids'].cpu().numpy(), S).any()
    assert not bool(a[3]['n_valid'][-3:].any())   # an erased user walks nowhere


def test_retracted_events_release_exactly_their_rows_and_the_model_computes_the_same():
    A, st = served()
    B, _ = served()
    rs = np.random.RandomState(4)
    R = np.concatenate([rs.choice(np.arange(1, 201), 30, replace=False), [200, 999]])   # (999 names no entry, 200 twice)
    n_ret = len(np.unique(R[R <= 200]))
    parent, table0 = A.graph, A.raw_feat_getter.efeats
    assert table0.shape[0] == 201
    gb = B.erase(eids=R)
    assert B.last_release is None and B.raw_feat_getter.efeats.shape[0] == 201
    ev = events_of(st)
    same_graph(gb, graph_over(st, filtered(ev, None, R)), 'erase(eids)')
    assert gb.tcsr.num_entry == 2 * (200 - n_ret)
    assert_same_state(state_of(A), state_of(B))   # a retraction touches no memory and no mailbox row
    ga = A.erase(eids=torch.as_tensor(R), release_edge_rows=True)
    res = A.last_release
    assert ga is A.graph is A.restarter_fn.graph and ga is not parent and parent.tcsr.num_entry == 400
    # the table shrinks by exactly the rows that only R named
    assert (res.rows_before, res.rows, res.shift) == (201, 201 - n_ret, n_ret) and A.raw_feat_getter.efeats.shape[0] == res.rows
    remap = res.remap.cpu().numpy()
    gone = np.isin(np.arange(201), R)
    assert (remap[gone] == -1).all() and np.array_equal(remap[~gone], np.arange(201 - n_ret))
    assert torch.equal(A.raw_feat_getter.efeats.view(torch.int32), table0[torch.from_numpy(~gone).to(dev())].view(torch.int32))
    # last_release.remap maps the surviving eids: A's graph is B's with the eids pushed through it
    for i in range(3):
        assert torch.equal(ga._tensors()[i], gb._tensors()[i])
    eb = gb._tensors()[3]
    want = res.remap[(eb & 0x7FFFFFFF).long()] | (eb & -0x80000000)
    assert torch.equal(ga._tensors()[3], want.to(torch.int32)) and bool((ga._tensors()[3] < 0).any())
    assert_same_state(state_of(A), state_of(B))
    # embeddings of a fixed query set
    cand = torch.arange(1, A.n_nodes, device=dev())
    t = float(st['ts'][-1]) + 1.0
    ha, hb = A.embed_catalogue(cand, t).h, B.embed_catalogue(cand, t).h
    assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)) and bool((ha != 0).any())
    q = torch.from_numpy(st['src'][100:140]).to(dev())
    tq = torch.full((40,), t, dtype=torch.float64, device=dev())
    items = torch.arange(61, 76, device=dev())
    same_out(A.recommend(q, tq, items, 5, exclude_seen=True), B.recommend(q, tq, items, 5, exclude_seen=True), 'recommend')


def test_an_erased_id_that_a_later_observe_brings_back_starts_as_a_node_never_seen():
    lo, hi = BATCHES[0]
    m, st = served(upto=hi)
    later = np.concatenate([st['src'][hi:], st['dst'][hi:]])
    S = np.intersect1d(np.concatenate([st['src'][:hi], st['dst'][:hi]]), later)[:6]
    S = S[S != 0]
    assert len(S) >= 4
    m.erase(nodes=S)
    assert not np.diff(m.graph._tensors()[0].cpu().numpy())[S].any()
    for lo2, hi2 in BATCHES[1:]:
        buf = observe(m, st, lo2, hi2)
        assert bool(torch.isfinite(buf.h[:2 * (hi2 - lo2)]).all())
    rest = tuple(np.ascontiguousarray(st[k][hi:]) for k in KEYS)
    want = graph_over(st, filtered(events_of(st, hi), S)).extended(*rest)
    same_graph(m.graph, want, 'observe after erase')
    deg = np.diff(m.graph._tensors()[0].cpu().numpy())
    np.testing.assert_array_equal(deg[S], np.bincount(later, minlength=m.n_nodes)[S])   # only what came after the erase


def test_a_catalogue_snapshot_taken_before_an_erase_is_stale():
    m, st = served()
    S = erased_nodes(st)
    cand = torch.arange(61, 76, device=dev())
    t = float(st['ts'][-1]) + 1.0
    q = torch.from_numpy(st['src'][100:120]).to(dev())
    tq = torch.full((20,), t, dtype=torch.float64, device=dev())
    snap = m.embed_catalogue(cand, t)
    m.recommend(q, tq, snap, 5)
    m.erase(nodes=S)
    with pytest.raises(RuntimeError, match='stale'):
        m.recommend(q, tq, snap, 5)
    snap = m.embed_catalogue(cand, t)
    m.recommend(q, tq, snap, 5)
    m.erase(eids=[10 ** 6])   # nothing goes, and still another graph
    with pytest.raises(RuntimeError, match='stale'):
        m.recommend(q, tq, snap, 5)


def test_refusals_change_nothing():
    m, st = served()
    S = erased_nodes(st)
    s0, g0, serial, table0 = state_of(m), m.graph, m.graph.serial, m.raw_feat_getter.efeats

    def untouched():
        assert_same_state(state_of(m), s0)
        assert m.graph is g0 and m.restarter_fn.graph is g0 and g0.serial == serial and m.raw_feat_getter.efeats is table0

    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.erase(nodes=S)
    m.eval()
    untouched()
    m._row_of = torch.zeros(m.n_nodes, dtype=torch.int32, device=dev())
    for kw in (dict(nodes=S), dict(eids=[3], release_edge_rows=True)):
        with pytest.raises(RuntimeError, match='partitioned'):
            m.erase(**kw)
    m._row_of = None
    untouched()
    for kw, match in ((dict(nodes=[5, 0]), 'padding id'), (dict(nodes=[m.n_nodes]), r'\[0, num_node\)'),
                      (dict(nodes=[-2], eids=[3]), r'\[0, num_node\)'), (dict(eids=[-1]), 'non-negative'), (dict(), 'both None'),
                      (dict(nodes=[5, 0], release_edge_rows=True), 'padding id')):
        with pytest.raises(ValueError, match=match):
            m.erase(**kw)
        untouched()
    with pytest.raises(ValueError):   # what release_edge_rows refuses: nothing at all has changed
        m.erase(eids=[3], release_edge_rows=True, keep_from=-1)
    untouched()
    m.erase(nodes=S)   # and it still works
    assert m.graph is not g0


def test_the_online_example_erases_once_before_the_replay(tmp_path):
    """examples/recommend.run_online(erase_nodes=..., retract_eids=...) on the toy JODIE files of
    tests/test_hip_release_rows.py: the entries it reports dropped are those of the train + validation events that name an
    erased node or a retracted eid, and the replay - which brings erased ids back - runs to its end."""
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
    n, rs = len(z['src']), np.random.RandomState(0)
    z['labels'] = np.zeros(n, dtype=np.int64)
    z['efeats'] = rs.standard_normal((n + 1, 8)).astype(np.float32)
    z['nfeats'] = np.zeros((int(max(z['src'].max(), z['dst'].max())) + 1, 8), dtype=np.float32)
    z['efeats'][0] = 0
    write_files(str(tmp_path), 'toy', z)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    S = np.unique(np.concatenate([z['src'][-30:-27], z['dst'][-3:]])).astype(np.int64)   # ids the test split brings back
    R = np.array([3, 4, 4, n + 50], dtype=np.int64)
    online, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, offline=False, verbose=False, erase_nodes=S, retract_eids=R, **kw)
    kept, dropped = online['erased']
    n_seen = n - online['n_events']
    assert 0 < n_seen < n
    gone = np.isin(z['src'][:n_seen], S) | np.isin(z['dst'][:n_seen], S) | np.isin(np.arange(1, n_seen + 1), R)
    assert dropped == 2 * int(gone.sum()) > 4 and kept == 2 * (n_seen - int(gone.sum()))
    assert 0 <= online['hit_rate'] <= 1
