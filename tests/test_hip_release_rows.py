"""TIGE.release_edge_rows / TIGE.forget(release_edge_rows=True) on the GPU.  Twin models with equal weights (the
construction of tests/test_hip_forget.py with an 8-wide edge table: d = 16, d_e = 8, one layer, `recent_edges`, K = M = 10,
a sequence restarter with hist_len 7) observe the same ragged batches of 64 / 1 / 98 events and forget all but every
node's last M entries after every batch.  Twin A also releases the edge-table rows that no kept entry names and feeds its
later eids through the returned shift; twin B never releases.  Embeddings and the whole state stay equal bit for bit while
A's table stays small.

The stream runs over 6 users and 6 items (13 node ids) instead of 60 and 15: with 75 nodes and 200 events hardly a node
has more than M entries and no row would ever be released.

The bound on A's table: after forget(keep_last=M) no row of the graph has more than M entries, every entry names one
table row, and a live row is named by at least one entry, so rows <= 1 (padding) + M * num_node + pending - inside the
looser 1 + 2 * M * num_node + pending, which is asserted as well.  The exact count is asserted too: 1 + distinct eids of
the graph + pending."""
import numpy as np
import pytest
import torch

from test_hip_observe import BATCHES, E0, install_seq_restarter
from test_hip_rank import assert_same_state, batch, build, dev, state_of

pytestmark = pytest.mark.gpu

M = 10    # = n_neighbors; the sequence restarter reads 7 <= M
D_E = 8


def twin(forms, *, preloaded):
    """a model over the first E0 events that has streamed them.  preloaded: the table holds the rows of the whole stream
    from the start (as examples/recommend.py --online has them) - the rows behind E0 are pending; otherwise it holds the
    first E0 + 1 rows and observe(efeats=...) appends"""
    from www2023tiger_amd.data.graph import Graph
    m, _, st = build(16, D_E, M, n_u=6, n_i=6)
    m.graph = Graph.from_arrays(*(st[k][:E0] for k in ('src', 'dst', 'ts', 'eids')), strategy='recent_edges', seed=0,
                                max_node_id=st['n_nodes'] - 1, device=dev())
    if not preloaded:
        m.raw_feat_getter.efeats = m.raw_feat_getter.efeats[:E0 + 1].clone()
    m.invalidate_struct()
    install_seq_restarter(m)
    if 'fused' in forms:
        m.fuse_attention()
    if 'eager' in forms:
        m.eager_updates()
    m.stream_step(*batch(st, 0, E0))
    return m, st


def observe(model, st, lo, hi, shift=0, with_rows=True):
    src, dst, neg, ts, eids = batch(st, lo, hi)
    buf = model.observe(src, dst, ts, eids - shift, efeats=st['efeats'][lo + 1:hi + 1] if with_rows else None, neg=neg)
    return buf.h[:3 * (hi - lo)].clone()


def live_rows(graph):
    e = graph._tensors()[3]
    return int(torch.unique(e & 0x7FFFFFFF).numel())


@pytest.mark.parametrize('preloaded', [False, True], ids=['appended', 'preloaded'])
@pytest.mark.parametrize('forms', [(), ('fused', 'eager')], ids=['default', 'fused+eager'])
def test_a_twin_that_releases_rows_stays_bit_identical_and_its_table_stays_small(forms, preloaded):
    A, st = twin(forms, preloaded=preloaded)
    B, _ = twin(forms, preloaded=preloaded)
    assert_same_state(state_of(A), state_of(B))
    assert A.n_neighbors == M and A.restarter_fn.hist_len <= M and st['efeats'].shape == (201, D_E)
    E, N = 200, st['n_nodes']
    shift = 0
    cand = torch.arange(7, 13, device=dev())   # the items
    for lo, hi in BATCHES:
        ha = observe(A, st, lo, hi, shift, with_rows=not preloaded)
        hb = observe(B, st, lo, hi, 0, with_rows=not preloaded)
        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)), f'h of batch [{lo}, {hi})'
        assert_same_state(state_of(A), state_of(B))
        B.forget(keep_last=M)
        parent, old_table = A.graph, A.raw_feat_getter.efeats
        p_arrays, t0 = [t.clone() for t in parent._tensors()], old_table.clone()
        rows_before = old_table.shape[0]
        first_unobserved = hi + 1 - shift   # in A's numbering
        g = A.forget(keep_last=M, release_edge_rows=True, keep_from=first_unobserved if preloaded else None)
        res = A.last_release
        assert g is A.graph is A.restarter_fn.graph is A.temporal_embedding_fn.graph and g is not parent
        assert (res.rows_before, res.rows, res.shift) == (rows_before, A.raw_feat_getter.efeats.shape[0], rows_before - res.rows)
        assert A.raw_feat_getter.n_edges == res.rows
        # the released parent and the old table are what they were
        for a, b in zip(parent._tensors(), p_arrays):
            assert torch.equal(a, b)
        assert torch.equal(old_table.view(torch.int32), t0.view(torch.int32))
        # indptr / ts / nbr as B's trimmed graph, the eids B's pushed through every remap so far
        for i in range(3):
            assert torch.equal(g._tensors()[i], B.graph._tensors()[i])
        pending = E - hi if preloaded else 0
        assert res.rows == 1 + live_rows(g) - (1 if bool((g._tensors()[3] & 0x7FFFFFFF == 0).any()) else 0) + pending
        assert res.rows <= 1 + M * N + pending <= 1 + 2 * M * N + pending
        assert res.rows <= rows_before
        if preloaded:   # the pending rows moved as one block
            assert torch.equal(res.remap[first_unobserved:].cpu(),
                               torch.arange(first_unobserved, rows_before, dtype=torch.int32) - res.shift)
        shift += res.shift
        # every entry of A names the row of features that B's entry names
        ea, eb = (x._tensors()[3].long() & 0x7FFFFFFF for x in (g, B.graph))
        assert torch.equal(A.raw_feat_getter.efeats[ea].view(torch.int32), B.raw_feat_getter.efeats[eb].view(torch.int32))
        assert torch.equal(g._tensors()[3] >> 31, B.graph._tensors()[3] >> 31)
        assert_same_state(state_of(A), state_of(B))   # the release touches no memory, mailbox or derived table
        # recommendations with the seen filter
        q = torch.from_numpy(st['src'][lo:lo + 40]).to(dev())
        t = torch.full((40,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
        for a, b, nm in zip(A.recommend(q, t, cand, 5, exclude_seen=True), B.recommend(q, t, cand, 5, exclude_seen=True),
                            ('ids', 'scores', 'n_valid')):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), nm
        # the sequence restarter reads history eids: from the renumbered graph, the same rows
        nodes = torch.unique(torch.from_numpy(np.concatenate([st['src'][lo:hi], st['dst'][lo:hi]]))).to(dev())
        tt = torch.full((nodes.numel(),), float(st['ts'][hi - 1]), dtype=torch.float64, device=dev())
        from www2023tiger_amd import hip_ops
        bm_a, bm_b = hip_ops.new_bitmap(N, dev()), hip_ops.new_bitmap(N, dev())
        na, nb = A.restart_involved(nodes, tt, bm_a), B.restart_involved(nodes, tt, bm_b)
        assert na == nb > 0 and torch.equal(bm_a, bm_b)
        assert_same_state(state_of(A), state_of(B))
    assert shift > E // 2   # more than half of the rows were released on the way
    assert B.raw_feat_getter.efeats.shape[0] == E + 1   # the twin that never releases has every row
    assert A.raw_feat_getter.efeats.shape[0] == E + 1 - shift


def test_observe_after_a_release_appends_at_row_n_live_without_moving_the_table():
    A, st = twin((), preloaded=False)
    lo, hi = BATCHES[0]
    observe(A, st, lo, hi)
    A.forget(keep_last=M, release_edge_rows=True)
    res, fg = A.last_release, A.raw_feat_getter
    n_live = res.rows
    assert fg._ef_store.shape[0] == n_live + max(16, n_live // 4) and fg.efeats.data_ptr() == fg._ef_store.data_ptr()
    ptr0 = fg.efeats.data_ptr()
    lo, hi = BATCHES[1]   # one event: the head-room takes it
    observe(A, st, lo, hi, res.shift)
    assert fg.efeats.shape[0] == n_live + 1 and fg.efeats.data_ptr() == ptr0
    assert torch.equal(fg.efeats[n_live].cpu().view(torch.int32), torch.from_numpy(st['efeats'][hi]).view(torch.int32))
    assert int(A.graph._tensors()[3].max()) == n_live   # the new event names the appended row
    # slack=: that many spare rows
    res = A.release_edge_rows(slack=0)
    assert fg._ef_store.shape[0] == res.rows == fg.efeats.shape[0]


def test_forget_without_the_flag_leaves_table_and_eids_untouched():
    A, st = twin((), preloaded=False)
    lo, hi = BATCHES[0]
    observe(A, st, lo, hi)
    table, ptr0 = A.raw_feat_getter.efeats.clone(), A.raw_feat_getter.efeats.data_ptr()
    parent = A.graph
    g = A.forget(keep_last=M)
    assert A.last_release is None
    assert A.raw_feat_getter.efeats.data_ptr() == ptr0 and torch.equal(A.raw_feat_getter.efeats, table)
    want = parent.trimmed(keep_last=M)
    for a, b in zip(g._tensors(), want._tensors()):
        assert torch.equal(a, b)
    assert int((g._tensors()[3] & 0x7FFFFFFF).max()) == hi   # old numbers


def test_refusals_change_nothing():
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    A, st = twin((), preloaded=False)
    lo, hi = BATCHES[0]
    observe(A, st, lo, hi)

    def snapshot():
        return state_of(A), A.graph, [t.clone() for t in A.graph._tensors()], A.raw_feat_getter.efeats, \
            A.raw_feat_getter.efeats.clone(), A._struct_cache

    def unchanged(s):
        assert_same_state(state_of(A), s[0])
        assert A.graph is s[1] and A.restarter_fn.graph is s[1] and A.raw_feat_getter.efeats is s[3]
        assert all(torch.equal(a, b) for a, b in zip(A.graph._tensors(), s[2])) and torch.equal(s[3], s[4])
        assert A._struct_cache is s[5]

    s = snapshot()
    A._row_of = torch.zeros(A.n_nodes, dtype=torch.int32, device=dev())
    for call in (lambda: A.release_edge_rows(), lambda: A.forget(keep_last=3, release_edge_rows=True)):
        with pytest.raises(RuntimeError, match='partitioned'):
            call()
    A._row_of = None
    unchanged(s)
    for kw in (dict(keep_from=-1), dict(keep_from=hi + 2), dict(pin=[hi + 1]), dict(pin=[-3]), dict(slack=-1)):
        with pytest.raises(ValueError):
            A.release_edge_rows(**kw)
        unchanged(s)
    with pytest.raises(ValueError, match='negative'):
        A.forget(keep_last=-2, release_edge_rows=True)
    unchanged(s)
    # an entry that names no row: the plan reports n_live = -1, Python raises, model, graph and table are what they were
    fg = A.raw_feat_getter
    full = fg.efeats
    fg.efeats = full[:hi].clone()   # one row short of the graph's largest eid
    s = snapshot()
    with pytest.raises(ValueError, match='names no row'):
        A.release_edge_rows()
    unchanged(s)
    with pytest.raises(ValueError, match='names no row'):
        A.forget(keep_last=M, release_edge_rows=True)   # eid `hi` belongs to the newest event: the trim keeps it
    unchanged(s)
    fg.efeats = full
    # a table in pinned host memory
    pinned = NumericalFeature(None, torch.from_numpy(st['efeats']), dim=16, register_buffer=False)   # (dim: unused here)
    A.raw_feat_getter, keep = pinned, A.raw_feat_getter
    g0 = A.graph
    with pytest.raises(NotImplementedError, match='pinned host memory'):
        A.release_edge_rows()
    assert A.graph is g0 and pinned.efeats.shape[0] == 201
    A.raw_feat_getter = keep


def test_a_model_without_an_edge_table_returns_none_and_keeps_its_graph():
    A, st = twin((), preloaded=False)
    A.raw_feat_getter.efeats = None
    g0 = A.graph
    arrays = [t.clone() for t in g0._tensors()]
    assert A.release_edge_rows() is None and A.last_release is None
    assert A.graph is g0 and all(torch.equal(a, b) for a, b in zip(g0._tensors(), arrays))
    g1 = A.forget(keep_last=3, release_edge_rows=True)   # the trim alone
    assert g1 is A.graph and A.last_release is None
    for a, b in zip(g1._tensors(), g0.trimmed(keep_last=3)._tensors()):
        assert torch.equal(a, b)


def test_the_online_example_releases_rows_and_answers_the_same(tmp_path):
    """examples/recommend.run_online(keep_last=M, release_rows=True) with M >= max(n_neighbors, hist_len) on toy JODIE
    files with an 8-wide edge table answers exactly what the online replay that never forgets answers - ids are compared
    through the metrics as tests/test_hip_forget.py does for the forgetting replay -, and the table shrinks on the way.
    (The replays run with offline=False, as in that test: on these toy files the example's own online / offline equality
    does not hold even for the plain replay that neither forgets nor releases.)"""
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
    never, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, offline=False, **kw)
    online, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keep_last=6, release_rows=True, verbose=False, offline=False, **kw)
    forgot, rows = online.pop('forgot'), online.pop('rows')
    assert online == never and online['n_events'] > 0 and online['hit_rate'] > 0   # the two metric lines
    assert len(rows) == len(forgot) == -(-online['n_events'] // 100)
    assert rows[0][0] == n + 1 and all(after <= before for before, after in rows) and rows[-1][1] < n // 2
    assert rows[-1][1] <= 1 + 6 * z['nfeats'].shape[0]   # nothing is pending after the last batch: 1 + keep_last * num_node
