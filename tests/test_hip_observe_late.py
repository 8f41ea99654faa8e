"""TIGE.observe_late on the GPU (d = 8, 65 nodes, batches of 16 - 32 events; the model of tests/test_hip_online_state.py with a
sequence restarter).  Model A observes the stream with a seeded third of every batch held back and admits the held events one
batch later, shuffled, through `observe_late`.  Model B is given A's state and a graph built in one go by `from_arrays` over
the whole stream in the order A was handed it, so that eids - edge-table rows - and the few equal times fall as they did for
A.  What is READ from the graph must agree bit for bit; what `observe_late` must not touch is compared before and after
every call."""
import io

import numpy as np
import pytest
import torch

from test_hip_keyed_online import scramble
from test_hip_online_state import E0, KEYS, assert_twins, build, stream
from test_hip_rank import assert_same_state, dev, state_of

pytestmark = pytest.mark.gpu

D = 8
BATCHES = [(40, 72), (72, 96), (96, 112), (112, 144), (144, 170), (170, 200)]   # 32, 24, 16, 32, 26, 30 events


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def start():
    st, nf = stream(D)
    A = build(st, nf, st['n_nodes'], E0, d=D)
    A.stream_step(*(st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')))
    return A, st, nf


def admit_late(A, st, idx, rows):
    """events idx of the stream, late and in the given order, with the table rows `rows` -> nothing but the graph and the
    edge table may have changed"""
    before, g0, n_rows = state_of(A), A.graph, A.raw_feat_getter.efeats.shape[0]
    p_arrays = [t.clone() for t in g0._tensors()]
    g = A.observe_late(st['src'][idx], st['dst'][idx], st['ts'][idx], rows, efeats=st['efeats'][idx + 1])
    assert g is A.graph is A.restarter_fn.graph is A.temporal_embedding_fn.graph and g is not g0 and g.serial != g0.serial
    assert g.tcsr.num_entry == g0.tcsr.num_entry + 2 * len(idx)
    assert_same_state(state_of(A), before)   # both memories and the mailbox, bit for bit
    assert A.raw_feat_getter.efeats.shape[0] == n_rows + len(idx)
    assert torch.equal(A.raw_feat_getter.efeats[n_rows:].cpu(), torch.from_numpy(st['efeats'][idx + 1]))
    for a, b in zip(g0._tensors(), p_arrays):
        assert torch.equal(a, b), 'the parent graph is what it was'


def arrival_plan(n_events=200, seed=7):
    """-> [(is it late?, stream indices in the order they are handed over)]: of every batch a seeded third - never its first
    event, always its second - is held back and arrives, shuffled, behind the NEXT batch's on-time events (the last
    batch's behind its own)"""
    rs = np.random.RandomState(seed)
    steps, pending = [], None
    for lo, hi in BATCHES:
        idx = np.arange(lo, hi)
        late = rs.uniform(size=hi - lo) < 1 / 3
        late[0], late[1] = False, True
        steps.append((False, idx[~late]))
        if pending is not None:
            steps.append((True, pending))
        pending = rs.permutation(idx[late])
    steps.append((True, pending))
    assert sorted(np.concatenate([i for _, i in steps]).tolist()) == list(range(E0, n_events))
    return steps


@pytest.fixture(scope='module')
def served():
    """-> A after the replay with late events; B with A's state over `from_arrays` of the whole stream IN THE ORDER A WAS
    HANDED IT (eid = edge-table row = position in that order: the stable per-node sort by time then breaks the stream's few
    equal times as the merges did); the stream; B's stream; the indices of the late events"""
    A, st, nf = start()
    next_row, late_all, order = E0 + 1, [], [np.arange(E0)]
    for is_late, idx in arrival_plan():
        rows = next_row + np.arange(len(idx))
        next_row += len(idx)
        order.append(idx)
        if is_late:
            admit_late(A, st, idx, rows)
            late_all.append(idx)
        else:
            A.observe(st['src'][idx], st['dst'][idx], st['ts'][idx], rows, efeats=st['efeats'][idx + 1])
    order, late_all = np.concatenate(order), np.concatenate(late_all)
    assert next_row == 201 and len(late_all) > 40
    st_b = dict(st, eids=np.arange(1, 201), efeats=np.concatenate([st['efeats'][:1], st['efeats'][order + 1]]),
                **{k: np.ascontiguousarray(st[k][order]) for k in ('src', 'dst', 'ts')})
    assert not np.all(st_b['ts'][1:] >= st_b['ts'][:-1])
    B = build(st_b, nf, st['n_nodes'], 200, d=D)
    for (ka, va), (kb, vb) in zip(A.named_parameters(), B.named_parameters()):   # build() seeds every initialiser
        assert ka == kb and torch.equal(va, vb), ka
    L, R, M, s = B.left_memory, B.right_memory, B.msg_store, state_of(A)
    for dst_t, k in ((L.vals, 'left_vals'), (L.update_ts, 'left_ts'), (L.active_mask, 'left_active'), (R.vals, 'right_vals'),
                     (R.update_ts, 'right_ts'), (R.active_mask, 'right_active'), (M.node_msg_vals, 'msg_vals'),
                     (M.node_msg_ts, 'msg_ts'), (M.has_msg_bits, 'has_msg')):
        dst_t.copy_(s[k])
    B.invalidate_struct()
    B.invalidate_pending()
    return A, B, st, st_b, late_all


def test_the_graph_and_the_table_are_those_of_the_whole_stream(served):
    from www2023tiger_amd import hip_ops
    A, B, st, _, late = served
    for a, b, nm in zip(A.graph._tensors(), B.graph._tensors(), ('indptr', 'ts', 'nbr', 'eid')):
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b)), nm
    assert torch.equal(bits(A.raw_feat_getter.efeats), bits(B.raw_feat_getter.efeats))
    assert A.raw_feat_getter.efeats.shape[0] == 201
    assert hip_ops.tcsr_verify(A.graph, 201)[0] == 0
    assert float(A.graph._t_last) == st['ts'].max()
    assert_same_state(state_of(A), state_of(B))


def test_what_is_read_from_the_graph_agrees_bit_for_bit(served):
    from www2023tiger_amd import hip_ops
    A, B, st, _, late = served
    # the sources of late events among the queries: their rows changed most
    q = torch.from_numpy(np.concatenate([st['src'][late[:20]], st['src'][180:200]])).to(dev())
    t = torch.full((q.numel(),), float(st['ts'][-1]) + 1.0, dtype=torch.float64, device=dev())
    items = torch.unique(torch.from_numpy(st['dst'])).to(dev())
    got, want = A.recommend(q, t, items, 5, exclude_seen=True), B.recommend(q, t, items, 5, exclude_seen=True)
    for a, b, nm in zip(got, want, ('ids', 'scores', 'n_valid')):
        assert torch.equal(bits(a), bits(b)), f'recommend {nm}'
    assert int(got[2].min()) < items.numel()   # something was seen and left out
    sa, sb = A.rank_scores(q, q, t, items), B.rank_scores(q, q, t, items)
    assert torch.equal(bits(sa), bits(sb)) and bool((sa != 0).any())
    for mid in (float(st['ts'][120]), float(st['ts'][-1]) + 1.0):   # a cut inside the stream: late entries on both sides of it
        tm = torch.full_like(t, mid)
        wa = hip_ops.walk_candidates(A.graph, q, tm, 16, exclude_seen=True)
        wb = hip_ops.walk_candidates(B.graph, q, tm, 16, exclude_seen=True)
        ta, tb = hip_ops.trending(A.graph, mid, 10, window=1500.0), hip_ops.trending(B.graph, mid, 10, window=1500.0)
        for x, y, what in ((wa, wb, 'walk_candidates'), (ta, tb, 'trending')):
            for k in x:
                assert torch.equal(x[k], y[k]), f'{what} {k} at t = {mid}'
        assert int(wa['n_valid'].sum()) > 0 and int(ta['n_valid']) > 0
    nodes = torch.unique(q)
    tr = torch.full((nodes.numel(),), float(st['ts'][-1]), device=dev())
    ha, hb = A.restarter_fn(nodes, tr)[0], B.restarter_fn(nodes, tr)[0]   # the sequence restarter's histories
    assert torch.equal(bits(ha), bits(hb))


def test_a_late_event_is_seen_afterwards_and_was_not_before():
    A, st, nf = start()
    lo, hi = BATCHES[0]
    late = np.arange(lo, hi)[::3]
    on = np.setdiff1d(np.arange(lo, hi), late)
    rows = np.concatenate([np.arange(E0 + 1, E0 + 1 + len(on)), np.arange(E0 + 1 + len(on), hi + 1)])
    A.observe(st['src'][on], st['dst'][on], st['ts'][on], rows[:len(on)], efeats=st['efeats'][on + 1])
    q = torch.from_numpy(st['src'][late]).to(dev())
    t = torch.full((len(late),), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    items = torch.unique(torch.from_numpy(st['dst'][:hi])).to(dev())
    before = A.recommend(q, t, items, 5, exclude_seen=True)
    admit_late(A, st, late, rows[len(on):])
    after = A.recommend(q, t, items, 5, exclude_seen=True)
    assert int(after[2].sum()) < int(before[2].sum())   # the late events' items are now seen: fewer candidates left
    # `observe` keeps refusing the same batch
    with pytest.raises(ValueError, match='before the latest event'):
        A.observe(st['src'][late], st['dst'][late], st['ts'][late], rows[len(on):])


def test_save_and_load_round_trip_after_late_events(served):
    A, _, st, st_b, _ = served
    _, nf = stream(D)
    C = build(st_b, nf, st['n_nodes'], 3, seed=99, stub=True, d=D)
    f = io.BytesIO()
    A.save_online(f)
    f.seek(0)
    assert C.load_online(f) is C.graph   # verify=True: tg_tcsr_verify accepts the merged graph
    assert_twins(A, C, st, 200, 'loaded after observe_late')


def test_observe_late_keys_admits_an_unknown_key_and_merges():
    from www2023tiger_amd.data.idmap import IdMap
    A, st, nf = start()
    N = A.n_nodes
    idmap = IdMap.from_keys(scramble(np.arange(1, N)), dev())
    before, g0 = state_of(A), A.graph
    src_k = torch.cat([scramble(st['src'][50:53]), torch.tensor([424242], dtype=torch.int64)])
    dst_k = scramble(st['dst'][50:54])
    ts = np.array([st['ts'][5], st['ts'][30] + 0.5, -3.0, st['ts'][20]])
    new_row = torch.full((1, D), 0.25)
    g = A.observe_late_keys(idmap, src_k, dst_k, ts, np.arange(E0 + 1, E0 + 5), efeats=st['efeats'][51:55], nfeats=new_row)
    assert g is A.graph and idmap.size == A.n_nodes == g.num_node == N + 1
    assert int(idmap.lookup(torch.tensor([424242], device=dev()))) == N
    assert torch.equal(A.raw_feat_getter.nfeats[N].cpu(), new_row[0])
    after = state_of(A)
    for k, v in before.items():   # the old rows, bit for bit; the new id's rows are zero
        if k != 'has_msg':
            assert torch.equal(after[k][:N], v) and not bool(after[k][N:].any()), k
    assert torch.equal(after['has_msg'][:before['has_msg'].numel()], before['has_msg'])
    ref = g0.merged(np.concatenate([st['src'][50:53], [N]]), st['dst'][50:54], ts, np.arange(E0 + 1, E0 + 5), num_node=N + 1)
    for a, b in zip(g._tensors(), ref._tensors()):
        assert torch.equal(a, b)
    indptr = g._tensors()[0]
    assert int(indptr[N + 1] - indptr[N]) == 1


def test_every_refusal_leaves_graph_tables_and_n_nodes_as_they_were(monkeypatch):
    A, st, nf = start()
    lo, hi = BATCHES[0]
    A.observe(*(st[k][lo:hi] for k in KEYS), efeats=st['efeats'][lo + 1:hi + 1])
    idx = np.array([3, 17, 50, 60])   # in order among themselves, and all of them before the latest event
    src, dst, ts = st['src'][idx], st['dst'][idx], st['ts'][idx] + 0.25
    eids, rows = np.arange(hi + 1, hi + 5), st['efeats'][idx + 1]
    s0, g0, table0, nfeats0, n0 = state_of(A), A.graph, A.raw_feat_getter.efeats, A.raw_feat_getter.nfeats, A.n_nodes

    def untouched():
        assert_same_state(state_of(A), s0)
        fg = A.raw_feat_getter
        assert A.graph is g0 and A.restarter_fn.graph is g0 and fg.efeats is table0 and fg.nfeats is nfeats0 and A.n_nodes == n0

    A.train()
    with pytest.raises(RuntimeError, match='eval'):
        A.observe_late(src, dst, ts, eids, efeats=rows)
    A.eval()
    untouched()
    A._row_of = torch.zeros(A.n_nodes, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError, match='partitioned'):
        A.observe_late(src, dst, ts, eids, efeats=rows)
    A._row_of = None
    untouched()
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='captured'):
        A.observe_late(src, dst, ts, eids, efeats=rows)
    monkeypatch.undo()
    untouched()
    nan = ts.copy()
    nan[2] = np.nan
    for args, kw, match in (((src, dst, nan, eids), dict(efeats=rows), 'NaN'),
                            ((np.full_like(src, n0), dst, ts, eids), dict(efeats=rows), 'node ids'),
                            ((src, -dst, ts, eids), dict(efeats=rows), 'node ids'),
                            ((src, dst, ts, eids), {}, 'no row of the edge table'),          # without their rows
                            ((src, dst, ts, eids + 1), dict(efeats=rows), 'no row of the edge table'),
                            ((src, dst, ts, eids - 2 ** 40), dict(efeats=rows), '31 bits'),
                            ((src, dst, ts, eids), dict(efeats=rows[:-1]), 'efeats'),
                            ((src, dst[:-1], ts, eids), dict(efeats=rows), 'one entry per event'),
                            ((src, dst, ts, eids), dict(efeats=rows, nfeats=nf[:1]), 'nfeats'),
                            ((src, dst, ts, eids), dict(efeats=rows, num_node=n0 - 1), 'below'),
                            ((src, dst, ts, eids), dict(efeats=rows, num_node=n0 + 2, nfeats=nf[:1]), 'nfeats')):
        with pytest.raises(ValueError, match=match):
            A.observe_late(*args, **kw)
        untouched()
    with pytest.raises(ValueError, match='before the latest event'):
        A.observe(src, dst, ts, eids, efeats=rows)
    untouched()
    g = A.observe_late(src, dst, ts, eids, efeats=rows)   # and it still works
    assert g is A.graph is not g0 and A.raw_feat_getter.efeats.shape[0] == hi + 5


def test_the_online_example_holds_events_back_and_merges_them_late(tmp_path, capsys):
    """examples/recommend.run_online(late=...) on the toy JODIE files of tests/test_hip_release_rows.py: a third of every
    test batch arrives two batches late; the replay asserts that its final graph is the graph over the whole stream, and
    reports how many events it merged"""
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
    kw = dict(seed=0, bs=40, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    online, offline = rc.run_online('toy', str(tmp_path), ckpt, k=5, late=1 / 3, late_by=2, **kw)
    assert offline is None and 0 < online['late'] < online['n_events'] and 0 <= online['hit_rate'] <= 1
    assert f"late: {online['late']} of {online['n_events']} events" in capsys.readouterr().out
    with pytest.raises(ValueError, match='plain online replay'):
        rc.run_online('toy', str(tmp_path), ckpt, k=5, late=0.2, keep_last=10, **kw)
    with pytest.raises(ValueError, match='fraction'):
        rc.run_online('toy', str(tmp_path), ckpt, k=5, late=1.0, **kw)
