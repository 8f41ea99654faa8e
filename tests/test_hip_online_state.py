"""TIGE.save_online / load_online on the GPU.  Twin runs: model A observes the whole tail of a stream; model B (equal
weights) observes a prefix and saves; model C - freshly built on a three-event stub graph and stub tables, with OTHER
parameters - loads the file and observes the rest.  After every batch A and C are compared with torch.equal: embeddings,
both memories, the mailbox, the four graph arrays, the tables, recommendations.  And what load_online refuses, each case
with a bitwise snapshot of the model before and after.  Small models (d = 8 and 16, 77 node ids, ragged batches of 1 to 40
events) on bench.make_stream with the ids renumbered in the order of their first appearance, so the tail brings new ids."""
import io

import numpy as np
import pytest
import torch

from test_hip_rank import dev

pytestmark = pytest.mark.gpu

E, E0 = 200, 40
BATCHES = [(40, 80), (80, 81), (81, 118), (118, 140), (140, 165), (165, 200)]   # ragged: 40, 1, 37, 22, 25, 35 events
SAVE_AFTER = 3                                                                    # B saves after this many batches
KEYS = ('src', 'dst', 'ts', 'eids')
_STREAMS = {}


def stream(d):
    """-> stream dict (ids in the order of their first appearance, 0 stays the padding id), nfeats [n_nodes, d]"""
    if d not in _STREAMS:
        import bench
        st = bench.make_stream(60, 15, E, 5000.0, seed=0, d_e=d, with_efeats=True)
        both = np.stack([st['src'], st['dst']], 1).reshape(-1)
        _, first = np.unique(both, return_index=True)
        order = both[np.sort(first)]
        new_id = np.zeros(st['n_nodes'], dtype=np.int64)
        new_id[order] = np.arange(1, len(order) + 1)
        st = dict(st, src=new_id[st['src']], dst=new_id[st['dst']], n_nodes=len(order) + 1)
        nf = (np.random.RandomState(1).standard_normal((st['n_nodes'], d)) * 0.3).astype(np.float32)
        nf[0] = 0
        _STREAMS[d] = (st, nf)
    return _STREAMS[d]


def ids_upto(st, hi):
    return int(max(st['src'][:hi].max(), st['dst'][:hi].max())) + 1


def build(st, nf, n_nodes, n_events, *, d, K=5, L=1, strategy='recent_edges', restarter='seq', forms=(), seed=0, stub=False,
          pinned=False):
    """a TIGER on `n_nodes` ids over the first n_events events and their edge rows; every initialiser is seeded.  stub: zeroed
    tables - what a fresh process that is about to load builds on"""
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    from www2023tiger_amd.model.restarters import SeqRestarter, StaticRestarter
    from www2023tiger_amd.model.tiger import TIGER
    g = Graph.from_arrays(*(st[k][:n_events] for k in KEYS), strategy=strategy, seed=0, max_node_id=n_nodes - 1, device=dev())
    torch.manual_seed(seed)
    nfeats, efeats = torch.from_numpy(nf[:n_nodes].copy()), torch.from_numpy(st['efeats'][:n_events + 1].copy())
    if stub:
        nfeats, efeats = torch.zeros_like(nfeats), torch.zeros_like(efeats)
    fg = NumericalFeature(nfeats, efeats, dim=d, device=dev(), register_buffer=not pinned)
    if restarter == 'seq':
        rst = SeqRestarter(raw_feat_getter=fg, graph=g, hist_len=7, n_head=2, dropout=0.0)
    else:
        rst = StaticRestarter(raw_feat_getter=fg, graph=g)
    model = TIGER(raw_feat_getter=fg, graph=g, restarter=rst, n_neighbors=K, hit_type='bin', n_layers=L, n_head=2,
                  dropout=0.0, msg_src='left', upd_src='right').to(dev())
    with torch.no_grad():
        model.time_encoder.phase.uniform_(-0.5, 0.5)
        model.hit_embedding.weight.normal_(0, 0.5)
        if restarter == 'static':
            rst.left_emb.weight.normal_(0, 0.1)
            rst.right_emb.weight.normal_(0, 0.1)
    model.eval()
    if 'fused' in forms:
        model.fuse_attention()
    if 'eager' in forms:
        model.eager_updates()
    return model


def observe(m, st, lo, hi, eids=None, **kw):
    """observe events [lo, hi) (eids: their rows in m's edge table, default lo + 1 .. hi) -> h of sources and destinations"""
    e = st['eids'][lo:hi] if eids is None else eids
    b = m.observe(st['src'][lo:hi], st['dst'][lo:hi], st['ts'][lo:hi], e, efeats=st['efeats'][lo + 1:hi + 1], **kw)
    return b.h[:2 * (hi - lo)].clone()


def everything(m):
    """every buffer (state_dict and mailbox), both tables, the four graph arrays and the parameters: clones"""
    out = {k: v.detach().clone() for k, v in m.state_dict().items()}
    S, fg = m.msg_store, m.raw_feat_getter
    out.update(msg_vals=S.node_msg_vals.clone(), msg_ts=S.node_msg_ts.clone(), has_msg=S.has_msg_bits.clone(),
               nfeats=fg.nfeats.clone(), efeats=fg.efeats.clone())
    out.update({f'graph{i}': t.clone() for i, t in enumerate(m.graph._tensors())})
    return out


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def assert_same(a, b, what=''):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])), f'{what}: {k}'


def recommend(m, st, hi):
    """the next events' sources ask for items at the time of the next event, seen items excluded"""
    q = torch.from_numpy(st['src'][hi - 20:hi]).to(dev())
    t = torch.full((20,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    items = torch.unique(torch.from_numpy(st['dst'][:hi])).to(dev())
    return m.recommend(q, t, items, 5, exclude_seen=True)


def assert_twins(A, C, st, hi, what, with_recommend=True):
    assert A.n_nodes == C.n_nodes == C.graph.num_node == C.raw_feat_getter.n_nodes == C.restarter_fn.n_nodes
    assert C.restarter_fn.graph is C.graph
    assert_same(everything(A), everything(C), what)
    if with_recommend:
        for x, y, nm in zip(recommend(A, st, hi), recommend(C, st, hi), ('ids', 'scores', 'n_valid')):
            assert torch.equal(bits(x), bits(y)), f'{what}: recommend {nm}'


VARIANTS = {
    'fused+eager': dict(d=16, K=10, forms=('fused', 'eager')),
    'two-layers-recent-nodes': dict(d=8, L=2, strategy='recent_nodes'),
    'uniform': dict(d=8, strategy='uniform'),
    'static': dict(d=8, restarter='static'),
}


def run_twins(kw, save, with_recommend=True, restart=False):
    """save(B) -> whatever C.load_online takes.  -> A, C after the run"""
    st, nf = stream(kw['d'])
    N = st['n_nodes']
    A, B = build(st, nf, N, E0, **kw), build(st, nf, N, E0, **kw)
    C = build(st, nf, N, 3, seed=99, stub=True, **kw)
    assert not torch.equal(C.score_fn.fc1.weight, A.score_fn.fc1.weight)
    for m in (A, B):
        m.stream_step(*(st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')))
    for i, (lo, hi) in enumerate(BATCHES):
        ha = observe(A, st, lo, hi)
        if i < SAVE_AFTER:
            assert torch.equal(observe(B, st, lo, hi), ha)
            if kw.get('strategy') == 'uniform':   # draws outside the step move the device stream too
                q, t = torch.arange(1, 9, device=dev()), torch.full((8,), 1e9, dtype=torch.float64, device=dev())
                for m in (A, B):
                    m.graph.sample_device(q, t, 3)
        if i == SAVE_AFTER - 1:
            g_stub = C.graph
            assert C.load_online(save(B)) is C.graph and C.graph is not g_stub and C.graph.serial != B.graph.serial
        if i >= SAVE_AFTER:
            assert torch.equal(observe(C, st, lo, hi), ha), f'h of batch [{lo}, {hi})'
        if i >= SAVE_AFTER - 1:
            assert_twins(A, C, st, hi, f'after batch [{lo}, {hi})', with_recommend)
            if restart:   # the sequence restarter reads its histories from the loaded graph
                nodes = torch.unique(torch.from_numpy(np.concatenate([st['src'][lo:hi], st['dst'][lo:hi]]))).to(dev())
                t = torch.full((nodes.numel(),), float(st['ts'][hi - 1]), device=dev())
                A.restart(nodes, t)
                C.restart(nodes, t)
                assert_twins(A, C, st, hi, f'restarted after batch [{lo}, {hi})', with_recommend)
    return A, C


def to_file(tmp_path):
    def save(B):
        B.save_online(tmp_path / 's.pt')
        return tmp_path / 's.pt'
    return save


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_a_fresh_model_that_loads_continues_as_the_uninterrupted_one(variant, tmp_path):
    kw = VARIANTS[variant]
    A, C = run_twins(kw, to_file(tmp_path), with_recommend=variant != 'uniform')
    if variant == 'uniform':   # the draws continue ONE stream: the next ones agree too
        q, t = torch.arange(1, 30, device=dev()), torch.full((29,), 1e9, dtype=torch.float64, device=dev())
        for x, y in zip(A.graph.sample_device(q, t, 4), C.graph.sample_device(q, t, 4)):
            assert torch.equal(x, y)


def test_the_sequence_restarter_restarts_after_the_load(tmp_path):
    run_twins(dict(d=8), to_file(tmp_path), restart=True)


def test_saving_to_a_file_object_and_loading_the_dict():
    def to_bytes(B):
        f = io.BytesIO()
        B.save_online(f)
        f.seek(0)
        return f
    run_twins(dict(d=8), to_bytes)
    run_twins(dict(d=8), lambda B: B.online_state())


def test_after_forget_erase_release_and_growth(tmp_path):
    """what motivates the feature: none of this can be replayed from the stream"""
    d = 8
    st, nf = stream(d)
    N0, N1 = ids_upto(st, E0), st['n_nodes']
    assert N0 < ids_upto(st, 118) < N1
    B = build(st, nf, N0, E0, d=d)
    B.stream_step(*(st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')))
    observe(B, st, 40, 80, num_node='auto', nfeats=torch.from_numpy(nf[N0:ids_upto(st, 80)]))
    B.forget(keep_last=4, release_edge_rows=True)
    assert B.last_release.shift > 0
    n1 = ids_upto(st, 118)
    rows = B.raw_feat_getter.efeats.shape[0]
    observe(B, st, 80, 118, eids=np.arange(rows, rows + 38), num_node='auto', nfeats=torch.from_numpy(nf[B.n_nodes:n1]))
    assert B.n_nodes == n1 > N0 and B.raw_feat_getter.efeats.shape[0] == rows + 38 < 119
    gone = torch.tensor([int(st['src'][50]), int(st['dst'][60])])
    live = B.graph._tensors()[3] & 0x7FFFFFFF
    B.erase(nodes=gone, eids=live[live > 0][:2].cpu(), release_edge_rows=True)
    rows = B.raw_feat_getter.efeats.shape[0]
    assert rows < B.last_release.rows_before
    B.save_online(tmp_path / 's.pt')
    C = build(st, nf, N0, E0, d=d, seed=99)   # the ORIGINAL node count and tables
    C.load_online(tmp_path / 's.pt')
    assert C.n_nodes == n1 and C.raw_feat_getter.efeats.shape[0] == rows
    assert_twins(B, C, st, 118, 'after the load')
    # the erased ids own empty rows and reset state
    indptr = C.graph._tensors()[0]
    for v in gone.tolist():
        assert int(indptr[v + 1] - indptr[v]) == 0
        assert not bool(C.left_memory.vals[v].any()) and not bool(C.right_memory.vals[v].any())
        assert not bool(C.msg_store.node_msg_vals[v].any()) and not bool(C.msg_store.has_msg_mask()[v])
    assert not bool((C.graph._tensors()[2].long().unsqueeze(1) == gone.to(dev())).any())
    for lo, hi in ((118, 140), (140, 141), (141, 200)):
        rows = B.raw_feat_getter.efeats.shape[0]
        n_now = max(B.n_nodes, ids_upto(st, hi))
        kw = dict(eids=np.arange(rows, rows + hi - lo), num_node='auto')
        hb = observe(B, st, lo, hi, nfeats=torch.from_numpy(nf[B.n_nodes:n_now]), **kw)
        hc = observe(C, st, lo, hi, nfeats=torch.from_numpy(nf[C.n_nodes:n_now]), **kw)
        assert torch.equal(hb, hc), f'h of batch [{lo}, {hi})'
        assert_twins(B, C, st, hi, f'after batch [{lo}, {hi})')
        if hi == 141:
            for m in (B, C):
                m.forget(keep_last=3, release_edge_rows=True)
            assert_twins(B, C, st, hi, 'after another forget')
    assert B.n_nodes == N1


# ---- refusals: nothing changes -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def saved():
    """the online state of a d = 8 model after two batches (a dict: every test corrupts a copy)"""
    st, nf = stream(8)
    B = build(st, nf, st['n_nodes'], E0, d=8)
    B.stream_step(*(st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')))
    for lo, hi in BATCHES[:2]:
        observe(B, st, lo, hi)
    return B.online_state()


def copy_of(state):
    c = lambda v: v.clone() if torch.is_tensor(v) else ({k: c(x) for k, x in v.items()} if isinstance(v, dict) else v)
    return c(state)


def refused(model, state, exc, pattern):
    before, g0, t0 = everything(model), model.graph, (model.raw_feat_getter.nfeats, model.raw_feat_getter.efeats)
    with pytest.raises(exc, match=pattern):
        model.load_online(state)
    assert model.graph is g0 and model.raw_feat_getter.nfeats is t0[0] and model.raw_feat_getter.efeats is t0[1]
    assert_same(everything(model), before, 'after a refusal')


def test_refusals_leave_the_model_as_it_was(saved):
    st, nf = stream(8)
    N = st['n_nodes']
    C = build(st, nf, N, 3, d=8, seed=99, stub=True)
    C.stream_step(*(st[k][:3] for k in ('src', 'dst', 'dst', 'ts', 'eids')))   # some state of its own to lose
    g = saved['graph']
    P, rows = g['ts'].numel(), saved['efeats'].shape[0]
    deg = (g['indptr'][1:] - g['indptr'][:-1])
    v = int(torch.nonzero(deg >= 3)[0])
    p = int(g['indptr'][v]) + 1

    def with_graph(key, index, value):
        s = copy_of(saved)
        s['graph'][key][index] = value
        return s
    cases = [(with_graph('indptr', 0, 1), r'ENDS.*row bound 0'),
             (with_graph('indptr', 9, -1), r'PTR_ORDER.*row 8'),
             (with_graph('ts', p, float(g['ts'][p - 1]) - 1.0), rf'TS_ORDER.*entry {p}\b'),
             (with_graph('ts', 5, float('nan')), r'TS_NAN.*entry 5'),
             (with_graph('nbr', P - 1, N), rf'NBR_RANGE.*entry {P - 1}\b'),
             (with_graph('eid', 7, rows), r'EID_RANGE.*entry 7')]
    for state, pattern in cases:
        refused(C, state, ValueError, pattern)
    s = copy_of(saved)
    s['efeats'] = s['efeats'][:-1].clone()   # an eid beyond the saved edge table
    refused(C, s, ValueError, 'EID_RANGE')
    s = copy_of(saved)
    s['mailbox']['has_msg_bits'][N // 64] |= 1 << (N % 64)   # the first spare bit
    refused(C, s, ValueError, f'has_msg_bits marks node id {N}')
    refused(C, dict(copy_of(saved), version=2), ValueError, 'version 2')
    refused(C, dict(copy_of(saved), format='tiger-graph'), ValueError, 'not a saved online state')
    s = copy_of(saved)
    del s['state_dict']['score_fn.fc1.weight']
    refused(C, s, ValueError, 'other keys')
    s = copy_of(saved)
    s['state_dict']['left_memory.vals'] = s['state_dict']['left_memory.vals'][:-1].clone()
    refused(C, s, ValueError, 'left_memory.vals')
    s = copy_of(saved)
    s['mailbox']['node_msg_ts'] = s['mailbox']['node_msg_ts'].double()
    refused(C, s, ValueError, 'node_msg_ts')
    s = copy_of(saved)
    s['nfeats'] = None
    refused(C, s, ValueError, 'nfeats table')
    C.train()
    refused(C, saved, RuntimeError, 'eval')
    C.eval()
    C._row_of = torch.zeros(1, dtype=torch.int32)   # what partition_state leaves behind
    refused(C, saved, RuntimeError, 'partitioned')
    del C._row_of
    C.load_online(copy_of(saved))   # and the uncorrupted state loads


def test_another_model_is_refused(saved):
    st, nf = stream(8)
    N = st['n_nodes']
    st16, nf16 = stream(16)
    refused(build(st16, nf16, N, 3, d=16, stub=True), saved, ValueError, r"another model.*'dim': \(8, 16\)")
    refused(build(st, nf, N, 3, d=8, K=7, stub=True), saved, ValueError, r"another model.*'n_neighbors': \(5, 7\)")
    refused(build(st, nf, N, 3, d=8, restarter='static', stub=True), saved, ValueError, 'restarter')
    # a smaller saved n_nodes: ids are never released
    big = (st, np.concatenate([nf, nf[:3]]))
    refused(build(big[0], big[1], N + 3, 3, d=8, stub=True), saved, ValueError, f'saved model has {N} node ids')


def test_tables_in_pinned_host_memory_are_refused(saved):
    st, nf = stream(8)
    C = build(st, nf, st['n_nodes'], 3, d=8, stub=True, pinned=True)
    assert not C.raw_feat_getter.nfeats.is_cuda
    refused(C, saved, NotImplementedError, 'pinned host memory')


def test_a_static_restarter_with_another_row_count_is_refused():
    st, nf = stream(8)
    N = st['n_nodes']
    B = build(st, nf, N, E0, d=8, restarter='static')
    B.stream_step(*(st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')))
    state = B.online_state()
    refused(build(st, nf, N - 2, 3, d=8, restarter='static', stub=True), state, ValueError, 'left_emb')


def test_a_snapshot_from_before_the_load_is_stale(saved):
    st, nf = stream(8)
    C = build(st, nf, st['n_nodes'], 3, d=8, seed=99, stub=True)
    items = torch.arange(1, 20, device=dev())
    snap = C.embed_catalogue(items, 10.0)
    q, t = torch.arange(1, 6, device=dev()), torch.full((5,), 10.0, dtype=torch.float64, device=dev())
    C.recommend(q, t, snap, 3)
    C.load_online(copy_of(saved))
    with pytest.raises(RuntimeError, match='stale'):
        C.recommend(q, t, snap, 3)
    C.recommend(q, torch.full((5,), 6000.0, dtype=torch.float64, device=dev()), C.embed_catalogue(items, 6000.0), 3)


def test_the_online_example_saved_and_loaded_writes_the_lists_of_the_uninterrupted_replay(tmp_path):
    """examples/recommend.run_online on toy JODIE files with an 8-wide edge table, forgetting and releasing rows on the way: a replay saved after two
    batches and one that starts from the file give, between them, the lists of the replay that was never interrupted"""
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
    z['efeats'][0] = 0
    z['nfeats'] = np.zeros((int(max(z['src'].max(), z['dst'].max())) + 1, 8), dtype=np.float32)
    write_files(str(tmp_path), 'toy', z)
    ckpt, path = str(tmp_path / 'model.pt'), str(tmp_path / 'served.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    on = dict(k=5, keep_last=6, release_rows=True, verbose=False, offline=False, **kw)
    whole, _ = rc.run_online('toy', str(tmp_path), ckpt, save_state=str(tmp_path / 'end.pt'), **on)
    head, _ = rc.run_online('toy', str(tmp_path), ckpt, save_state=path, save_after=2, **on)
    tail, _ = rc.run_online('toy', str(tmp_path), ckpt, load_state=path, **on)
    assert head['n_events'] == 200 and tail['n_events'] == whole['n_events'] - 200 > 0
    assert sum(b - a for b, a in head['rows']) > 0   # rows were released before the save: the eids are renumbered
    np.testing.assert_array_equal(np.concatenate([head['ids'], tail['ids']]), whole['ids'])
    assert head['forgot'] + tail['forgot'] == whole['forgot'] and head['rows'] + tail['rows'] == whole['rows']
