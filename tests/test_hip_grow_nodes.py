"""TIGE.grow_nodes / TIGE.observe(num_node=) on the GPU - the acceptance property of online node admission: a model built on
N0 nodes that observes a stream and admits ids up to N1 on the way ends in the state, and returns the embeddings, of a twin
with equal weights that was built on N1 nodes with the full graph from the start.  Everything is compared with torch.equal.
The stream is bench.make_stream's (d = 8, K = 5, 240 events) with the ids renumbered in the order of their first appearance,
so that every batch of the tail brings ids nobody has seen; two twins are compared, so no recorded fixture is needed."""
import numpy as np
import pytest
import torch

from test_hip_rank import dev

pytestmark = pytest.mark.gpu

D, K, E, E0 = 8, 5, 240, 40
BATCHES = [(40, 100), (100, 104), (104, 105), (105, 180), (180, 240)]   # ragged; two bring no new id, (180, 240) admits within the capacity
KEYS = ('src', 'dst', 'ts', 'eids')


def make_stream():
    """ids in the order of their first appearance (0 stays the padding id) -> stream dict, nfeats [N1, D]; N1 leaves ONE id
    beyond the stream's: the brand-new node of the tests below"""
    import bench
    st = bench.make_stream(60, 15, E, 5000.0, seed=0, d_e=D, with_efeats=True)
    both = np.stack([st['src'], st['dst']], 1).reshape(-1)
    _, first = np.unique(both, return_index=True)
    order = both[np.sort(first)]
    new_id = np.zeros(st['n_nodes'], dtype=np.int64)
    new_id[order] = np.arange(1, len(order) + 1)
    st = dict(st, src=new_id[st['src']], dst=new_id[st['dst']])
    st['n_stream'] = len(order) + 1
    st['n_nodes'] = st['n_stream'] + 1
    nf = (np.random.RandomState(1).standard_normal((st['n_nodes'], D)) * 0.3).astype(np.float32)
    nf[0] = 0
    return st, nf


def ids_upto(st, hi):
    return int(max(st['src'][:hi].max(), st['dst'][:hi].max())) + 1


def test_the_stream_has_what_the_tests_need():
    st, _ = make_stream()
    seen = ids_upto(st, E0)
    assert seen < ids_upto(st, E) == st['n_stream']
    twice = False
    for lo, hi in BATCHES:
        now = ids_upto(st, hi)
        assert (now > seen) == ((lo, hi) not in ((100, 104), (104, 105)))   # three batches admit ids, two do not
        ids = np.concatenate([st['src'][lo:hi], st['dst'][lo:hi]])
        twice |= bool((np.bincount(ids[ids >= seen], minlength=now) >= 2).any())
        seen = now
    assert twice   # an id nobody has seen appears twice in the batch that admits it


def build(st, nf, n_nodes, n_events, *, strategy='recent_edges', L=1, forms=()):
    """as tests/test_hip_rank.py::build on `n_nodes` ids and the first n_events events, with the sequence restarter (a
    static restarter's per-node parameters do not grow); every initialiser is seeded, so equal calls give equal weights"""
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    from www2023tiger_amd.model.restarters import SeqRestarter
    from www2023tiger_amd.model.tiger import TIGER
    g = Graph.from_arrays(*(st[k][:n_events] for k in KEYS), strategy=strategy, seed=0, max_node_id=n_nodes - 1, device=dev())
    torch.manual_seed(0)
    fg = NumericalFeature(torch.from_numpy(nf[:n_nodes].copy()), torch.from_numpy(st['efeats']), dim=D, device=dev())
    fg.n_nodes, fg.n_edges = n_nodes, E
    rst = SeqRestarter(raw_feat_getter=fg, graph=g, hist_len=7, n_head=2, dropout=0.0)
    model = TIGER(raw_feat_getter=fg, graph=g, restarter=rst, n_neighbors=K, hit_type='bin', n_layers=L, n_head=2,
                  dropout=0.0, msg_src='left', upd_src='right').to(dev())
    with torch.no_grad():
        model.time_encoder.phase.uniform_(-0.5, 0.5)
        model.hit_embedding.weight.normal_(0, 0.5)
    model.eval()
    if 'fused' in forms:
        model.fuse_attention()
    if 'eager' in forms:
        model.eager_updates()
    return model


def twins(zero_new_nfeats=False, **kw):
    """A: born with N1 ids and the full graph.  B: born with the ids and the graph of the first E0 events.  Equal weights;
    both have streamed the events [0, E0)."""
    st, nf = make_stream()
    N0 = ids_upto(st, E0)
    if zero_new_nfeats:
        nf[N0:] = 0
    A, B = build(st, nf, st['n_nodes'], E, **kw), build(st, nf, N0, E0, **kw)
    pa, pb = dict(A.named_parameters()), dict(B.named_parameters())
    assert pa.keys() == pb.keys() and all(torch.equal(pa[k], pb[k]) for k in pa)
    for m in (A, B):
        m.stream_step(*batch(st, 0, E0))
    assert_same_state(A, B)
    return A, B, st, nf


def batch(st, lo, hi):
    return [st[k][lo:hi] for k in ('src', 'dst', 'dst', 'ts', 'eids')]   # the negatives are the destinations


def state_of(m):
    L, R, S = m.left_memory, m.right_memory, m.msg_store
    return dict(left_vals=L.vals, left_ts=L.update_ts, left_active=L.active_mask, right_vals=R.vals, right_ts=R.update_ts,
                right_active=R.active_mask, msg_vals=S.node_msg_vals, msg_ts=S.node_msg_ts, has_msg=S.has_msg_bits)


def assert_same_state(A, B):
    """B's rows against A's leading rows, and nothing in A's further rows: A was born with ids B has yet to admit"""
    a, b = state_of(A), state_of(B)
    n = B.n_nodes
    assert all(t.shape[0] == n for k, t in b.items() if k != 'has_msg')
    for k in a:
        if k == 'has_msg':
            w = b[k].numel()
            assert torch.equal(a[k][:w], b[k]) and not bool(a[k][w:].any()), k
        else:
            assert torch.equal(a[k][:n], b[k]), k
            assert not bool(a[k][n:].any()), k + ': the twin holds state for an id nobody has seen'


def pointers(m):
    return tuple(t.data_ptr() for t in state_of(m).values()) + (m.raw_feat_getter.nfeats.data_ptr(),)


def assert_spare_bits_zero(m):
    """the bits at and beyond n_nodes in the last word of the bitmap the ENGINE wrote: a growth hands them to new ids"""
    bits = m.msg_store.has_msg_bits
    assert bool(bits.any())   # (messages are pending: the bitmap is not trivially empty)
    used = m.n_nodes - 64 * (bits.numel() - 1)
    assert 0 < used <= 64
    last = int(bits[-1]) & ((1 << 64) - 1)
    assert last >> used == 0, f'bits beyond node {m.n_nodes - 1} are set: {last:#018x}'


def capacity(m):
    stores = getattr(m.left_memory, '_stores', None)
    return stores['vals'].shape[0] if stores else m.n_nodes


def feed(A, B, st, nf, lo, hi, **kw):
    """one batch through both -> whether B's tables moved; embeddings and state compared"""
    a = A.stream_step(*batch(st, lo, hi))
    ha = a.h[:3 * (hi - lo)].clone()
    n_old, n_new = B.n_nodes, max(B.n_nodes, ids_upto(st, hi))
    cap, before = capacity(B), pointers(B)
    assert_spare_bits_zero(B)
    src, dst, neg, ts, eids = batch(st, lo, hi)
    kw.setdefault('nfeats', nf[n_old:n_new])
    b = B.observe(src, dst, ts, eids, num_node='auto', **kw)
    assert torch.equal(b.h[:3 * (hi - lo)], ha), f'h of batch [{lo}, {hi})'
    assert B.n_nodes == n_new == B.graph.num_node == B.restarter_fn.n_nodes == B.raw_feat_getter.n_nodes
    assert B.restarter_fn.graph is B.graph
    assert_same_state(A, B)
    moved = pointers(B) != before
    assert moved == (n_new > cap), f'batch [{lo}, {hi}): {n_old} -> {n_new} ids on a capacity of {cap}'
    if not moved:
        assert pointers(B) == before   # every pointer, not just one
    return moved, n_new > n_old


VARIANTS = {'plain': {}, 'recent_nodes': dict(strategy='recent_nodes'), 'two-layers': dict(L=2),
            'fused+eager': dict(forms=('fused', 'eager'))}


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_admitting_ids_on_the_way_equals_having_been_born_with_them(variant):
    A, B, st, nf = twins(**VARIANTS[variant])
    g0, n0 = B.graph, B.n_nodes
    seen = set()
    for lo, hi in BATCHES:
        parent = B.graph
        seen.add(feed(A, B, st, nf, lo, hi))
        assert parent.num_node <= B.graph.num_node and parent.tcsr.num_entry == 2 * lo   # the parent is what it was
    # a growth that reallocated, one that stayed within the capacity (same data pointers), a batch without new ids
    assert {(True, True), (False, True), (False, False)} <= seen
    assert g0.num_node == n0 and g0.tcsr.num_entry == 2 * E0
    assert B.n_nodes == st['n_stream'] and torch.equal(B.raw_feat_getter.nfeats, A.raw_feat_getter.nfeats[:B.n_nodes])
    # the one id left: no events, admitted by hand - then the two are the same model
    assert B.grow_nodes(st['n_nodes'], nfeats=nf[-1:]) in (True, False)
    assert B.n_nodes == A.n_nodes == B.graph.num_node
    for a, b in zip(A.graph._tensors(), B.graph._tensors()):
        assert torch.equal(a, b)
    for k, v in state_of(A).items():
        assert torch.equal(v, state_of(B)[k]), k


def test_reserve_sizes_every_store_the_node_table_included():
    A, B, st, nf = twins()
    n = B.n_nodes
    assert B.grow_nodes(n + 1, reserve=n + 1) is True
    for i in (2, 3):   # stores without head-room: every table moves again, the feature table too
        before = pointers(B)
        assert B.grow_nodes(n + i, reserve=n + i) is True
        assert all(a != b for a, b in zip(pointers(B), before))
        assert B.raw_feat_getter._stores['nfeats'].shape[0] == B.left_memory._stores['vals'].shape[0] == n + i
    assert B.grow_nodes(n + 4, reserve=n + 40) is True and B.grow_nodes(n + 40) is False
    assert B.raw_feat_getter._stores['nfeats'].shape[0] == n + 40 and B.n_nodes == n + 40


def test_a_memory_state_saved_before_a_growth_is_refused_until_it_was_grown():
    A, B, st, nf = twins()
    saved = B.save_memory_state()
    lo, hi = BATCHES[0]
    feed(A, B, st, nf, lo, hi)
    now = {k: v.clone() for k, v in state_of(B).items()}
    with pytest.raises(ValueError, match='rows'):
        B.load_memory_state(saved)
    assert all(torch.equal(v, now[k]) for k, v in state_of(B).items()) and B.left_memory is not saved[0]
    for mod in saved:
        mod.grow(B.n_nodes)
    B.load_memory_state(saved)
    assert B.left_memory is saved[0] and B.left_memory.vals.shape[0] == B.n_nodes == B.msg_store.n
    lo, hi = BATCHES[1]
    B.observe(*[batch(st, lo, hi)[i] for i in (0, 1, 3, 4)])   # and the model runs on it


def test_omitted_feature_rows_are_zeros():
    A, B, st, nf = twins(zero_new_nfeats=True)
    for lo, hi in BATCHES[:2]:
        feed(A, B, st, nf, lo, hi, nfeats=None)
    assert not bool(B.raw_feat_getter.nfeats[ids_upto(st, E0):].any())


def test_the_sequence_restarter_restarts_admitted_nodes():
    A, B, st, nf = twins()
    top = 0
    for lo, hi in BATCHES[:4]:
        feed(A, B, st, nf, lo, hi)
        nodes = torch.unique(torch.from_numpy(np.concatenate([st['src'][lo:hi], st['dst'][lo:hi]]))).to(dev())
        top = max(top, int(nodes.max()))
        t = torch.full((nodes.numel(),), float(st['ts'][hi - 1]), device=dev())
        A.restart(nodes, t)
        B.restart(nodes, t)
        assert_same_state(A, B)
    assert top >= ids_upto(st, BATCHES[2][1])   # ids the model was not born with were restarted


def same(got, want):
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_recommend_lists_and_filters_a_new_item_only_after_the_growth():
    A, B, st, nf = twins()
    lo, hi = BATCHES[0]
    n_old = B.n_nodes
    e = lo + int(np.argmax(st['dst'][lo:hi] >= n_old))        # the first event whose destination nobody has seen
    item, user = int(st['dst'][e]), int(st['src'][e])
    assert item >= n_old
    other = int(next(u for u in st['src'][:E0] if u != user and not np.any((st['src'][:hi] == u) & (st['dst'][:hi] == item))))
    q = torch.tensor([user, other], device=dev())
    t = torch.full((2,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    cand = torch.tensor([item] + sorted(set(st['dst'][:E0].tolist()))[:6], device=dev())
    with pytest.raises(ValueError, match='outside'):
        B.recommend(q, t, cand, 3, exclude_seen=True)
    feed(A, B, st, nf, lo, hi)
    got, want = B.recommend(q, t, cand, len(cand), exclude_seen=True), A.recommend(q, t, cand, len(cand), exclude_seen=True)
    same(got, want)
    ids, _, n_valid = got
    assert item not in ids[0, :int(n_valid[0])].tolist()      # filtered for the user who has seen it
    assert item in ids[1, :int(n_valid[1])].tolist()          # listed for one who has not
    same(B.rank_scores(q, q, t, cand), A.rank_scores(q, q, t, cand))


def test_a_brand_new_source_gets_a_full_row_from_the_walk_with_back_fill():
    A, B, st, nf = twins()
    for lo, hi in BATCHES:
        feed(A, B, st, nf, lo, hi)
    newcomer = st['n_nodes'] - 1                               # no event names it
    q = torch.tensor([newcomer, int(st['src'][0])], device=dev())
    t = torch.full((2,), float(st['ts'][-1]) + 1.0, dtype=torch.float64, device=dev())
    with pytest.raises(ValueError):
        B.recommend_walk(q, t, 5, C=12, fill=dict(T=8))
    B.grow_nodes(st['n_nodes'], nfeats=nf[-1:])
    got, want = B.recommend_walk(q, t, 5, C=12, fill=dict(T=8)), A.recommend_walk(q, t, 5, C=12, fill=dict(T=8))
    same(got[:3], want[:3])
    assert int(got[2][0]) >= 5 and bool((got[0][0] > 0).all()) and int(got[3]['n_filled'][0]) > 0   # a full row of back-fill


def test_a_checkpoint_after_growth_loads_into_a_model_born_big(tmp_path):
    A, B, st, nf = twins()
    for lo, hi in BATCHES[:2]:
        feed(A, B, st, nf, lo, hi)
    B.grow_nodes(st['n_nodes'], nfeats=nf[B.n_nodes:])
    torch.save(B.state_dict(), tmp_path / 'grown.pt')
    fresh = build(st, nf, st['n_nodes'], E)
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    fresh.load_state_dict(torch.load(tmp_path / 'grown.pt'))
    sa, sf = A.state_dict(), fresh.state_dict()
    assert sa.keys() == sf.keys()
    for k in sa:
        assert sa[k].shape == sf[k].shape and torch.equal(sa[k], sf[k]), k


def test_a_snapshot_from_before_the_growth_is_stale_and_its_index_is_padded():
    A, B, st, nf = twins()
    lo, hi = BATCHES[0]
    items = torch.tensor(sorted(set(st['dst'][:E0].tolist())), device=dev())
    t_snap = float(st['ts'][E0 - 1]) + 0.5
    snap = B.embed_catalogue(items, t_snap)
    n_old = B.n_nodes
    feed(A, B, st, nf, lo, hi)
    q = torch.from_numpy(st['src'][lo:lo + 4]).to(dev())
    t = torch.full((4,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    with pytest.raises(RuntimeError, match='stale'):           # today's text, not a count mismatch
        B.recommend(q, t, snap, 3)
    ids, _, n_valid = B.recommend(q, t, snap, 3, stale_ok=True, exclude_seen=True)
    assert snap.col_of.numel() == B.n_nodes and bool((snap.col_of[n_old:] == -1).all())
    assert bool((n_valid > 0).all()) and bool(torch.isin(ids[:, 0], items).all())


def test_uptodate_bitmaps_are_grown_or_refused_by_name():
    from www2023tiger_amd import hip_ops
    A, B, st, nf = twins()
    bm = hip_ops.new_bitmap(B.n_nodes, dev())
    B.grow_nodes(B.n_nodes + 200)
    nodes = torch.from_numpy(st['src'][:8]).to(dev())
    t = torch.full((8,), float(st['ts'][E0 - 1]) + 1.0, dtype=torch.float64, device=dev())
    with pytest.raises(ValueError, match='bitmap_grown'):
        B.restart_involved(nodes, t, bm)
    with pytest.raises(ValueError, match='bitmap_grown'):
        B.recommend(nodes, t, nodes, 3, uptodate=bm)
    bm = hip_ops.bitmap_grown(bm, B.n_nodes)
    assert B.restart_involved(nodes, t, bm) > 0


def test_every_refusal_leaves_the_model_as_it_was(monkeypatch):
    from www2023tiger_amd.model.restarters import StaticRestarter
    A, B, st, nf = twins()
    lo, hi = BATCHES[0]
    src, dst, _, ts, eids = batch(st, lo, hi)
    n_new = ids_upto(st, hi)
    rows = nf[B.n_nodes:n_new]
    n0, g0, p0, fg = B.n_nodes, B.graph, pointers(B), B.raw_feat_getter
    s0 = {k: v.clone() for k, v in state_of(B).items()}

    def untouched():
        assert B.n_nodes == n0 == fg.n_nodes == B.restarter_fn.n_nodes and B.graph is g0 and pointers(B) == p0
        assert all(torch.equal(v, s0[k]) for k, v in state_of(B).items())

    def both(exc, match, restore=None):
        with pytest.raises(exc, match=match):
            B.observe(src, dst, ts, eids, num_node='auto', nfeats=rows)
        with pytest.raises(exc, match=match):
            B.grow_nodes(n_new, nfeats=rows)
        if restore is not None:
            restore()
        untouched()
    with pytest.raises(ValueError, match='does not grow'):    # without the argument: as ever
        B.observe(src, dst, ts, eids)
    with pytest.raises(ValueError, match='num_node'):
        B.observe(src, dst, ts, eids, nfeats=rows)
    untouched()
    B.train()
    both(RuntimeError, 'eval')
    B.eval()
    B._row_of = torch.zeros(B.n_nodes, dtype=torch.int32, device=dev())
    both(RuntimeError, 'partitioned')
    B._row_of = None
    seq = B.restarter_fn
    B.restarter_fn = StaticRestarter(raw_feat_getter=fg, graph=B.graph).to(dev())
    both(NotImplementedError, 'static restarter')
    B.restarter_fn = seq
    fg.pin_mem = False
    both(NotImplementedError, 'pinned')
    fg.pin_mem = True
    table, fg.nfeats = fg.nfeats, None
    both(NotImplementedError, 'no node table', restore=lambda: setattr(fg, 'nfeats', table))
    assert fg.nfeats is table
    with pytest.raises(ValueError, match='nfeats'):
        B.observe(src, dst, ts, eids, num_node='auto', nfeats=rows[:-1])
    with pytest.raises(ValueError, match='nfeats'):
        B.grow_nodes(n_new, nfeats=rows[:, :-1])
    with pytest.raises(ValueError, match='below'):
        B.grow_nodes(n0 - 1)
    with pytest.raises(ValueError, match='reserve'):
        B.grow_nodes(n_new, reserve=n_new - 1)
    with pytest.raises(ValueError, match='node ids must lie'):   # an id at the count the caller names
        B.observe(src, dst, ts, eids, num_node=n_new - 1, nfeats=rows[:-1])
    with pytest.raises(ValueError, match='before the latest event'):
        B.observe(src, dst, ts - 1e6, eids, num_node='auto', nfeats=rows)
    untouched()
    # (the capture check alone: a stream that IS capturing is refused - no graph is captured for it here)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    both(RuntimeError, 'captured')
    monkeypatch.undo()
    untouched()
    assert B.grow_nodes(n0) is False                           # nothing to admit: nothing happens
    untouched()
    feed(A, B, st, nf, lo, hi)                                 # and the model still follows its twin


def test_the_online_example_admits_the_ids_of_the_test_split(tmp_path):
    """examples/recommend.run_online(grow=True) on toy JODIE files: the model starts with the ids of train + validation,
    ends with those of the whole stream and the ids admitted per batch add up"""
    import os
    import sys
    from _util import load
    from test_input_side import write_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'examples'))
    import link_prediction as lp
    import recommend as rc
    z0 = load('input_side')
    z = {k: z0[k].copy() for k in ('src', 'dst', 'ts')}
    top = int(max(z['src'].max(), z['dst'].max()))
    late = np.arange(len(z['src']) - 250, len(z['src']))       # newcomers in the tail: 7 items and 3 users nobody has seen
    z['dst'][late[::10]] = top + 1 + np.arange(len(late[::10])) % 7
    z['src'][late[5::17]] = top + 8 + np.arange(len(late[5::17])) % 3
    z['labels'] = np.zeros(len(z['src']), dtype=np.int64)
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    grown, none = rc.run_online('toy', str(tmp_path), ckpt, k=5, grow=True, verbose=False, **kw)
    assert none is None and grown['n_events'] > 0
    n_test = grown['n_events']
    n_all = int(max(z['src'].max(), z['dst'].max())) + 1
    n_seen = int(max(z['src'][:-n_test].max(), z['dst'][:-n_test].max())) + 1
    assert len(grown['admitted']) == -(-n_test // 100) and sum(grown['admitted']) == n_all - n_seen == 10
