"""Lazy restarts for ranking and recommendation candidates on the GPU: TIGER.restart_involved, the `uptodate` forms of
rank_scores / recommend and the `lazy_restarts` forms of eval_edge_ranking / eval_recommendation, each against a twin model
that does the same the long way round from public pieces.  On build() of tests/test_hip_rank.py (d = 16, K = 10), with its
static restarter or the SeqRestarter of tests/test_hip_observe.py, one and two layers.  Counts, bitmaps, ranks and state:
bit for bit; scores of the operator path against one-call scores: TOL of tests/test_hip_rank.py."""
import numpy as np
import pytest
import torch

import _involved_ref as R
from _rank_ref import numpy_ranks
from _util import assert_close
from test_hip_observe import install_seq_restarter
from test_hip_rank import KS, TOL, WARM, assert_same_state, batch, build, dev, state_of, warm

pytestmark = pytest.mark.gpu
D, K = 16, 10
MODELS = [(1, False), (1, True), (2, False), (2, True)]
MODEL_IDS = ['L1-static', 'L1-seq', 'L2-static', 'L2-seq']


def t(x, dt=torch.int64):
    return torch.as_tensor(x).to(dev(), dt)


def twins(n, L, seq, *, warmed=True, forms=(), **kw):
    """n models with equal weights and equal state [, a few ragged stream batches in]"""
    built = [build(D, D, K, 'bin', L=L, **kw) for _ in range(n)]
    st = built[0][2]
    for m, orc, _ in built:
        if seq:
            install_seq_restarter(m)
        if 'fused' in forms:
            m.fuse_attention()
        if 'eager' in forms:
            m.eager_updates()
        if warmed:
            warm(m, orc, st, K, with_oracle=False)
    return [b[0] for b in built], st


def loader(model, st, L, bs=50):
    """tests/test_hip_rank.py::loader with the collator's layer count following the model's"""
    from www2023tiger_amd.data.data_loader import BatchLoader, GraphCollator, InteractionData
    E = len(st['src'])
    data = InteractionData(st['src'], st['dst'], st['ts'], st['eids'], np.zeros(E, dtype=np.int64), seed=0, eval=True,
                           neg_dst=st['neg'])
    return BatchLoader(data, bs, GraphCollator(model.graph, K, L, restarter='static'))


def ranked_batch(st, B, C, seed=4):
    lo = WARM[-1]
    src, dst, _, ts, _ = batch(st, lo, lo + B)
    cand = np.random.RandomState(seed).randint(0, st['n_nodes'], (B, C)).astype(np.int64)
    return src, dst, ts, cand


def flat_queries(src, dst, ts, cand):
    """the flat list rank_scores embeds: sources, then [dst | cand] row by row, each at its event's time"""
    ids_all = np.concatenate([dst[:, None], cand], 1)
    return np.concatenate([src, ids_all.ravel()]), np.concatenate([ts, np.repeat(ts, ids_all.shape[1])])


def bitmap_ids(bm, n_nodes):
    return set(np.nonzero(R.from_bitmap(bm.cpu().numpy(), n_nodes))[0].tolist())


def long_way(model, nodes, ts, uptodate: set, L):
    """restart_involved from public pieces: the collator's involved set, a Python set difference on the host, restart_list"""
    from www2023tiger_amd.data.data_loader import GraphCollator
    _, _, comp = GraphCollator(model.graph, K, L).collate_memory_nodes(t(nodes), t(ts, torch.float64))
    involved = set(comp['ids'][:int(comp['count'].item())].cpu().tolist())
    todo = sorted(involved - uptodate)
    if todo:
        model.restart_list(t(todo), torch.tensor([np.float32(ts.min())], dtype=torch.float32, device=dev()))
    uptodate |= involved
    return len(todo)


# ------------------------------------------------------------------------------------------ restart_involved
@pytest.mark.parametrize('L,seq', MODELS, ids=MODEL_IDS)
def test_restart_involved_equals_the_long_way(L, seq):
    from www2023tiger_amd import hip_ops
    (A, B), st = twins(2, L, seq)
    n_nodes = st['n_nodes']
    nodes, ts = flat_queries(*ranked_batch(st, 9, 5))
    start = set(np.nonzero(np.random.RandomState(1).rand(n_nodes) < 0.3)[0].tolist())
    bm = hip_ops.new_bitmap(n_nodes, dev())
    hip_ops.bitmap_mark(t(sorted(start)), bm, n_nodes)
    before = state_of(A)
    n = A.restart_involved(t(nodes), t(ts, torch.float64), bm)
    upto = set(start)
    assert n == long_way(B, nodes, ts, upto, L) and n > 0 and A.last_restarted == n
    assert bitmap_ids(bm, n_nodes) == upto
    assert_same_state(state_of(A), state_of(B))
    assert not torch.equal(before['left_vals'], A.left_memory.vals)
    # the reference's set, and a second call that finds everybody up to date
    og = R.oracle_graph(dict(st, n_nodes=n_nodes), 'recent_edges')
    assert upto - start == set(R.numpy_involved(og, nodes, ts, K, L, 'recent_edges').tolist()) - start
    after = state_of(A)
    assert A.restart_involved(t(nodes), t(ts, torch.float64), bm) == 0
    assert_same_state(after, state_of(A))


@pytest.mark.parametrize('L,seq', MODELS, ids=MODEL_IDS)
def test_rank_scores_with_a_bitmap_is_restart_involved_then_rank_scores(L, seq):
    from www2023tiger_amd import hip_ops
    (A, B), st = twins(2, L, seq)
    src, dst, ts, cand = ranked_batch(st, 9, 5)
    bm_a, bm_b = (hip_ops.new_bitmap(st['n_nodes'], dev()) for _ in range(2))
    got = A.rank_scores(t(src), t(dst), t(ts, torch.float64), t(cand), uptodate=bm_a)
    nodes, times = flat_queries(src, dst, ts, cand)
    assert B.restart_involved(t(nodes), t(times, torch.float64), bm_b) == A.last_restarted > 0
    want = B.rank_scores(t(src), t(dst), t(ts, torch.float64), t(cand))
    assert torch.equal(got, want) and torch.equal(bm_a, bm_b)
    assert_same_state(state_of(A), state_of(B))


CHUNK_STREAM = dict(n_u=300)   # 300 users over 200 events: most nodes stay out of a call's involved set


def chunk_case(st, L):
    """B = 21 events (every fourth behind the warm-up: the call spans 80 events), C = 5 candidates from a pool of four items:
    chunk_queries = 7 (C + 2) scores seven events per chunk, three chunks.  The last candidate of the last event is a node X
    that nothing else involves - it comes in through that candidate alone, in the last chunk alone - and that has an event
    between the earliest time of the whole call and the earliest time of the last chunk.  A restart depends on its time
    through the history before it only, so this is the node a restart per chunk gets wrong: one restart over all queries
    gives X the state of the call's earliest time, a restart per chunk the state of the last chunk's, which has seen that
    event.  (Where the stream has one, X also has an edge with a query node of the first chunk.)"""
    B, C = 21, 5
    rows = WARM[-1] + 4 * np.arange(B)
    src, dst, ts = st['src'][rows], st['dst'][rows], st['ts'][rows]
    cand = dst[np.random.RandomState(4).randint(0, 4, (B, C))]
    og = R.oracle_graph(dict(st, n_nodes=st['n_nodes']), 'recent_edges')
    involved = lambda lo, hi: set(R.numpy_involved(og, *flat_queries(src[lo:hi], dst[lo:hi], ts[lo:hi], cand[lo:hi]), K, L,
                                                   'recent_edges').tolist())
    others = involved(0, B)
    first = set(flat_queries(src[:7], dst[:7], ts[:7], cand[:7])[0].tolist())
    t_all, t_last = ts.min(), ts[14:].min()
    assert t_all < t_last
    found = []
    for x in range(1, st['n_nodes']):
        mine = (st['src'] == x) | (st['dst'] == x)
        if x not in others and (mine & (st['ts'] >= t_all) & (st['ts'] < t_last)).any():
            partners = set(st['src'][mine].tolist()) | set(st['dst'][mine].tolist())
            found.append((not partners & first, x))
    assert found, 'no node would come in through the last candidate alone'
    x = min(found)[1]
    cand[-1, -1] = x
    assert x in involved(14, B) and x not in involved(0, 14) and x in involved(0, B)
    return src, dst, ts, cand


@pytest.mark.parametrize('L,seq', [(1, True), (2, False)], ids=['L1-seq', 'L2-static'])
def test_scores_do_not_depend_on_the_chunking(L, seq):
    from www2023tiger_amd import hip_ops
    (A, B), st = twins(2, L, seq, **CHUNK_STREAM)
    src, dst, ts, cand = chunk_case(st, L)
    C = cand.shape[1]
    bm_a, bm_b = (hip_ops.new_bitmap(st['n_nodes'], dev()) for _ in range(2))
    a = A.rank_scores(t(src), t(dst), t(ts, torch.float64), t(cand), uptodate=bm_a, chunk_queries=7 * (C + 2))
    b = B.rank_scores(t(src), t(dst), t(ts, torch.float64), t(cand), uptodate=bm_b)
    assert torch.equal(a, b) and torch.equal(bm_a, bm_b) and A.last_restarted == B.last_restarted > 0
    assert_same_state(state_of(A), state_of(B))


# ------------------------------------------------------------------------------------------ evaluation loops
def record(model, name, store):
    """keep what model.<name> returns, call by call"""
    inner = getattr(model, name)

    def wrapped(*a, **kw):
        out = inner(*a, **kw)
        keep = lambda x: x.clone() if torch.is_tensor(x) else x   # (a step may hand out views of buffers it reuses)
        store.append(tuple(keep(x) for x in out) if isinstance(out, tuple) else keep(out))
        return out
    setattr(model, name, wrapped)


@pytest.mark.parametrize('L', [1, 2])
def test_eval_edge_ranking_with_the_loader_negatives_is_restart_mode_edge_prediction(L, monkeypatch):
    """candidates = the loader's own negatives: the candidate queries are the batch's own, so the lazy restarts are those of
    eval_edge_prediction(restart_mode=True) - same final state and up-to-date set, bit for bit against its per-batch loop -
    and columns 0 / 1 are its positive / negative scores (operator path against the one-call step: TOL)"""
    from www2023tiger_amd.eval_utils import eval_edge_prediction, eval_edge_ranking
    monkeypatch.setenv('TG_EVAL_RESIDENT', '0')
    (A, B), st = twins(2, L, False, warmed=False)
    start = {1, 2, 3, 61, 70}
    set_a, set_b = set(start), set(start)
    ranked, stepped = [], []
    record(A, 'rank_scores', ranked)
    record(B, 'contrast_learning', stepped)
    out = eval_edge_ranking(A, loader(A, st, L), dev(), st['neg'][:, None], ks=KS, lazy_restarts=True, uptodate_nodes=set_a)
    eval_edge_prediction(B, loader(B, st, L), dev(), True, set_b)
    assert out['n_events'] == len(st['src']) and len(ranked) == len(stepped) == 4
    assert set_a == set_b and len(set_a) > len(start)
    assert_same_state(state_of(A), state_of(B))
    got = torch.cat(ranked).cpu().numpy()
    assert_close(got[:, 0], torch.cat([s[2] for s in stepped]).cpu().numpy(), 'positive scores', TOL)
    assert_close(got[:, 1], torch.cat([s[3] for s in stepped]).cpu().numpy(), 'negative scores', TOL)


def lazy_twin_loop(model, st, L, cand_rows, bm, per_batch):
    """the lazy-restart evaluation loop from public pieces: per batch ONE restart_involved over cat[src, dst, neg] plus the
    candidate queries, then per_batch(src, dst, ts64, lo) on the restarted state, then the batch itself"""
    lo, counts = 0, []
    with torch.no_grad():
        for src, dst, neg, ts, eids, _, cg in loader(model, st, L):
            src, dst, neg, ts, eids = (x.to(dev()) for x in (src, dst, neg, ts, eids))
            n = len(src)
            c = cand_rows(lo, n)
            nodes = torch.cat([src, dst, neg, c.reshape(-1)])
            times = torch.cat([cg.ts64.repeat(3), cg.ts64.repeat_interleave(c.shape[1])])
            counts.append(model.restart_involved(nodes, times, bm, graph=model.graph))
            per_batch(src, dst, cg.ts64, lo, c)
            model.contrast_learning(src, dst, neg, ts, eids, cg)
            lo += n
    return counts


@pytest.mark.parametrize('L,seq', [(1, True), (2, False)], ids=['L1-seq', 'L2-static'])
def test_eval_edge_ranking_lazy_restarts_end_to_end(L, seq):
    """200 events at batch 50 with 11 random candidates against the twin loop: ranks exactly, MRR / Hits to 1e-12, state
    and up-to-date set equal"""
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.eval_utils import eval_edge_ranking
    (A, B), st = twins(2, L, seq, warmed=False)
    E, C = len(st['src']), 11
    cand = np.random.RandomState(9).randint(0, st['n_nodes'], (E, C)).astype(np.int64)
    cand[::7, 0] = st['dst'][::7]
    set_a = {4, 5, 66}
    bm = hip_ops.new_bitmap(st['n_nodes'], dev())
    hip_ops.bitmap_mark(t(sorted(set_a)), bm, st['n_nodes'])
    out = eval_edge_ranking(A, loader(A, st, L), dev(), cand, ks=KS, lazy_restarts=True, uptodate_nodes=set_a,
                            return_ranks=True)
    ranks = []

    def per_batch(src, dst, ts64, lo, c):
        s = B.rank_scores(src, dst, ts64, c).cpu().numpy()
        ids = np.concatenate([dst.cpu().numpy()[:, None], c.cpu().numpy()], 1)
        ranks.append(numpy_ranks(s, ids, dst.cpu().numpy())[3])

    counts = lazy_twin_loop(B, st, L, lambda lo, n: t(cand[lo:lo + n]), bm, per_batch)
    r = np.concatenate(ranks)
    np.testing.assert_array_equal(out['ranks'].cpu().numpy(), r)
    assert abs(out['mrr'] - float(np.mean(1.0 / r))) < 1e-12
    for k in KS:
        assert abs(out['hits'][k] - float(np.mean(r <= k))) < 1e-12
    assert counts[0] > 0 and sum(counts) + 3 == len(set_a) == len(bitmap_ids(bm, st['n_nodes']))
    assert set_a == bitmap_ids(bm, st['n_nodes'])
    assert_same_state(state_of(A), state_of(B))


@pytest.mark.parametrize('L,seq', [(1, True), (2, False)], ids=['L1-seq', 'L2-static'])
def test_eval_recommendation_lazy_restarts_end_to_end(L, seq):
    """the same for the positions of eval_recommendation: a 40-id catalogue, exclude_seen=True"""
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.eval_utils import eval_recommendation
    (A, B), st = twins(2, L, seq, warmed=False)
    n_nodes, k = st['n_nodes'], 10
    cat = np.random.RandomState(2).permutation(np.arange(1, n_nodes))[:40].astype(np.int64)
    set_a = set()
    bm = hip_ops.new_bitmap(n_nodes, dev())
    out = eval_recommendation(A, loader(A, st, L), dev(), cat, k=k, exclude_seen=True, lazy_restarts=True,
                              uptodate_nodes=set_a, return_positions=True)
    col_of = hip_ops.catalogue_index(t(cat), n_nodes)
    positions = []

    def per_batch(src, dst, ts64, lo, c):
        seen = hip_ops.seen_mask(B.graph, src, ts64, col_of, len(cat))
        ids, _, _ = B.recommend(src, ts64, t(cat), k, mask=seen)
        hit = (ids == dst[:, None]) & (ids != 0)
        positions.append(torch.where(hit.any(1), hit.float().argmax(1), -1).cpu().numpy())

    lazy_twin_loop(B, st, L, lambda lo, n: t(cat).unsqueeze(0).expand(n, -1), bm, per_batch)
    pos = np.concatenate(positions)
    np.testing.assert_array_equal(out['positions'].cpu().numpy(), pos)
    hit = pos >= 0
    assert hit.any() and abs(out['hit_rate'] - hit.mean()) < 1e-12
    assert abs(out['mrr_at_k'] - np.where(hit, 1.0 / (np.maximum(pos, 0) + 1.0), 0.0).mean()) < 1e-12
    assert set_a == bitmap_ids(bm, n_nodes) and len(set_a) > 40
    assert_same_state(state_of(A), state_of(B))


# ------------------------------------------------------------------------------------------ forms, cold start, refusals
def test_per_node_tables_follow_the_restart():
    """eager updates + pre-multiplied weights with current tables: rank_scores(uptodate=bm) restarts and keeps the tables
    current (the restarted rows are recomputed, no rebuild over every node), and the next stream step embeds as a
    plain-form twin does"""
    from www2023tiger_amd import hip_ops
    (A,), st = twins(1, 1, True, forms=('fused', 'eager'))
    (B,), _ = twins(1, 1, True)
    src, dst, ts, cand = ranked_batch(st, 20, 5)
    assert A._pending_stamp == A._state_stamp() and getattr(A, '_gtab', None) is not None
    bm_a, bm_b = (hip_ops.new_bitmap(st['n_nodes'], dev()) for _ in range(2))
    sa = A.rank_scores(t(src), t(dst), t(ts, torch.float64), t(cand), uptodate=bm_a)
    assert A.last_restarted > 0 and A._pending_stamp == A._state_stamp()
    sb = B.rank_scores(t(src), t(dst), t(ts, torch.float64), t(cand), uptodate=bm_b)
    assert torch.equal(bm_a, bm_b)
    assert_close(sa.cpu().numpy(), sb.cpu().numpy(), 'scores', TOL)
    lo = WARM[-1]
    ha = A.stream_step(*batch(st, lo, lo + 20)).h[:40].cpu().numpy()
    hb = B.stream_step(*batch(st, lo, lo + 20)).h[:40].cpu().numpy()
    assert_close(ha, hb, 'h after the restart', TOL)


@pytest.mark.parametrize('L,seq', [(1, True), (2, False)], ids=['L1-seq', 'L2-static'])
def test_cold_start_recommendation(L, seq):
    """a freshly built model (memories at reset) answers from an empty bitmap: the restart covers exactly the reference's
    involved set; asked again it restarts nothing and answers the same"""
    from www2023tiger_amd import hip_ops
    (A,), st = twins(1, L, seq, warmed=False)
    n_nodes = st['n_nodes']
    src, ts = st['src'][-50:], st['ts'][-50:]
    cat = np.arange(st['n_nodes'] - 15, st['n_nodes'], dtype=np.int64)   # the items
    bm = hip_ops.new_bitmap(n_nodes, dev())
    ids, scores, n_valid = A.recommend(t(src), t(ts, torch.float64), t(cat), 5, uptodate=bm)
    assert torch.isfinite(scores).all() and (n_valid > 0).all()
    og = R.oracle_graph(dict(st, n_nodes=n_nodes), 'recent_edges')
    nodes = np.concatenate([src, np.tile(cat, 50)])
    want = R.numpy_involved(og, nodes, np.concatenate([ts, np.repeat(ts, len(cat))]), K, L, 'recent_edges')
    assert A.last_restarted == len(want) and bitmap_ids(bm, n_nodes) == set(want.tolist())
    after = state_of(A)
    ids2, scores2, n_valid2 = A.recommend(t(src), t(ts, torch.float64), t(cat), 5, uptodate=bm)
    assert A.last_restarted == 0
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2) and torch.equal(n_valid, n_valid2)
    assert_same_state(after, state_of(A))


def test_refusals_come_before_anything_runs():
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.eval_utils import eval_edge_ranking, eval_recommendation
    from www2023tiger_amd.model.tiger import TIGE
    (m,), st = twins(1, 1, False)
    n = st['n_nodes']
    src, dst, ts, cand = ranked_batch(st, 3, 5)
    nodes, times = flat_queries(src, dst, ts, cand)
    bm = hip_ops.new_bitmap(n, dev())
    before = state_of(m)
    args = (t(src), t(dst), t(ts, torch.float64), t(cand))
    uni = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='uniform', seed=0, max_node_id=n - 1,
                            device=dev())
    mt = uni._mt_state().clone()
    with pytest.raises(NotImplementedError, match='uniform'):
        m.restart_involved(t(nodes), t(times, torch.float64), bm, graph=uni)
    with pytest.raises(NotImplementedError, match='uniform'):
        m.rank_scores(*args, uptodate=bm, graph=uni)
    assert torch.equal(mt, uni._mt_state())
    bad = nodes.copy()
    bad[-1] = n
    with pytest.raises(ValueError, match='node id'):
        m.restart_involved(t(bad), t(times, torch.float64), bm)
    with pytest.raises(ValueError, match='node id'):
        m.recommend(t(src), t(ts, torch.float64), torch.full_like(t(cand), n), 3, uptodate=bm)
    small = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='recent_edges', max_node_id=n + 3,
                              device=dev())
    with pytest.raises(ValueError, match='node ids'):
        m.restart_involved(t(nodes), t(times, torch.float64), bm, graph=small)
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.restart_involved(t(nodes), t(times, torch.float64), bm)
    with pytest.raises(RuntimeError, match='eval'):
        m.rank_scores(*args, uptodate=bm)
    m.eval()
    with pytest.raises(NotImplementedError, match='restart'):
        eval_edge_ranking(m, None, dev(), cand, restart_mode=True)
    with pytest.raises(NotImplementedError, match='restart'):
        eval_recommendation(m, None, dev(), cand[0], restart_mode=True)
    # a TIGE has no restarter
    restarter = m.restarter_fn
    del m.restarter_fn
    assert isinstance(m, TIGE)
    with pytest.raises(NotImplementedError, match='restarter'):
        m.rank_scores(*args, uptodate=bm)
    with pytest.raises(NotImplementedError, match='restarter'):
        m.recommend(t(src), t(ts, torch.float64), t(cand), 3, uptodate=bm)
    with pytest.raises(NotImplementedError, match='restarter'):
        eval_edge_ranking(m, None, dev(), cand, lazy_restarts=True)
    m.restarter_fn = restarter
    assert_same_state(before, state_of(m))
    assert not bm.any()
    m.partition_state(torch.arange(n, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.restart_involved(t(nodes), t(times, torch.float64), bm)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.rank_scores(*args, uptodate=bm)
    assert not bm.any()


def test_examples_run_with_their_new_flags(tmp_path):
    """examples/link_prediction.run(rank=C) in restart mode ranks with lazy restarts from the test's own up-to-date set;
    examples/recommend.run_cold answers from memories at reset - on toy JODIE files"""
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
    out, _ = lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, restart_prob=0.5, rank=3, ckpt_path=ckpt, **kw)
    assert 0.0 < out['test_mrr'] <= 1.0 and 0.0 < out['ind_test_mrr'] <= 1.0
    assert all(np.isfinite(out[k]) for k in ('test_ap', 'test_auc', 'ind_test_ap', 'ind_test_auc'))
    m, restarted = rc.run_cold('toy', str(tmp_path), ckpt, k=5, verbose=False, **kw)
    assert m['n_events'] > 0 and restarted[0] > 0 and 0.0 <= m['hit_rate'] <= 1.0
