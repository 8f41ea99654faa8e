"""Catalogue snapshots on the GPU: TIGE.embed_catalogue, TIGE.recommend on a snapshot (tg_rank_cand_half +
tg_rank_scores_shared) and eval_recommendation(catalogue_at='batch'), on the small model of tests/test_hip_rank.py
(d = 16, K = 10) with the catalogue of ALL node ids (the padding id 0 included).  When every query stands at the
snapshot's time the lists are those of the per-pair path: every comparison is exact - ids, score bits, n_valid, state.
For queries later than the snapshot the scores are checked against the float64 head of tests/_rank_ref.py within its
derived bound."""
import numpy as np
import pytest
import torch

from _rank_ref import score_bound, score_ref
from test_hip_rank import WARM, assert_same_state, batch, build, dev, loader, state_of, warm

pytestmark = pytest.mark.gpu
D, K = 16, 10


def t(x, dt=torch.int64):
    return torch.as_tensor(x).to(dev(), dt)


def warmed(hit='bin', seed=D + K, **kw):
    model, orc, st = build(D, D, K, hit, seed=seed, **kw)
    warm(model, orc, st, K, with_oracle=False)
    return model, st


def at_one_time(st, B, ahead=20):
    """B sources behind the warm-up, all asking at ONE time: that of an event `ahead` events later (so the sources' own
    events of the batch lie before the query time and the neighbour lists are not empty), and the catalogue of all ids"""
    lo = WARM[-1]
    src = batch(st, lo, lo + B)[0]
    when = float(st['ts'][lo + B + ahead])
    cat = np.arange(st['n_nodes'], dtype=np.int64)
    return t(src), torch.full((B,), when, dtype=torch.float64, device=dev()), t(cat), when


def same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2]))


# ------------------------------------------------------------------------------------------ snapshot == per-pair path
MODELS = [dict(hit='none'), dict(hit='bin'), dict(hit='count'), dict(hit='vec'), dict(hit='bin', L=2),
          dict(hit='count', strategy='recent_nodes')]


@pytest.mark.parametrize('kw', MODELS, ids=['none', 'bin', 'count', 'vec', 'bin-L2', 'count-recent_nodes'])
def test_a_snapshot_at_the_query_time_gives_the_lists_of_the_per_pair_path(kw):
    """recommend(src, full(t), snap) == recommend(src, full(t), cat) == recommend(src, full(t), cat, catalogue_at=t) - ids,
    score bits, n_valid; also with a mask, with exclude_seen, with one query per chunk and with k above the items left in.
    (Fails without the feature: there is no embed_catalogue.)"""
    from www2023tiger_amd.model.tiger import CatalogueSnapshot
    model, st = warmed(**kw)
    src, ts, cat, when = at_one_time(st, 9)
    k, C = 10, cat.numel()
    before = state_of(model)
    snap = model.embed_catalogue(cat, when)
    assert isinstance(snap, CatalogueSnapshot) and len(snap) == C and snap.t == when and snap.model is model
    assert snap.h.shape == (C, D) and snap.h.dtype == torch.float32 and torch.equal(snap.ids, cat)
    assert (snap.nb is None) == (kw['hit'] == 'none') and (snap.nb is None or snap.nb.shape == (C, K))
    want = model.recommend(src, ts, cat, k)
    assert (want[2] == C - 1).all() and torch.isfinite(want[1]).all()   # everything but the padding id is left in
    assert want[1].unique().numel() > 9                                 # (the queries do not all score alike)
    assert same(model.recommend(src, ts, snap, k), want)
    assert same(model.recommend(src, ts, cat, k, catalogue_at=when), want)
    # a mask [C] and a mask [B, C]; k above the items left in
    rs = np.random.RandomState(5)
    m1 = t(rs.rand(C) > 0.4, torch.bool)
    m2 = t(rs.rand(9, C) > 0.9, torch.bool)
    for mk, kk in ((m1, k), (m2, 64)):
        want_m = model.recommend(src, ts, cat, kk, mask=mk)
        assert same(model.recommend(src, ts, snap, kk, mask=mk), want_m)
        assert same(model.recommend(src, ts, cat, kk, mask=mk, catalogue_at=when), want_m)
    assert int(want_m[2].min()) < 64 and (want_m[0][0, int(want_m[2][0]):] == 0).all()
    # exclude_seen (with the caller's mask on top), and one query per chunk
    want_s = model.recommend(src, ts, cat, k, exclude_seen=True, mask=m1)
    assert int(want_s[2].min()) < int(m1[1:].sum())                    # something was seen
    assert same(model.recommend(src, ts, snap, k, exclude_seen=True, mask=m1), want_s)
    assert same(model.recommend(src, ts, snap, k, chunk_queries=1), want)
    assert same(model.recommend(src, ts, cat, k, chunk_queries=1, catalogue_at=when), want)
    assert_same_state(before, state_of(model))


def test_nothing_is_written_and_a_later_step_equals_a_twin_that_never_made_a_snapshot():
    (m1, st), (m2, _) = warmed(), warmed()
    assert_same_state(state_of(m1), state_of(m2))
    src, ts, cat, when = at_one_time(st, 5)
    before = state_of(m1)
    snap = m1.embed_catalogue(cat, when)
    assert_same_state(before, state_of(m1))
    m1.recommend(src, ts, snap, 10)
    m1.recommend(src, ts + 3.0, snap, 10, exclude_seen=True)
    m1.recommend(src, ts, cat, 10, catalogue_at=when)
    assert_same_state(before, state_of(m1))
    a = batch(st, WARM[-1], WARM[-1] + 5)
    assert torch.equal(m1.stream_step(*a).h.clone(), m2.stream_step(*a).h.clone())
    assert_same_state(state_of(m1), state_of(m2))


def test_the_lazy_one_shot_form_equals_the_lazy_per_pair_form():
    """twin models at reset, empty bitmaps: one restart over B + C queries against one over B (1 + C) - the same involved
    set when every query stands at t, so the same count, bitmap, state and lists"""
    from www2023tiger_amd import hip_ops
    built = [build(D, D, K, 'bin', seed=D + K) for _ in range(3)]
    (A, B, E), st = [b[0] for b in built], built[0][2]
    src, ts, cat, when = at_one_time(st, 9)
    cat = cat[40:]   # (a part of the nodes: the restart does not simply cover everything)
    bm_a, bm_b, bm_e = (hip_ops.new_bitmap(st['n_nodes'], dev()) for _ in range(3))
    one = A.recommend(src, ts, cat, 10, catalogue_at=when, uptodate=bm_a)
    two = B.recommend(src, ts, cat, 10, uptodate=bm_b)
    assert same(one, two)
    assert A.last_restarted == B.last_restarted > 0 and torch.equal(bm_a, bm_b)
    assert int((bm_a != 0).sum()) > 0
    assert_same_state(state_of(A), state_of(B))
    # the two-step way out named by the refusal: restart the sources, then embed_catalogue(..., uptodate=bm)
    n1 = E.restart_involved(src, ts, bm_e)
    snap = E.embed_catalogue(cat, when, uptodate=bm_e)
    assert n1 + E.last_restarted == A.last_restarted and torch.equal(bm_e, bm_a)
    # (the nodes are restarted at the earliest query time, which is `when` in either call: the same state)
    assert_same_state(state_of(A), state_of(E))
    assert same(E.recommend(src, ts, snap, 10), one)


# ------------------------------------------------------------------------------------------ later queries
def head_ref(model, src, ts, snap, graph=None):
    """float64 scores [B, C] and bounds of the score head fed with the sources' embeddings at ts[i] (`_embed_queries`) and
    the snapshot's stored rows"""
    from www2023tiger_amd import hip_ops
    graph = model.graph if graph is None else graph
    with torch.no_grad():
        model._embed_prepare()
        err = hip_ops.new_err(dev())
        h_src, nb_src = model._embed_queries(src, ts, graph, graph.strategy, err)
        hip_ops.raise_if_err(err)
    n = lambda a: None if a is None else a.detach().cpu().numpy()
    B, C = src.numel(), len(snap)
    hit = model.hit_type
    bc = lambda a: None if a is None else np.broadcast_to(a[None], (B,) + a.shape)
    emb = n(model.hit_embedding.weight) if hit in ('bin', 'count') else None
    s, A = score_ref(n(h_src), bc(n(snap.h)), n(nb_src), bc(n(snap.nb)), n(src), bc(n(snap.ids)),
                     n(model.score_fn.fc1.weight), n(model.score_fn.fc1.bias), n(model.score_fn.fc2.weight),
                     n(model.score_fn.fc2.bias), hit, emb)
    W = D + (K if hit == 'vec' else 0)
    return s, score_bound(A, D, W)


def assert_lists_within_bound(got, ref, bound, cat):
    """every listed (id, score): the score within the bound of the float64 score of that id's column (catalogue = all ids,
    so the column is the id), and the list in descending order"""
    ids, scores, n_valid = (x.cpu().numpy() for x in got)
    assert np.array_equal(cat, np.arange(len(cat)))
    worst = 0.0
    for i in range(ids.shape[0]):
        nv = int(n_valid[i])
        assert nv > 0 and (ids[i, :nv] != 0).all() and (np.diff(scores[i, :nv]) <= 0).all()
        err = np.abs(scores[i, :nv].astype(np.float64) - ref[i, ids[i, :nv]])
        worst = max(worst, float((err / bound[i, ids[i, :nv]]).max()))
    print(f'worst err / bound over the listed pairs {worst:.3e}')
    assert worst <= 1.0


@pytest.mark.parametrize('hit', ['count', 'vec'])
def test_queries_later_than_the_snapshot_score_items_as_of_the_snapshot(hit):
    model, st = warmed(hit)
    src, ts, cat, when = at_one_time(st, 9, ahead=0)
    snap = model.embed_catalogue(cat, when)
    at_t = model.recommend(src, ts, snap, 64)
    later = ts + torch.linspace(0.0, 400.0, 9, dtype=torch.float64, device=dev())   # query 0 stays at t
    got = model.recommend(src, later, snap, 64)
    ref, bound = head_ref(model, src, later, snap)
    assert_lists_within_bound(got, ref, bound, cat.cpu().numpy())
    assert torch.equal(got[0][0], at_t[0][0]) and torch.equal(got[1][0], at_t[1][0])   # the query at t: unchanged
    assert not torch.equal(got[1][1:], at_t[1][1:])                                     # a later one: other scores
    # and they are not the per-pair path's either: that one embeds the items at the queries' own times
    assert not torch.equal(got[1], model.recommend(src, later, cat, 64)[1])


# ------------------------------------------------------------------------------------------ staleness
def prefix_model(hit='bin', n_seen=WARM[-1] + 30):
    """a warmed model whose graph covers the first n_seen events only, so that `observe` can ingest the next ones"""
    from www2023tiger_amd.data.graph import Graph
    model, orc, st = build(D, D, K, hit, seed=D + K)
    model.graph = Graph.from_arrays(st['src'][:n_seen], st['dst'][:n_seen], st['ts'][:n_seen], st['eids'][:n_seen],
                                    strategy='recent_edges', seed=0, max_node_id=st['n_nodes'] - 1, device=dev())
    warm(model, orc, st, K, with_oracle=False)
    return model, st, n_seen


def test_a_stale_snapshot_is_refused_unless_stale_ok():
    model, st, n_seen = prefix_model()
    B = 6
    src = t(batch(st, WARM[-1], WARM[-1] + B)[0])
    cat = t(np.arange(st['n_nodes'], dtype=np.int64))
    when = float(st['ts'][n_seen - 1]) + 1.0
    ts = torch.full((B,), when + 2000.0, dtype=torch.float64, device=dev())   # behind everything that is observed below
    nxt = [n_seen]

    def stream_step():
        model.stream_step(*batch(st, WARM[-1], WARM[-1] + 5))

    def observe():
        a = batch(st, nxt[0], nxt[0] + 5)
        nxt[0] += 5
        model.observe(a[0], a[1], a[3], a[4])

    def forget():
        model.forget(keep_last=10 ** 6)   # drops nothing: a new graph object with the same entries

    def restart():
        model.restart(t([3, 4, 70]), torch.full((3,), np.float32(when), device=dev()))

    for change in (forget, stream_step, observe, restart):
        snap = model.embed_catalogue(cat, when)
        fresh = model.recommend(src, ts, snap, 64)
        change()
        before = state_of(model)
        with pytest.raises(RuntimeError, match='stale'):
            model.recommend(src, ts, snap, 64)
        assert_same_state(before, state_of(model))
        got = model.recommend(src, ts, snap, 64, stale_ok=True)   # items as of the snapshot, sources on the new state
        ref, bound = head_ref(model, src, ts, snap)
        assert_lists_within_bound(got, ref, bound, cat.cpu().numpy())
        if change is forget:      # nothing the scores read has changed: the lists of the fresh snapshot
            assert same(got, fresh)
        if change is restart:     # items 3 and 4 were re-initialised; the snapshot still holds their old rows
            again = model.recommend(src, ts, model.embed_catalogue(cat, when), 64)
            assert not torch.equal(again[1], got[1])
        assert_same_state(before, state_of(model))


def test_P_follows_the_score_head():
    """an in-place change of fc1.weight does not make the snapshot stale (the embeddings do not read it), but P is computed
    again: the lists equal those of a fresh snapshot and of the per-pair path"""
    model, st = warmed('count')
    src, ts, cat, when = at_one_time(st, 7)
    snap = model.embed_catalogue(cat, when)
    first = model.recommend(src, ts, snap, 10)
    P0 = snap._P.clone()
    with torch.no_grad():
        model.score_fn.fc1.weight.mul_(1.5)
    second = model.recommend(src, ts, snap, 10)
    assert not torch.equal(P0, snap._P) and not torch.equal(first[1], second[1])
    assert same(second, model.recommend(src, ts, model.embed_catalogue(cat, when), 10))
    assert same(second, model.recommend(src, ts, cat, 10))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_anything_runs():
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.data.graph import Graph
    (m, st), (other, _) = warmed(), warmed()
    src, ts, cat, when = at_one_time(st, 5)
    snap = m.embed_catalogue(cat, when)
    bm = hip_ops.new_bitmap(st['n_nodes'], dev())
    bm0 = bm.clone()
    before = state_of(m)
    early = ts.clone()
    early[3] = when - 1.0
    with pytest.raises(ValueError, match='future'):
        m.recommend(src, early, snap, 5)
    with pytest.raises(ValueError, match='future'):
        m.recommend(src, early, cat, 5, catalogue_at=when, uptodate=bm)
    with pytest.raises(ValueError, match='another model'):
        m.recommend(src, ts, other.embed_catalogue(cat, when), 5)
    small = m.embed_catalogue(cat, when)
    small.n_nodes -= 1
    with pytest.raises(ValueError, match='node ids'):
        m.recommend(src, ts, small, 5)
    with pytest.raises(ValueError, match=r'(?s)catalogue_at.*embed_catalogue'):
        m.recommend(src, ts, snap, 5, uptodate=bm)
    with pytest.raises(ValueError, match='catalogue_at'):
        m.recommend(src, ts, cat.unsqueeze(0).expand(5, -1), 5, catalogue_at=when)
    with pytest.raises(ValueError, match='catalogue_at'):
        m.recommend(src, ts, snap, 5, catalogue_at=when)
    with pytest.raises(ValueError, match='NaN'):
        m.embed_catalogue(cat, float('nan'))
    with pytest.raises(ValueError, match=r'\[C\]'):
        m.embed_catalogue(cat.unsqueeze(0), when)
    with pytest.raises(ValueError, match='node id'):
        m.embed_catalogue(torch.full_like(cat, st['n_nodes']), when)
    with pytest.raises(ValueError, match='k <='):
        m.recommend(src, ts, snap, 65)
    with pytest.raises(ValueError, match='mask'):
        m.recommend(src, ts, snap, 5, mask=torch.ones(5, 4, dtype=torch.bool))
    uni = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='uniform', seed=0,
                            max_node_id=st['n_nodes'] - 1, device=dev())
    mt = uni._mt_state().clone()
    with pytest.raises(NotImplementedError, match='uniform'):
        m.embed_catalogue(cat, when, graph=uni)
    with pytest.raises(NotImplementedError, match='uniform'):
        m.recommend(src, ts, snap, 5, graph=uni)
    assert torch.equal(mt, uni._mt_state())
    assert_same_state(before, state_of(m))
    assert torch.equal(bm, bm0)
    assert same(m.recommend(src, ts, snap, 5), m.recommend(src, ts, cat, 5))   # the snapshot is still good
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.recommend(src, ts, snap, 5)
    with pytest.raises(RuntimeError, match='eval'):
        m.embed_catalogue(cat, when)
    m.eval()
    with pytest.raises(RuntimeError, match='stale'):   # train() starts a new parameter epoch: whoever trains passes through it
        m.recommend(src, ts, snap, 5)
    assert_same_state(before, state_of(m))
    ids, scores, n_valid = m.recommend(src, ts, m.embed_catalogue(cat[:0], when), 3)   # an empty catalogue: all padding
    assert (ids == 0).all() and torch.isneginf(scores).all() and (n_valid == 0).all()
    plain, _, _ = build(D, D, K, 'bin')
    plain.restarter_fn = None
    with pytest.raises(NotImplementedError, match='restarter'):
        plain.embed_catalogue(cat, when, uptodate=bm)
    vec, _, _ = build(8, 8, 5, 'vec')
    with pytest.raises(NotImplementedError, match='vec'):
        vec.embed_catalogue(cat, when)
    n = st['n_nodes']
    m.partition_state(torch.arange(n, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.embed_catalogue(cat, when)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.recommend(src, ts, snap, 5)


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('lazy', [False, True], ids=['plain', 'lazy-restarts'])
def test_eval_recommendation_with_one_snapshot_per_batch(lazy):
    """150 events at batch 50: eval_recommendation(catalogue_at='batch') equals the loop written out from public pieces -
    embed_catalogue at the batch's first time on the state before the batch (lazy: after ONE restart_involved over
    cat[src, dst, neg] at the event times and the catalogue at that one time), recommend on the snapshot,
    contrast_learning - in positions, metrics, state and up-to-date set; the default protocol is another one"""
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.eval_utils import eval_recommendation
    k, E = 10, 150
    built = [build(D, D, K, 'bin', seed=3, E=E) for _ in range(3)]
    (A, B, X), st = [b[0] for b in built], built[0][2]
    n_nodes = st['n_nodes']
    cat = np.arange(1, n_nodes, dtype=np.int64)
    set_a = set() if lazy else None
    out = eval_recommendation(A, loader(A, st, K), dev(), cat, k=k, exclude_seen=True, return_positions=True,
                              catalogue_at='batch', lazy_restarts=lazy, uptodate_nodes=set_a)
    col_of = hip_ops.catalogue_index(t(cat), n_nodes)
    bm = hip_ops.new_bitmap(n_nodes, dev())
    positions, counts = [], []
    with torch.no_grad():
        for src, dst, neg, ts, eids, _, cg in loader(B, st, K):
            src, dst, neg, ts, eids = (x.to(dev()) for x in (src, dst, neg, ts, eids))
            t0 = float(cg.ts64[0])
            assert t0 == float(cg.ts64.min())
            if lazy:
                nodes = torch.cat([src, dst, neg, t(cat)])
                times = torch.cat([cg.ts64.repeat(3), torch.full((len(cat),), t0, dtype=torch.float64, device=dev())])
                counts.append(B.restart_involved(nodes, times, bm))
            snap = B.embed_catalogue(t(cat), t0)
            seen = hip_ops.seen_mask(B.graph, src, cg.ts64, col_of, len(cat))
            ids, _, _ = B.recommend(src, cg.ts64, snap, k, mask=seen)
            hit = (ids == dst[:, None]) & (ids != 0)
            positions.append(torch.where(hit.any(1), hit.float().argmax(1), -1).cpu().numpy())
            B.contrast_learning(src, dst, neg, ts, eids, cg)
    pos = np.concatenate(positions)
    np.testing.assert_array_equal(out['positions'].cpu().numpy(), pos)
    hit = pos >= 0
    assert out['n_events'] == E and hit.any() and abs(out['hit_rate'] - hit.mean()) < 1e-12
    assert abs(out['ndcg'] - np.where(hit, 1.0 / np.log2(np.maximum(pos, 0) + 2.0), 0.0).mean()) < 1e-12
    assert abs(out['mrr_at_k'] - np.where(hit, 1.0 / (np.maximum(pos, 0) + 1.0), 0.0).mean()) < 1e-12
    assert_same_state(state_of(A), state_of(B))
    if lazy:
        import _involved_ref as R
        assert counts[0] > 0 and set_a == set(np.nonzero(R.from_bitmap(bm.cpu().numpy(), n_nodes))[0].tolist())
    else:   # the exact protocol advances the state the same way
        exact = eval_recommendation(X, loader(X, st, K), dev(), cat, k=k, exclude_seen=True, return_positions=True)
        assert exact['n_events'] == E and exact['coverage'] == out['coverage']
        assert_same_state(state_of(A), state_of(X))
        print(f"catalogue_at='batch': hit_rate {out['hit_rate']:.4f} ndcg {out['ndcg']:.4f}; exact: hit_rate "
              f"{exact['hit_rate']:.4f} ndcg {exact['ndcg']:.4f}; {(exact['positions'].cpu().numpy() != pos).sum()} of {E} "
              'positions differ (untrained weights)')
