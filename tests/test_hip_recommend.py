"""TIGE.recommend and eval_recommendation on the GPU, on the small model of tests/test_hip_rank.py.  recommend is
rank_scores followed by tg_topk_rows: every comparison here is exact - ids, score bits, state."""
import numpy as np
import pytest
import torch

from _topk_ref import numpy_seen_mask
from _rank_ref import numpy_ranks
from test_hip_rank import WARM, assert_same_state, batch, build, dev, loader, state_of, warm

pytestmark = pytest.mark.gpu
D, K = 16, 10


def t(x, dt=torch.int64):
    return torch.as_tensor(x).to(dev(), dt)


def warmed(hit='bin', seed=D + K, **kw):
    model, orc, st = build(D, D, K, hit, seed=seed, **kw)
    warm(model, orc, st, K, with_oracle=False)
    return model, st


def queries(st, B, C, seed=4):
    """B (source, time) queries behind the warm-up and per-query candidates [B, C]: random nodes, the pad id in column 1,
    column 3 a copy of column 2"""
    lo = WARM[-1]
    src, _, _, ts, _ = batch(st, lo, lo + B)
    cand = np.random.RandomState(seed).randint(1, st['n_nodes'], (B, C)).astype(np.int64)
    cand[:, 1] = 0
    cand[:, 3] = cand[:, 2]
    return t(src), t(ts, torch.float64), t(cand)


def test_recommend_is_topk_rows_of_rank_scores():
    """cand[:, 0] as rank_scores's destination column: the same [B, C] pairs, so the same bits (a pair's score does not
    depend on where it stands), then the library's selection"""
    from www2023tiger_amd import hip_ops
    model, st = warmed()
    src, ts, cand = queries(st, 32, 33)
    k = 10
    before = state_of(model)
    ids, scores, n_valid = model.recommend(src, ts, cand, k)
    assert ids.shape == (32, k) and ids.dtype == torch.int64 and scores.dtype == torch.float32 and n_valid.dtype == torch.int32
    pair = model.rank_scores(src, cand[:, 0], ts, cand[:, 1:])
    want = hip_ops.topk_rows(pair, cand, k)
    assert torch.equal(ids, want['ids']) and torch.equal(scores.view(torch.int32), want['scores'].view(torch.int32))
    assert torch.equal(n_valid, want['n_valid']) and int(n_valid.max()) == 32 and (ids != 0).all()
    # the duplicated candidate stands twice, earlier column first, with equal bits
    s = pair.cpu().numpy()
    assert np.array_equal(s[:, 2].view(np.uint32), s[:, 3].view(np.uint32))
    # a mask, k above the candidates left in
    mask = torch.ones_like(cand, dtype=torch.bool)
    mask[::2, 5:] = False
    ids, scores, n_valid = model.recommend(src, ts, cand, 64, mask=mask)
    want = hip_ops.topk_rows(pair, cand, 64, mask=mask)
    assert torch.equal(ids, want['ids']) and torch.equal(scores.view(torch.int32), want['scores'].view(torch.int32))
    assert n_valid[0] == 4 and (ids[0, 4:] == 0).all() and torch.isneginf(scores[0, 4:]).all() and n_valid[1] == 32
    # a shared catalogue is its broadcast form
    one = model.recommend(src, ts, cand[0], k)
    two = model.recommend(src, ts, cand[0].unsqueeze(0).expand(32, -1).contiguous(), k)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    assert_same_state(before, state_of(model))


def test_chunked_equals_unchunked():
    model, st = warmed()
    src, ts, cand = queries(st, 32, 33)
    whole = model.recommend(src, ts, cand, 10)
    for per_chunk in (10 * 34, 1):   # 10 queries per chunk (4 chunks); one query per chunk
        parts = model.recommend(src, ts, cand, 10, chunk_queries=per_chunk)
        assert all(torch.equal(a, b) for a, b in zip(whole, parts)), per_chunk


def test_a_step_after_recommend_equals_a_twin_that_never_called_it():
    (m1, st), (m2, _) = warmed(), warmed()
    assert_same_state(state_of(m1), state_of(m2))
    src, ts, cand = queries(st, 5, 7)
    cat = t(np.arange(1, st['n_nodes']))
    m1.recommend(src, ts, cand, 3)
    m1.recommend(src, ts, cat, 10, exclude_seen=True)
    assert_same_state(state_of(m1), state_of(m2))
    a = batch(st, WARM[-1], WARM[-1] + 5)
    assert torch.equal(m1.stream_step(*a).h.clone(), m2.stream_step(*a).h.clone())
    assert_same_state(state_of(m1), state_of(m2))


def test_exclude_seen_removes_exactly_the_listed_items():
    from www2023tiger_amd import hip_ops
    model, st = warmed()
    B = 40
    lo = WARM[-1] + 50   # queries deep in the stream: sources with a history
    src_np, _, _, ts_np, _ = batch(st, lo, lo + B)
    src, ts = t(src_np), t(ts_np, torch.float64)
    cat_np = np.random.RandomState(2).permutation(np.arange(1, st['n_nodes'])).astype(np.int64)
    cat = t(cat_np)
    C, k = len(cat_np), 64
    allowed = numpy_seen_mask(st['src'], st['dst'], st['ts'], src_np, ts_np, cat_np)
    assert (~allowed).any(1).sum() > B // 2 and allowed.any(1).all()
    ids, scores, n_valid = model.recommend(src, ts, cat, k, exclude_seen=True)
    np.testing.assert_array_equal(n_valid.cpu().numpy(), allowed.sum(1))
    pair = model.rank_scores(src, cat[:1].expand(B), ts, cat[1:])
    want = hip_ops.topk_rows(pair, cat, k, mask=t(allowed, torch.bool))
    assert torch.equal(ids, want['ids']) and torch.equal(scores.view(torch.int32), want['scores'].view(torch.int32))
    got = ids.cpu().numpy()
    for i in range(B):   # and said directly: no listed item is a seen one, every other item is listed (k >= C here or not)
        listed = set(got[i][got[i] != 0].tolist())
        seen = set(cat_np[~allowed[i]].tolist())
        assert not (listed & seen)
        if allowed[i].sum() <= k:
            assert listed == set(cat_np[allowed[i]].tolist())
    # with the caller's mask on top, and a prepared col_of
    mine = np.random.RandomState(3).rand(C) > 0.5
    col_of = hip_ops.catalogue_index(cat, st['n_nodes'])
    ids2, _, nv2 = model.recommend(src, ts, cat, k, exclude_seen=True, mask=t(mine, torch.bool), col_of=col_of)
    np.testing.assert_array_equal(nv2.cpu().numpy(), (allowed & mine[None, :]).sum(1))
    assert torch.equal(ids2, hip_ops.topk_rows(pair, cat, k, mask=t(allowed & mine[None, :], torch.bool))['ids'])


def test_refusals_come_before_anything_runs():
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.eval_utils import eval_recommendation
    m, st = warmed()
    src, ts, cand = queries(st, 3, 5)
    before = state_of(m)
    uni = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='uniform', seed=0,
                            max_node_id=st['n_nodes'] - 1, device=dev())
    mt = uni._mt_state().clone()
    with pytest.raises(NotImplementedError, match='uniform'):
        m.recommend(src, ts, cand, 3, graph=uni)
    assert torch.equal(mt, uni._mt_state())
    with pytest.raises(ValueError, match='shared'):
        m.recommend(src, ts, cand, 3, exclude_seen=True)
    with pytest.raises(ValueError, match='duplicate'):
        m.recommend(src, ts, t([5, 6, 5]), 3, exclude_seen=True)
    with pytest.raises(ValueError, match='k <='):
        m.recommend(src, ts, cand, 65)
    with pytest.raises(ValueError, match='k <='):
        m.recommend(src, ts, cand, 0)
    with pytest.raises(ValueError, match='node id'):
        m.recommend(src, ts, torch.full_like(cand, st['n_nodes']), 3)
    with pytest.raises(ValueError, match='mask'):
        m.recommend(src, ts, cand, 3, mask=torch.ones(3, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match='restart'):
        eval_recommendation(m, None, dev(), cand[0], restart_mode=True)
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.recommend(src, ts, cand, 3)
    m.eval()
    assert_same_state(before, state_of(m))
    ids, scores, n_valid = m.recommend(src, ts, cand[:, :0], 3)   # no candidates: all padding, nothing scored
    assert (ids == 0).all() and torch.isneginf(scores).all() and (n_valid == 0).all()
    vec, _, _ = build(8, 8, 5, 'vec')
    with pytest.raises(NotImplementedError, match='vec'):
        vec.recommend(src, ts, cand, 3)
    n = st['n_nodes']
    m.partition_state(torch.arange(n, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.recommend(src, ts, cand, 3)
    with pytest.raises(RuntimeError, match='partitioned'):
        eval_recommendation(m, None, dev(), cand[0])


def test_a_non_finite_score_raises():
    m, st = warmed()
    src, ts, cand = queries(st, 3, 5)
    with torch.no_grad():
        m.score_fn.fc2.bias.fill_(float('nan'))
    with pytest.raises(ValueError, match='12 non-finite'):   # 3 queries x 4 candidates left in (column 1 is the pad id)
        m.recommend(src, ts, cand, 3)


@pytest.mark.parametrize('exclude_seen', [False, True], ids=['all-items', 'exclude-seen'])
def test_eval_recommendation_end_to_end(exclude_seen):
    """150 events at batch 50 over the catalogue of all nodes.  Without ties at the positive's score, the destination's
    place in the list is the number of items scored above it, so [listed in the top k] = [rank <= k] of eval_edge_ranking
    over the same catalogue (with the seen items masked there too); ndcg / mrr_at_k from the returned positions; the
    state advances as eval_edge_ranking's."""
    from www2023tiger_amd.eval_utils import eval_edge_ranking, eval_recommendation
    k, E = 10, 150
    built = [build(D, D, K, 'bin', seed=3, E=E) for _ in range(3)]
    models, st = [b[0] for b in built], built[0][2]
    cat = np.arange(1, st['n_nodes'], dtype=np.int64)
    out = eval_recommendation(models[0], loader(models[0], st, K), dev(), cat, k=k, exclude_seen=exclude_seen,
                              return_positions=True)
    pos = out['positions'].cpu().numpy()
    assert out['n_events'] == E and pos.shape == (E,) and pos.min() >= -1 and pos.max() < k
    allowed = numpy_seen_mask(st['src'], st['dst'], st['ts'], st['src'], st['ts'], cat) if exclude_seen else None
    ranked = eval_edge_ranking(models[1], loader(models[1], st, K), dev(), np.tile(cat, (E, 1)), ks=(k,), mask=allowed,
                               return_ranks=True)
    ranks = ranked['ranks'].cpu().numpy()
    # ties at the positive's score, from a twin loop over the per-batch scores
    n_equal, lo = [], 0
    with torch.no_grad():
        for src, dst, neg, ts, eids, _, cg in loader(models[2], st, K):
            s = models[2].rank_scores(src.to(dev()), dst.to(dev()), cg.ts64, t(cat)).cpu().numpy()
            ids = np.concatenate([dst.cpu().numpy()[:, None], np.broadcast_to(cat, (len(src), len(cat)))], 1)
            mk = None if allowed is None else allowed[lo:lo + len(src)]
            g, e, v, r = numpy_ranks(s, ids, dst.cpu().numpy(), mk)
            np.testing.assert_array_equal(r, ranks[lo:lo + len(src)])
            n_equal.append(e)
            models[2].contrast_learning(src.to(dev()), dst.to(dev()), neg.to(dev()), ts.to(dev()), eids.to(dev()), cg)
            lo += len(src)
    untied = np.concatenate(n_equal) == 0
    print(f'exclude_seen={exclude_seen}: {int((~untied).sum())} of {E} events tie at the positive, hit_rate {out["hit_rate"]:.4f}, '
          f'coverage {out["coverage"]:.4f}, ndcg {out["ndcg"]:.4f}, mrr@k {out["mrr_at_k"]:.4f}')
    assert (~untied).sum() <= 0.05 * E
    # the destination takes part in the list only where it is left in; elsewhere it cannot be listed
    dcol = st['dst'] - 1
    left_in = np.ones(E, dtype=bool) if allowed is None else allowed[np.arange(E), dcol]
    np.testing.assert_array_equal((pos >= 0)[untied & left_in], (ranks <= k)[untied & left_in])
    np.testing.assert_array_equal(pos[untied & left_in], np.where(ranks <= k, ranks - 1, -1)[untied & left_in].astype(np.int64))
    assert (pos[~left_in] == -1).all()
    assert abs(out['coverage'] - left_in.mean()) < 1e-12
    if not exclude_seen:
        assert out['coverage'] == 1.0
        assert abs(np.mean((pos >= 0)[untied]) - np.mean((ranks <= k)[untied])) < 1e-12
    hit = pos >= 0
    assert abs(out['hit_rate'] - hit.mean()) < 1e-12
    assert abs(out['ndcg'] - np.where(hit, 1.0 / np.log2(np.maximum(pos, 0) + 2.0), 0.0).mean()) < 1e-12
    assert abs(out['mrr_at_k'] - np.where(hit, 1.0 / (np.maximum(pos, 0) + 1.0), 0.0).mean()) < 1e-12
    assert_same_state(state_of(models[0]), state_of(models[1]))
