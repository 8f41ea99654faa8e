"""tg_walk_candidates on the GPU, exactly.  Three groups: every host case of tests/test_walk_host.py through the kernel,
against the host twin and the numpy / dict reference of tests/_walk_ref.py; the launch at and past its grid cap; and the
model side - TIGE.recommend_walk and eval_recommendation(walk=...) on the small model of tests/test_hip_rank.py against
the two-call forms and a Python loop over the REFERENCE generator.  Integer work and bit-equal scores: no tolerance."""
import numpy as np
import pytest
import torch

import _cap_ref
import _walk_ref as R
import test_walk_host as H
from test_hip_rank import WARM, assert_same_state, batch, build, dev, loader, state_of, warm

pytestmark = pytest.mark.gpu
D, K = 16, 10


def t(x, dt=torch.int64):
    return torch.as_tensor(x).to(dev(), dt)


# ---- the host cases on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('exclude_seen', (False, True), ids=('all', 'exclude-seen'))
@pytest.mark.parametrize('Cn', R.CS)
@pytest.mark.parametrize('walk', R.WALKS, ids=R.walk_id)
def test_kernel_equals_the_host_twin_and_the_reference(walk, Cn, exclude_seen):
    H.check_small(walk, Cn, exclude_seen, dev())


def test_keep_self_on_the_self_loops():
    H.check_keep_self(dev())


@pytest.mark.parametrize('n', R.SWEEP_PREFIXES)
def test_exclude_seen_sweeps_the_whole_prefix(n):
    H.check_sweep(n, dev())


def test_degrees_around_the_largest_fan_out():
    H.check_degrees(dev())


def test_fan_outs_exactly_at_the_caps():
    H.check_at_caps(dev())


def test_power_of_two_strides_fill_the_table():
    H.check_strides(dev())


def test_trimmed_and_extended_graphs():
    H.check_derived_graphs(dev())


def test_refusals_and_no_queries_on_the_device():
    from www2023tiger_amd import hip_ops
    N, ev, _, src, ts = R.small_case()
    g = R.library_graph(N, ev, dev())
    for fanout, take, cap in R.PAST_CAPS:
        with pytest.raises(ValueError, match=cap):
            hip_ops.walk_candidates(g, t(src[:3]), t(ts[:3], torch.float64), 16, fanout=fanout, take=take)
    with pytest.raises(ValueError, match='source id'):
        hip_ops.walk_candidates(g, t([1, N, 2]), t(ts[:3], torch.float64), 16)
    with pytest.raises(ValueError, match='lives on'):                  # a host graph, device queries
        hip_ops.walk_candidates(R.library_graph(N, ev, 'cpu'), t(src[:3]), t(ts[:3], torch.float64), 16)
    out = hip_ops.walk_candidates(g, t(src[:0]), t(ts[:0], torch.float64), 16)
    assert out['ids'].shape == (0, 16) and out['ids'].device.type == 'cuda' and out['n_distinct'].shape == (0,)


# ---- the grid cap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', (R.Q_WALK_AT, R.Q_WALK_PAST), ids=('at-the-cap', 'past-the-cap'))
def test_at_and_past_the_grid_cap(B):
    """one workgroup per query up to the cap; past it the first five workgroups take a second query each - the last five
    queries, ordinary non-empty ones.  Every row against the host twin, the last five and a sample against the reference."""
    N, src, dst, ts, eids = _cap_ref.small_graph()
    ev = (src, dst, ts, eids)
    q, qt = _cap_ref.queries(N, B, float(ts.max()), seed=B % 1000)
    fanout, take = R.DEFAULT
    got = R.library_rows(R.library_graph(N, ev, dev()), q, qt, 64, fanout, take, dev(), exclude_seen=True)
    host = R.library_rows(R.library_graph(N, ev, 'cpu'), q, qt, 64, fanout, take, 'cpu', exclude_seen=True)
    R.assert_same(got, {k: v.numpy() for k, v in host.items()}, f'B={B}')
    rows = np.r_[np.random.RandomState(3).choice(B - 5, 60, replace=False), B - 5:B]
    want = R.WalkRef(N, src, dst, ts).rows(q[rows], qt[rows], 64, fanout, take, exclude_seen=True)
    R.assert_same({k: v[t(rows)] for k, v in got.items()}, want, f'B={B}, the checked rows')
    assert (want['n_distinct'][-5:] > 0).all()


# ---- the model side ----------------------------------------------------------------------------------------------------------
WALK = dict(fanout=(10, 10, 10), take=(True, False, True))


def stream_ref(st):
    return R.WalkRef(st['n_nodes'], st['src'], st['dst'], st['ts'])


def test_recommend_walk_is_recommend_over_the_walk_ids():
    from www2023tiger_amd import hip_ops
    model, orc, st = build(D, D, K, 'bin', seed=D + K)
    warm(model, orc, st, K, with_oracle=False)
    lo = WARM[-1] + 40
    src, _, _, ts, _ = batch(st, lo, lo + 32)
    before = state_of(model)
    ids, scores, n_valid, cand = model.recommend_walk(t(src), t(ts, torch.float64), 5, C=12, exclude_seen=True, **WALK)
    R.assert_same(cand, stream_ref(st).rows(src, ts, 12, WALK['fanout'], WALK['take'], exclude_seen=True), 'the walk of recommend_walk')
    assert int(cand['n_valid'].max()) > 5 and int(cand['n_valid'].min()) == 0    # rows longer than k, rows without a candidate
    two = hip_ops.walk_candidates(model.graph, t(src), t(ts, torch.float64), 12, exclude_seen=True, **WALK)
    want = model.recommend(t(src), t(ts, torch.float64), two['ids'], 5)
    assert torch.equal(ids, want[0]) and torch.equal(scores.view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(n_valid, want[2]) and torch.equal(n_valid, cand['n_valid'])    # the padding id 0 is left out
    assert (ids != 0).sum() == n_valid.clamp(max=5).sum() and int(n_valid.sum()) > 0
    assert_same_state(before, state_of(model))
    # chunked; with the defaults
    parts = model.recommend_walk(t(src), t(ts, torch.float64), 5, C=12, exclude_seen=True, chunk_queries=13, **WALK)
    assert torch.equal(parts[0], ids) and torch.equal(parts[1], scores)
    wide = model.recommend_walk(t(src), t(ts, torch.float64), 5)
    assert wide[3]['ids'].shape == (32, 256)
    assert all(torch.equal(a, b) for a, b in zip(wide[:3], model.recommend(t(src), t(ts, torch.float64), wide[3]['ids'], 5)))


def test_recommend_walk_with_uptodate_restarts_what_the_two_calls_restart():
    from www2023tiger_amd import hip_ops
    (A, _, st), (B, _, _) = (build(D, D, K, 'bin', seed=5) for _ in range(2))
    src, ts = t(st['src'][-40:]), t(st['ts'][-40:], torch.float64)
    bm_a, bm_b = (hip_ops.new_bitmap(st['n_nodes'], dev()) for _ in range(2))
    a = A.recommend_walk(src, ts, 5, C=16, uptodate=bm_a, **WALK)
    cand = hip_ops.walk_candidates(B.graph, src, ts, 16, **WALK)
    b = B.recommend(src, ts, cand['ids'], 5, uptodate=bm_b)
    assert A.last_restarted == B.last_restarted > 0 and torch.equal(bm_a, bm_b)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b)) and torch.equal(a[3]['ids'], cand['ids'])
    assert_same_state(state_of(A), state_of(B))
    A.recommend_walk(src, ts, 5, C=16, uptodate=bm_a, **WALK)
    assert A.last_restarted == 0


def loop_over_the_reference(model, st, walk, Cn, k, exclude_seen, bm=None):
    """per batch: the REFERENCE generator, [the restart over cat[src, dst, neg] and the candidates,] recommend, the batch
    -> (positions, covered) per event"""
    ref = stream_ref(st)
    positions, covered, lo = [], [], 0
    with torch.no_grad():
        for src, dst, neg, ts, eids, _, cg in loader(model, st, K):
            B = len(src)
            s_np, t_np, d_np = st['src'][lo:lo + B], st['ts'][lo:lo + B], st['dst'][lo:lo + B]
            assert np.array_equal(s_np, src.cpu().numpy())
            cand = ref.rows(s_np, t_np, Cn, walk['fanout'], walk['take'], exclude_seen=exclude_seen)['ids']
            src, dst, neg = src.to(dev()), dst.to(dev()), neg.to(dev())
            if bm is not None:
                t64 = t(t_np, torch.float64)
                model.restart_involved(torch.cat([src, dst, neg, t(cand).reshape(-1)]),
                                       torch.cat([t64.repeat(3), t64.repeat_interleave(Cn)]), bm)
            ids = model.recommend(src, cg.ts64, t(cand), k)[0].cpu().numpy()
            hit = (ids == d_np[:, None]) & (ids != 0)
            positions.append(np.where(hit.any(1), hit.argmax(1), -1))
            covered.append(((cand == d_np[:, None]) & (cand != 0)).any(1))
            model.contrast_learning(src, dst, neg, ts.to(dev()), eids.to(dev()), cg)
            lo += B
    return np.concatenate(positions), np.concatenate(covered)


@pytest.mark.parametrize('exclude_seen', (False, True), ids=('all-items', 'exclude-seen'))
def test_eval_recommendation_over_walk_candidates_equals_the_loop(exclude_seen):
    from www2023tiger_amd.eval_utils import eval_recommendation
    k, E, Cn = 5, 150, 8
    (A, _, st), (B, _, _) = (build(D, D, K, 'bin', seed=3, E=E) for _ in range(2))
    out = eval_recommendation(A, loader(A, st, K), dev(), walk=dict(WALK, C=Cn), k=k, exclude_seen=exclude_seen,
                              return_positions=True)
    pos, covered = loop_over_the_reference(B, st, WALK, Cn, k, exclude_seen)
    np.testing.assert_array_equal(out['positions'].cpu().numpy(), pos)
    assert out['n_events'] == E and abs(out['coverage'] - covered.mean()) < 1e-12
    hit = pos >= 0
    print(f'exclude_seen={exclude_seen}: recall@{Cn} {out["coverage"]:.4f}, hit_rate {out["hit_rate"]:.4f}')
    assert 0 < covered.sum() < E and hit.any() and (covered | ~hit).all()      # listed only where the generator recalled it
    assert abs(out['hit_rate'] - hit.mean()) < 1e-12
    assert abs(out['ndcg'] - np.where(hit, 1.0 / np.log2(np.maximum(pos, 0) + 2.0), 0.0).mean()) < 1e-12
    assert abs(out['mrr_at_k'] - np.where(hit, 1.0 / (np.maximum(pos, 0) + 1.0), 0.0).mean()) < 1e-12
    assert_same_state(state_of(A), state_of(B))


def test_eval_recommendation_walk_with_lazy_restarts_equals_the_loop():
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.eval_utils import eval_recommendation
    k, E, Cn = 5, 150, 8
    (A, _, st), (B, _, _) = (build(D, D, K, 'bin', seed=3, E=E) for _ in range(2))
    upto = set()
    out = eval_recommendation(A, loader(A, st, K), dev(), walk=dict(WALK, C=Cn), k=k, lazy_restarts=True, uptodate_nodes=upto,
                              return_positions=True)
    bm = hip_ops.new_bitmap(st['n_nodes'], dev())
    pos, covered = loop_over_the_reference(B, st, WALK, Cn, k, False, bm=bm)
    np.testing.assert_array_equal(out['positions'].cpu().numpy(), pos)
    assert abs(out['coverage'] - covered.mean()) < 1e-12
    comp = hip_ops.unique_compact(bm, st['n_nodes'], st['n_nodes'])
    assert upto == set(comp['ids'][:int(comp['count'].item())].tolist()) and len(upto) > 0
    assert_same_state(state_of(A), state_of(B))


def test_walk_refusals_come_before_anything_runs():
    from www2023tiger_amd.data.graph import Graph
    from www2023tiger_amd.eval_utils import eval_recommendation
    m, orc, st = build(D, D, K, 'bin', seed=D + K)
    warm(m, orc, st, K, with_oracle=False)
    src, ts = t(st['src'][-3:]), t(st['ts'][-3:], torch.float64)
    before = state_of(m)
    cat = np.arange(1, st['n_nodes'], dtype=np.int64)
    with pytest.raises(ValueError, match='walk'):
        eval_recommendation(m, None, dev(), cat, walk=dict(C=8))
    with pytest.raises(ValueError, match='walk'):
        eval_recommendation(m, None, dev(), walk=dict(C=8), catalogue_at='batch')
    with pytest.raises(ValueError, match='walk'):
        eval_recommendation(m, None, dev())
    with pytest.raises(ValueError, match="'C'"):
        eval_recommendation(m, None, dev(), walk=dict(fanout=(3, 3, 3)))
    with pytest.raises(ValueError, match='TG_WALK_MAX_FANOUT'):
        eval_recommendation(m, None, dev(), walk=dict(C=8, fanout=(65, 3, 3)))
    with pytest.raises(NotImplementedError, match='restart'):
        eval_recommendation(m, None, dev(), walk=dict(C=8), restart_mode=True)
    with pytest.raises(ValueError, match='k <='):
        m.recommend_walk(src, ts, 0)
    with pytest.raises(ValueError, match='TG_WALK_MAX_ENDPOINTS'):
        m.recommend_walk(src, ts, 3, C=4096)
    uni = Graph.from_arrays(st['src'], st['dst'], st['ts'], st['eids'], strategy='uniform', seed=0,
                            max_node_id=st['n_nodes'] - 1, device=dev())
    with pytest.raises(NotImplementedError, match='uniform'):
        m.recommend_walk(src, ts, 3, graph=uni)
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        m.recommend_walk(src, ts, 3)
    m.eval()
    assert_same_state(before, state_of(m))
    n = st['n_nodes']
    m.partition_state(torch.arange(n, dtype=torch.int32), n)
    with pytest.raises(RuntimeError, match='partitioned'):
        m.recommend_walk(src, ts, 3)
    with pytest.raises(RuntimeError, match='partitioned'):
        eval_recommendation(m, None, dev(), walk=dict(C=8))


def test_without_a_walk_eval_recommendation_is_what_it_was():
    """walk=None: the catalogue path, positional as before and by keyword - two calls on twin models, compared"""
    from www2023tiger_amd.eval_utils import eval_recommendation
    (A, _, st), (B, _, _) = (build(D, D, K, 'bin', seed=3, E=150) for _ in range(2))
    cat = np.arange(1, st['n_nodes'], dtype=np.int64)
    a = eval_recommendation(A, loader(A, st, K), dev(), cat, k=10, exclude_seen=True, return_positions=True)
    b = eval_recommendation(B, loader(B, st, K), dev(), catalogue=cat, walk=None, k=10, exclude_seen=True, return_positions=True)
    assert torch.equal(a.pop('positions'), b.pop('positions')) and a == b and a['n_events'] == 150
    assert_same_state(state_of(A), state_of(B))
