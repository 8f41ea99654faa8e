"""tg_trending and tg_fill_candidates on the GPU, exactly.  Three groups: every host case of tests/test_trend_host.py through
the kernels, against the host twins and the numpy reference of tests/_trend_ref.py; the launches past their grid caps and
through every merge round; and the model side - TIGE.recommend_walk(fill=...) and eval_recommendation(walk=dict(fill=...))
on the small model of tests/test_hip_rank.py against the three hip_ops calls and a numpy loop over the REFERENCE.  Integer
work and bit-equal scores: no tolerance."""
import numpy as np
import pytest
import torch

import _cap_ref
import _trend_ref as R
import _walk_ref as W
import test_trend_host as H
from test_hip_rank import WARM, assert_same_state, batch, build, dev, loader, state_of, warm

pytestmark = pytest.mark.gpu
D, K = 16, 10
WALK = dict(fanout=(10, 10, 10), take=(True, False, True))


def t(x, dt=torch.int64):
    return torch.as_tensor(x).to(dev(), dt)


# ---- the host cases on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', R.MS)
def test_trending_among_lists_of_every_size(M):
    H.check_among_sizes(M, dev())


def test_trending_windows():
    H.check_windows(dev())


def test_trending_ties_across_a_tile_edge():
    H.check_ties(dev())


def test_trending_degrees_at_the_probe_rounds():
    H.check_degrees(dev())


def test_trending_on_trimmed_and_extended_graphs():
    H.check_derived_graphs(dev())


@pytest.mark.parametrize('T', R.FILL_TS)
@pytest.mark.parametrize('Cn', R.FILL_CS)
def test_fill_equals_the_host_twin_and_the_reference(Cn, T):
    H.check_fill(Cn, T, dev())


def test_fill_special_rows():
    H.check_fill_special(dev())


@pytest.mark.parametrize('n', W.SWEEP_PREFIXES)
def test_fill_exclude_seen_sweeps_the_whole_prefix(n):
    H.check_fill_sweep(n, dev())


def test_fill_power_of_two_strides_fill_the_table():
    H.check_fill_strides(dev())


def test_refusals_on_the_device():
    from www2023tiger_amd import hip_ops
    N, ev, _ = R.wide_case()
    g = W.library_graph(N, ev, dev())
    with pytest.raises(ValueError, match='among.*duplicate'):
        hip_ops.trending(g, 10.0, 16, among=t([3, 4, 3]))
    with pytest.raises(ValueError, match='lives on'):                  # a host graph, a device list
        hip_ops.trending(W.library_graph(N, ev, 'cpu'), 10.0, 16, among=t([3, 4]))
    s, ts = t([1, 2, 3]), t([50.0] * 3, torch.float64)
    cand, trend = hip_ops.walk_candidates(g, s, ts, 8), hip_ops.trending(g, 50.0, 16)
    assert trend['ids'].device.type == 'cuda' and int(trend['n_valid']) == 16
    with pytest.raises(ValueError, match='source id'):
        hip_ops.fill_candidates(g, t([1, N, 2]), ts, cand, trend)
    with pytest.raises(ValueError, match='live on'):
        hip_ops.fill_candidates(g, s, ts, cand, {k: v.cpu() for k, v in trend.items()})
    none = hip_ops.fill_candidates(g, s[:0], ts[:0], {k: v[:0] for k, v in cand.items()}, trend)
    assert none['ids'].shape == (0, 8) and none['n_filled'].shape == (0,)


# ---- past the grid caps, through the merge rounds ----------------------------------------------------------------------------
def sparse_trending(N, ev, t_lo, t_hi, T):
    """the contract over an event list whose nodes are mostly idle: one bincount instead of a row per node"""
    src, dst, ts = ev[:3]
    inside = (ts >= t_lo) & (ts < t_hi)
    c = np.bincount(np.concatenate([src[inside], dst[inside]]), minlength=N)
    c[0] = 0
    best = sorted(np.flatnonzero(c).tolist(), key=lambda v: (-c[v], v))
    k = min(T, len(best))
    ids, counts = np.zeros(T, np.int64), np.zeros(T, np.int32)
    ids[:k], counts[:k] = best[:k], [c[v] for v in best[:k]]
    return dict(ids=ids, counts=counts, n_valid=np.array([k], np.int32), n_distinct=np.array([len(best)], np.int32))


def spread_events(N, seed):
    """the small graph's events plus 600 between nodes spread over all N ids, the last five ids among them"""
    _, src, dst, ts, _ = _cap_ref.small_graph()
    rs = np.random.RandomState(seed)
    far = np.r_[rs.randint(400, N, 1190), np.arange(N - 5, N), np.arange(N - 5, N)].astype(np.int64)
    s2, d2 = far[:600], far[600:]
    t2 = np.floor(rs.uniform(0, float(ts.max()), 600))
    src, dst, ts = np.r_[src, s2], np.r_[dst, d2], np.r_[ts, t2]
    order = np.argsort(ts, kind='stable')
    return src[order], dst[order], ts[order], np.arange(1, len(ts) + 1, dtype=np.int64)


# N: one 16-lane pass past the key kernel's grid (33 tiles: two merge rounds, the second over 3 runs); 600 000 nodes: 293
# tiles, three merge rounds with ragged last groups
@pytest.mark.parametrize('N', (R.N_KEYS_PAST, 600000), ids=('past-the-key-grid', 'three-merge-rounds'))
def test_trending_over_every_node_past_the_key_grid(N):
    ev = spread_events(N, seed=N % 1000)
    t_hi = float(ev[2].max()) * 0.75
    g_dev, g_host = W.library_graph(N, ev, dev()), W.library_graph(N, ev, 'cpu')
    for T, window in ((256, None), (2048, 400.0), (1, None)):
        t_lo = -np.inf if window is None else t_hi - window
        want = sparse_trending(N, ev, t_lo, t_hi, T)
        R.assert_same(R.library_trending(g_dev, t_hi, T, dev(), window), want, f'N={N} T={T}')
        R.assert_same(R.library_trending(g_host, t_hi, T, 'cpu', window), want, f'N={N} T={T} (host twin)')
        assert want['n_distinct'][0] > 300 and (want['ids'][:want['n_valid'][0]] >= 400).any() == (T == 2048)
    if N == R.N_KEYS_PAST:
        ref = W.WalkRef(N, *ev[:3])
        R.assert_same(R.library_trending(g_dev, t_hi, 2048, dev(), 400.0), R.trending(ref, t_hi, 2048, 400.0), 'the row reference')
    late = sparse_trending(N, ev, -np.inf, float(ev[2].max()) + 1, 2048)
    assert set(range(N - 5, N)) <= set(late['ids'].tolist())          # the second pass's nodes are listed
    R.assert_same(R.library_trending(g_dev, float(ev[2].max()) + 1, 2048, dev()), late, f'N={N}, everything')


def test_fill_past_the_grid_cap():
    """one workgroup per query up to the cap; past it the first five workgroups serve a second query each - the last five,
    ordinary non-empty ones - with the table they built for their first and freshly cleared flags"""
    from www2023tiger_amd import hip_ops
    B, Cn, T = R.B_FILL_PAST, 64, 64
    N, src, dst, ts, eids = _cap_ref.small_graph()
    ev = (src, dst, ts, eids)
    q, qt = _cap_ref.queries(N, B, float(ts.max()), seed=B % 1000)
    ref = W.WalkRef(N, src, dst, ts)
    g_host = W.library_graph(N, ev, 'cpu')
    rows = W.library_rows(g_host, q, qt, Cn, *W.DEFAULT, 'cpu', exclude_seen=True)
    cand = {k: v.numpy() for k, v in rows.items()}
    trend = R.trending(ref, float(np.median(ts)), T, 200.0)
    want = R.fill(ref, q, qt, cand, trend['ids'], int(trend['n_valid'][0]), exclude_seen=True)
    got = R.library_fill(W.library_graph(N, ev, dev()), q, qt, cand, trend['ids'], int(trend['n_valid'][0]), dev(), exclude_seen=True)
    R.assert_same(got, want, f'B={B}', R.FILL_NAMES)
    R.assert_same(R.library_fill(g_host, q, qt, cand, trend['ids'], int(trend['n_valid'][0]), 'cpu', exclude_seen=True), want,
                  f'B={B} (host twin)', R.FILL_NAMES)
    # the second pass: rows with walk candidates, two of them short and filled, three full and left alone; and the same
    # workgroups' first queries were filled too
    assert (cand['n_valid'][-5:] > 0).all() and (want['n_filled'][-5:] > 0).sum() == 2 and (want['n_filled'][:5] > 0).sum() == 3
    assert (want['n_filled'] == 0).any() and (want['n_valid'] < Cn).any() and (want['n_valid'] == Cn).any()


# ---- the model side ----------------------------------------------------------------------------------------------------------
def stream_ref(st):
    return W.WalkRef(st['n_nodes'], st['src'], st['dst'], st['ts'])


def queries_with_a_cold_source(st, B=32):
    lo = WARM[-1] + 40
    src, _, _, ts, _ = batch(st, lo, lo + B)
    src, ts = src.copy(), ts.copy()
    known = set(st['src'][:lo + B].tolist()) | set(st['dst'][:lo + B].tolist())
    cold = [v for v in range(1, st['n_nodes']) if v not in known]
    assert cold
    src[3] = cold[0]
    return src, ts, 3


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])


def test_recommend_walk_with_fill_is_recommend_over_the_filled_ids():
    from www2023tiger_amd import hip_ops
    model, orc, st = build(D, D, K, 'bin', seed=D + K, n_u=150)
    warm(model, orc, st, K, with_oracle=False)
    src, ts, cold = queries_with_a_cold_source(st)
    s, tt = t(src), t(ts, torch.float64)
    before = state_of(model)
    ids, scores, n_valid, cand = model.recommend_walk(s, tt, 5, C=24, fill=dict(T=64), exclude_seen=True, **WALK)
    # the three hip_ops calls
    rows = hip_ops.walk_candidates(model.graph, s, tt, 24, exclude_seen=True, **WALK)
    trend = hip_ops.trending(model.graph, float(ts.min()), 64)
    filled = hip_ops.fill_candidates(model.graph, s, tt, rows, trend, exclude_seen=True)
    for name in ('ids', 'counts', 'n_valid', 'n_filled', 'n_distinct'):
        assert torch.equal(cand[name], filled[name]), name
    assert same((ids, scores, n_valid), model.recommend(s, tt, filled['ids'], 5))
    # ... and the reference
    ref = stream_ref(st)
    want_rows = ref.rows(src, ts, 24, WALK['fanout'], WALK['take'], exclude_seen=True)
    want_trend = R.trending(ref, float(ts.min()), 64)
    R.assert_same(cand, R.fill(ref, src, ts, want_rows, want_trend['ids'], int(want_trend['n_valid'][0]), exclude_seen=True),
                  'the fill of recommend_walk', R.FILL_NAMES)
    assert int(rows['n_valid'][cold]) == 0 and int(cand['n_filled'][cold]) > 0 and int(n_valid[cold]) > 0 and int(ids[cold, 0]) != 0
    assert_same_state(before, state_of(model))
    # fill=None is the walk alone, as before
    plain = model.recommend_walk(s, tt, 5, C=24, fill=None, exclude_seen=True, **WALK)
    assert same(plain[:3], model.recommend(s, tt, rows['ids'], 5)) and 'n_filled' not in plain[3]
    assert all(torch.equal(plain[3][k], rows[k]) for k in rows) and int(plain[2][cold]) == 0
    # a window, an explicit time and list; chunked
    kw = dict(T=16, window=800.0, t=float(ts.min()) - 1.0, among=np.unique(st['dst']))
    a = model.recommend_walk(s, tt, 5, C=24, fill=kw, **WALK)
    tr = hip_ops.trending(model.graph, kw['t'], 16, window=800.0, among=t(kw['among']))
    b = hip_ops.fill_candidates(model.graph, s, tt, hip_ops.walk_candidates(model.graph, s, tt, 24, **WALK), tr)
    assert torch.equal(a[3]['ids'], b['ids']) and same(a[:3], model.recommend(s, tt, b['ids'], 5))
    assert same(model.recommend_walk(s, tt, 5, C=24, fill=kw, chunk_queries=13, **WALK)[:3], a[:3])
    with pytest.raises(ValueError, match='TG_TREND_MAX'):
        model.recommend_walk(s, tt, 5, fill=dict(T=0))
    with pytest.raises(ValueError, match="'T'"):
        model.recommend_walk(s, tt, 5, fill=dict(window=5.0))
    with pytest.raises(ValueError, match='fill takes'):
        model.recommend_walk(s, tt, 5, fill=dict(T=4, C=3))
    assert_same_state(before, state_of(model))


def test_recommend_walk_with_fill_on_a_snapshot_is_the_subset_form_over_the_filled_ids():
    from www2023tiger_amd import hip_ops
    model, orc, st = build(D, D, K, 'bin', seed=D + K, n_u=150)
    warm(model, orc, st, K, with_oracle=False)
    src, ts, cold = queries_with_a_cold_source(st)
    s, tt = t(src), t(ts, torch.float64)
    items = t(np.unique(st['dst'])[::2].astype(np.int64))
    snap = model.embed_catalogue(items, float(ts.min()))
    before = state_of(model)
    ids, scores, n_valid, cand = model.recommend_walk(s, tt, 5, C=24, snapshot=snap, fill=dict(T=64), **WALK)
    rows = hip_ops.walk_candidates(model.graph, s, tt, 24, **WALK)
    trend = hip_ops.trending(model.graph, float(ts.min()), 64, among=items)       # among defaults to the snapshot's ids
    filled = hip_ops.fill_candidates(model.graph, s, tt, rows, trend)
    assert torch.equal(cand['ids'], filled['ids']) and torch.equal(cand['n_filled'], filled['n_filled'])
    assert same((ids, scores, n_valid), model.recommend_subset(s, tt, snap, 5, filled['ids']))
    assert bool(torch.isin(trend['ids'][:int(trend['n_valid'])], items).all()) and int(trend['n_valid']) > 0
    assert int(n_valid[cold]) > 0 and int(ids[cold, 0]) != 0 and 'n_in_catalogue' in cand
    assert_same_state(before, state_of(model))


def reference_recalls(st, Cn, T, window, exclude_seen, bs=50):
    ref = stream_ref(st)
    E = len(st['src'])
    walked, covered, n_filled, n_all = [], [], 0, 0
    for lo in range(0, E, bs):
        s, d, ts = (st[k][lo:lo + bs] for k in ('src', 'dst', 'ts'))
        rows = ref.rows(s, ts, Cn, WALK['fanout'], WALK['take'], exclude_seen=exclude_seen)
        trend = R.trending(ref, float(ts.min()), T, window)
        full = R.fill(ref, s, ts, rows, trend['ids'], int(trend['n_valid'][0]), exclude_seen=exclude_seen)
        walked.append(((rows['ids'] == d[:, None]) & (rows['ids'] != 0)).any(1))
        covered.append(((full['ids'] == d[:, None]) & (full['ids'] != 0)).any(1))
        n_filled, n_all = n_filled + int(full['n_filled'].sum()), n_all + int(full['n_valid'].sum())
    return np.concatenate(walked), np.concatenate(covered), n_filled, n_all


@pytest.mark.parametrize('exclude_seen', (False, True), ids=('all-items', 'exclude-seen'))
def test_eval_recommendation_with_fill_reports_the_reference_recalls(exclude_seen):
    from test_hip_walk import loop_over_the_reference
    from www2023tiger_amd.eval_utils import eval_recommendation
    k, E, Cn, T, window = 5, 150, 32, 32, 1500.0
    (A, _, st), (B, _, _), (Cm, _, _) = (build(D, D, K, 'bin', seed=3, E=E) for _ in range(3))
    out = eval_recommendation(A, loader(A, st, K), dev(), walk=dict(WALK, C=Cn, fill=dict(T=T, window=window)), k=k,
                              exclude_seen=exclude_seen)
    walked, covered, n_filled, n_all = reference_recalls(st, Cn, T, window, exclude_seen)
    print(f'exclude_seen={exclude_seen}: coverage_walk {out["coverage_walk"]:.4f} -> coverage {out["coverage"]:.4f}, '
          f'filled {out["filled"]:.4f}')
    assert set(out) == {'hit_rate', 'ndcg', 'mrr_at_k', 'n_events', 'coverage', 'coverage_walk', 'filled'}
    assert out['coverage'] == covered.sum() / E and out['coverage_walk'] == walked.sum() / E and out['n_events'] == E
    assert out['coverage'] >= out['coverage_walk'] and (covered | ~walked).all()
    assert out['filled'] == n_filled / n_all and 0 < out['filled'] <= 1
    assert out['hit_rate'] <= out['coverage']
    # without fill: the keys and values of the walk alone
    plain = eval_recommendation(B, loader(B, st, K), dev(), walk=dict(WALK, C=Cn), k=k, exclude_seen=exclude_seen,
                                return_positions=True)
    pos, cov = loop_over_the_reference(Cm, st, WALK, Cn, k, exclude_seen)
    np.testing.assert_array_equal(plain.pop('positions').cpu().numpy(), pos)
    hit = pos >= 0
    assert set(plain) == {'hit_rate', 'ndcg', 'mrr_at_k', 'n_events', 'coverage'}
    assert abs(plain['coverage'] - cov.mean()) < 1e-12 and abs(plain['hit_rate'] - hit.mean()) < 1e-12
    assert abs(plain['ndcg'] - np.where(hit, 1.0 / np.log2(np.maximum(pos, 0) + 2.0), 0.0).mean()) < 1e-12
    assert abs(plain['mrr_at_k'] - np.where(hit, 1.0 / (np.maximum(pos, 0) + 1.0), 0.0).mean()) < 1e-12
    assert plain['coverage'] == out['coverage_walk']
    assert_same_state(state_of(A), state_of(B))                  # the batches advance the state alike


def test_eval_recommendation_with_fill_on_a_catalogue():
    """walk['catalogue'] + fill: among defaults to the catalogue, the filled rows are ranked on the batch's snapshot"""
    from www2023tiger_amd.eval_utils import eval_recommendation
    E = 150
    A, _, st = build(D, D, K, 'bin', seed=3, E=E)
    cat = np.unique(st['dst']).astype(np.int64)
    out = eval_recommendation(A, loader(A, st, K), dev(), walk=dict(WALK, C=32, catalogue=cat, fill=dict(T=32)), k=5)
    ref = stream_ref(st)
    covered = []
    for lo in range(0, E, 50):
        s, d, ts = (st[k][lo:lo + 50] for k in ('src', 'dst', 'ts'))
        rows = ref.rows(s, ts, 32, WALK['fanout'], WALK['take'])
        trend = R.trending(ref, float(ts.min()), 32, None, cat)
        full = R.fill(ref, s, ts, rows, trend['ids'], int(trend['n_valid'][0]))
        covered.append(((full['ids'] == d[:, None]) & (full['ids'] != 0)).any(1))
    assert out['coverage'] == np.concatenate(covered).sum() / E and 'in_catalogue' in out and out['coverage'] >= out['coverage_walk']
    with pytest.raises(ValueError, match="no 't'"):
        eval_recommendation(A, None, dev(), walk=dict(C=8, fill=dict(T=8, t=3.0)))
