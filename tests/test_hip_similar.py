"""Embedding nearest neighbours at the model level, on the GPU: TIGE.similar_items / similar_items_keys (tg_knn_rows on a
catalogue snapshot's own rows), TIGE.recommend_similar (retrieve in embedding space, rank with the score head) and
eval_recommendation(similar=...), on the small model of tests/test_hip_rank.py (d = 16, K = 6, about 40 items).  Every
comparison is exact: the lists equal tg_topk_rows on the host twin's matrix of the snapshot's rows, and recommend_similar
equals recommend_subset on the candidates it returns.  (Fails without the feature: none of the methods exists.)"""
import numpy as np
import pytest
import torch

from test_hip_rank import WARM, assert_same_state, batch, build, dev, loader, state_of
from test_hip_walk_snapshot import at_one_time, same, snapshot_tensors, t, warmed

pytestmark = pytest.mark.gpu
D, K = 16, 6
_M = {}


def shared():
    """one warmed 'bin' model, the queries of one time, and two snapshots at that time: `snap` of every node id but the
    padding id (75 rows: more than two 32-column blocks), `snap_items` of the destination nodes alone (15 rows)"""
    if not _M:
        model, st = warmed('bin')
        src, ts, when = at_one_time(st, 9)
        cat = t(np.arange(1, st['n_nodes'], dtype=np.int64))
        items = t(np.unique(st['dst']).astype(np.int64))
        snap, snap_items = model.embed_catalogue(cat, when), model.embed_catalogue(items, when)
        _M.update(model=model, st=st, src=src, ts=ts, when=when, cat=cat, snap=snap, snap_items=snap_items,
                  before=state_of(model))
    return _M


def twin_lists(snap, items, k, metric, exclude_self, mask=None):
    """tg_topk_rows (host) on the host twin's full matrix of the snapshot's rows, with the mask row the header states"""
    from www2023tiger_amd import hip_ops
    h, ids = snap.h.cpu(), snap.ids.cpu()
    col = snap.col_of.cpu()[items.cpu()].long()
    inv = snap.inv_norm.cpu() if metric == 'cos' else None
    S = torch.empty(len(items), len(ids))
    hip_ops.knn_rows(h[col], h, k, ids=ids, q_scale=None if inv is None else inv[col], c_scale=inv, _scores_out=S)
    m = torch.ones(len(items), len(ids), dtype=torch.bool)
    if exclude_self:
        m &= ids[None, :] != items.cpu()[:, None]
    if mask is not None:
        m &= mask.cpu()[None, :]
    return hip_ops.topk_rows(S, ids, k, mask=m)


@pytest.mark.parametrize('metric', ['cos', 'ip'])
@pytest.mark.parametrize('exclude_self', [True, False], ids=['no-self', 'self'])
def test_similar_items_equals_topk_rows_on_the_twins_matrix(metric, exclude_self):
    b = shared()
    m, snap = b['model'], b['snap']
    items = snap.ids[torch.arange(0, len(snap), 3, device=dev())]
    frozen = snapshot_tensors(snap)
    for k, mask in ((5, None), (64, None), (7, torch.arange(len(snap), device=dev()) % 3 != 1)):
        ids, scores, n_valid = m.similar_items(items, snap, k, metric=metric, exclude_self=exclude_self, mask=mask)
        want = twin_lists(snap, items, k, metric, exclude_self, mask)
        assert torch.equal(ids.cpu(), want['ids']) and torch.equal(n_valid.cpu(), want['n_valid'])
        assert torch.equal(scores.cpu().view(torch.int32), want['scores'].view(torch.int32))
        assert int(n_valid.min()) > 5
        if exclude_self:
            assert not bool((ids == items[:, None]).any())
    if metric == 'cos':   # the cosine of an item with itself rounds to 1: it leads its own list
        ids, scores, _ = m.similar_items(items, snap, 1, metric='cos', exclude_self=False)
        assert bool((scores > 0.9999).all())
    assert_same_state(b['before'], state_of(m))
    after = snapshot_tensors(snap)
    assert all(torch.equal(frozen[n], after[n]) for n in frozen)


def test_inv_norm_is_the_float64_reciprocal_norm_rounded_once():
    b = shared()
    snap = b['snap']
    h64 = snap.h.cpu().numpy().astype(np.float64)
    n = np.sqrt((h64 * h64).sum(1))
    want = np.where((n > 0) & np.isfinite(n), 1.0 / np.where(n > 0, n, 1.0), 0.0).astype(np.float32)
    got = snap.inv_norm.cpu().numpy()
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= np.spacing(want).max()   # (sqrt / sum order)
    assert snap.inv_norm is snap.inv_norm   # cached


def test_similar_items_refusals():
    b = shared()
    m, st, snap = b['model'], b['st'], b['snap_items']
    users = t(np.unique(st['src']).astype(np.int64)[:2])
    with pytest.raises(ValueError, match=f'item {int(users[0])} '):
        m.similar_items(torch.cat([snap.ids[:1], users]), snap, 3)              # not in the snapshot: the first offender
    with pytest.raises(ValueError, match='item 0 '):
        m.similar_items(torch.cat([snap.ids[:2], t([0])]), snap, 3)
    with pytest.raises(ValueError, match=f'item {st["n_nodes"]} '):
        m.similar_items(t([st['n_nodes']]), snap, 3)
    with pytest.raises(ValueError, match='metric'):
        m.similar_items(snap.ids[:2], snap, 3, metric='l2')
    with pytest.raises(ValueError, match='64'):
        m.similar_items(snap.ids[:2], snap, 65)
    with pytest.raises(ValueError, match='mask'):
        m.similar_items(snap.ids[:2], snap, 3, mask=torch.ones(3, dtype=torch.bool))
    other, _ = warmed('bin', seed=5)
    with pytest.raises(ValueError, match='another model'):
        other.similar_items(snap.ids[:2], snap, 3)
    assert_same_state(b['before'], state_of(m))


def test_a_stale_snapshot_is_refused_unless_stale_ok():
    model, st = warmed('bin', seed=7)
    src, ts, when = at_one_time(st, 9)
    cat = t(np.unique(st['dst']).astype(np.int64))
    snap = model.embed_catalogue(cat, when)
    fresh = model.similar_items(cat[:4], snap, 3)
    model.stream_step(*batch(st, WARM[-1], WARM[-1] + 5))   # the state moves on: the snapshot's stamp no longer matches
    late = ts + 1.0e6
    with pytest.raises(RuntimeError, match='stale'):
        model.similar_items(cat[:4], snap, 3)
    with pytest.raises(RuntimeError, match='stale'):
        model.recommend_similar(src, late, snap, 3, S=8)
    assert same(model.similar_items(cat[:4], snap, 3, stale_ok=True), fresh)   # items as of the snapshot


def test_similar_items_keys_round_trips_through_an_id_map():
    from www2023tiger_amd.data.idmap import IdMap
    b = shared()
    m, st, snap = b['model'], b['st'], b['snap_items']
    idmap = IdMap(dev(), capacity=1024)
    keys = torch.arange(1, st['n_nodes'], device=dev(), dtype=torch.int64) * 1000 + 7    # node id i <-> key 1000 i + 7
    assert idmap.assign(keys).tolist() == list(range(1, st['n_nodes']))
    items = snap.ids[:6]
    got_keys, scores, n_valid = m.similar_items_keys(idmap, items * 1000 + 7, snap, 64, metric='ip')
    ids, scores2, n_valid2 = m.similar_items(items, snap, 64, metric='ip')
    assert int(n_valid.min()) < 64   # padding is present
    want_keys = torch.where(ids != 0, ids * 1000 + 7, torch.full_like(ids, -(1 << 63)))
    assert torch.equal(got_keys, want_keys) and torch.equal(n_valid, n_valid2)
    assert torch.equal(scores.view(torch.int32), scores2.view(torch.int32))
    with pytest.raises(ValueError, match='1 of the 2'):
        m.similar_items_keys(idmap, torch.stack([items[0] * 1000 + 7, items[0] * 1000 + 8]), snap, 3)


def test_recommend_similar_is_recommend_subset_on_the_candidates_it_returns():
    from www2023tiger_amd import _lib, hip_ops
    b = shared()
    m, st, snap, src, ts = b['model'], b['st'], b['snap'], b['src'], b['ts']
    for metric in ('cos', 'ip'):
        ids, scores, n_valid, cand = m.recommend_similar(src, ts, snap, 5, S=12, metric=metric)
        seeds = hip_ops.walk_candidates(m.graph, src, ts, 1, fanout=(1,), take=(True,))['ids'].reshape(-1)
        assert torch.equal(cand['seeds'], seeds) and cand['ids'].shape == (9, 12)
        assert cand['n_valid'].tolist() == [len(snap) - 1] * 9 and bool((cand['ids'] != 0).all())   # every row but the seed's
        want_c = m.similar_items(seeds, snap, 12, metric=metric)    # every seed is a destination node: in the snapshot
        assert torch.equal(cand['ids'], want_c[0]) and not bool((cand['ids'] == seeds[:, None]).any())
        assert same((ids, scores, n_valid), m.recommend_subset(src, ts, snap, 5, cand['ids']))
        assert n_valid.tolist() == [12] * 9 and bool(torch.isfinite(scores).all())    # n_valid counts the columns left in
    # explicit seeds on the items-only snapshot: 0 and an id that is not in the snapshot (a user) have no candidates
    small = b['snap_items']
    seeds = torch.cat([small.ids[:7], t([0, int(src[0])])])
    ids, scores, n_valid, cand = m.recommend_similar(src, ts, small, 5, S=64, seeds=seeds)
    assert n_valid[7:].tolist() == [0, 0] and cand['n_valid'][7:].tolist() == [0, 0]
    assert torch.equal(n_valid[:7], cand['n_valid'][:7])    # every candidate is a row of the snapshot
    assert bool((cand['ids'][7:] == 0).all()) and bool((ids[7:] == 0).all()) and bool(torch.isneginf(scores[7:]).all())
    assert int(cand['n_valid'][:7].max()) == len(small) - 1 < 64          # every other item, then padding
    assert same((ids, scores, n_valid), m.recommend_subset(src, ts, small, 5, cand['ids']))
    # sources whose first event comes after the query time have no entry before it: the default seed is 0
    nodes = np.r_[st['src'], st['dst']]
    first_t = {int(n): float(np.r_[st['ts'], st['ts']][nodes == n].min()) for n in np.unique(nodes)}
    fresh = [n for n, ft in first_t.items() if ft > b['when']][:4]
    assert len(fresh) > 0
    mixed = torch.cat([t(fresh), src[:2]])
    ids, _, n_valid, cand = m.recommend_similar(mixed, ts[:len(mixed)], snap, 5, S=8)
    nf = len(fresh)
    assert bool((cand['seeds'][:nf] == 0).all()) and n_valid[:nf].tolist() == [0] * nf and bool((ids[:nf] == 0).all())
    assert n_valid[nf:].tolist() == [8, 8]
    with pytest.raises(ValueError, match=str(_lib.TG_TOPK_MAX_K)):
        m.recommend_similar(src, ts, snap, 5, S=65)
    with pytest.raises(ValueError, match='seeds'):
        m.recommend_similar(src, ts, snap, 5, seeds=seeds[:3])
    assert_same_state(b['before'], state_of(m))


def test_eval_recommendation_similar_on_a_two_batch_loader(monkeypatch):
    """100 events at batch 50: finite metrics, and coverage equal to a numpy recount from the candidates the generator
    returned and the true destinations; walk together with similar raises"""
    from www2023tiger_amd.eval_utils import eval_recommendation
    E, S, k = 100, 16, 5
    A, _, st = build(D, D, K, 'bin', seed=3, E=E)
    cat = np.unique(st['dst']).astype(np.int64)
    seen = []
    real = A.recommend_similar

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append(out[3]['ids'].cpu().numpy())
        return out
    monkeypatch.setattr(A, 'recommend_similar', spy)
    out = eval_recommendation(A, loader(A, st, K), dev(), similar=dict(S=S, catalogue=cat, metric='cos'), k=k,
                              return_positions=True)
    assert out['n_events'] == E and len(seen) == 2
    for key in ('hit_rate', 'ndcg', 'mrr_at_k', 'coverage', 'seeded', 'candidates'):
        assert np.isfinite(out[key]), key
    cand = np.concatenate(seen)
    dst = np.asarray(st['dst'][:E])
    covered = ((cand == dst[:, None]) & (cand != 0)).any(1)
    assert abs(out['coverage'] - covered.mean()) < 1e-12 and 0.0 <= out['hit_rate'] <= out['coverage'] <= 1.0
    assert abs(out['candidates'] - (cand != 0).sum() / E) < 1e-12 and 0.0 < out['seeded'] <= 1.0
    pos = out['positions'].cpu().numpy()
    assert ((pos >= 0) <= covered).all()
    print(f"similar: recall@{S} {out['coverage']:.4f}, seeded {out['seeded']:.4f}, hit_rate {out['hit_rate']:.4f}")
    with pytest.raises(ValueError, match='walk and similar'):
        eval_recommendation(A, None, dev(), walk=dict(C=8), similar=dict(S=S, catalogue=cat))
    with pytest.raises(ValueError, match='similar'):
        eval_recommendation(A, None, dev(), cat, similar=dict(S=S, catalogue=cat))
    with pytest.raises(ValueError, match='64'):
        eval_recommendation(A, None, dev(), similar=dict(S=65, catalogue=cat))
