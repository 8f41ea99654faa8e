"""Retrieve, then rank on a catalogue snapshot, on the GPU: TIGE.recommend_subset(..., snap, ids) (tg_rank_scores_gathered),
TIGE.recommend_walk(..., snapshot=snap) and eval_recommendation(walk=dict(C=..., catalogue=cat)), on the small model of
tests/test_hip_rank.py (d = 16, K = 6, 200 events; 150 for the evaluation loops).  When every query stands at the
snapshot's time the lists are those of the per-query tensor form, which embeds every (candidate, time) pair: every
comparison is exact - ids, score bits, n_valid, state, bitmap."""
import numpy as np
import pytest
import torch

from test_hip_rank import WARM, assert_same_state, batch, build, dev, loader, state_of, warm

pytestmark = pytest.mark.gpu
D, K = 16, 6
WALK = dict(fanout=(10, 10, 10), take=(True, False, True))


def t(x, dt=torch.int64):
    return torch.as_tensor(x).to(dev(), dt)


def warmed(hit='bin', seed=D + K, **kw):
    model, orc, st = build(D, D, K, hit, seed=seed, **kw)
    warm(model, orc, st, K, with_oracle=False)
    return model, st


def at_one_time(st, B, ahead=20):
    """B sources behind the warm-up, all asking at ONE time (that of an event `ahead` events later), and that time"""
    lo = WARM[-1]
    src = batch(st, lo, lo + B)[0]
    when = float(st['ts'][lo + B + ahead])
    return t(src), torch.full((B,), when, dtype=torch.float64, device=dev()), when


def every_other_item(st):
    """the catalogue of the tests below: every second destination node - the stream is bipartite and the default walk
    ends in destination nodes, so about half of the walked-to nodes are in this catalogue and half are not"""
    return np.unique(st['dst'])[::2].astype(np.int64)


def walk_ids(model, src, ts, Cn=12):
    from www2023tiger_amd import hip_ops
    ids = hip_ops.walk_candidates(model.graph, src, ts, Cn, **WALK)['ids']
    assert int((ids != 0).sum(1).max()) > 5 and int((ids == 0).sum()) > 0   # rows longer than k, and padding
    return ids


def same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2]))


def snapshot_tensors(snap):
    return {k: v.clone() for k, v in dict(ids=snap.ids, h=snap.h, nb=snap.nb, P=snap._P, col_of=snap._col_of).items()
            if v is not None}


# ------------------------------------------------------------------------------------------ subset == the per-query form
MODELS = [dict(hit='none'), dict(hit='bin'), dict(hit='count'), dict(hit='vec'), dict(hit='bin', L=2),
          dict(hit='count', strategy='recent_nodes')]


@pytest.mark.parametrize('kw', MODELS, ids=['none', 'bin', 'count', 'vec', 'bin-L2', 'count-recent_nodes'])
def test_a_subset_at_the_snapshot_time_gives_the_lists_of_the_per_query_form(kw):
    """every ts[i] == t, every id of the subset in the catalogue (all node ids): recommend_subset(src, ts, snap, k, ids) ==
    recommend(src, ts, ids, k), and the catalogue broadcast as a subset == recommend(src, ts, snap, k).  Nothing is written.
    (Fails without the feature: there is no recommend_subset.)"""
    model, st = warmed(**kw)
    src, ts, when = at_one_time(st, 9)
    cat = t(np.arange(st['n_nodes'], dtype=np.int64))
    k = 5
    before = state_of(model)
    snap = model.embed_catalogue(cat, when)
    ids = walk_ids(model, src, ts)
    want = model.recommend(src, ts, ids, k)
    assert int(want[2].max()) > k and torch.isfinite(want[1][:, 0]).any() and want[1].unique().numel() > 9
    got = model.recommend_subset(src, ts, snap, k, ids)
    assert same(got, want)
    assert same(model.recommend_subset(src, ts, cat, k, ids, catalogue_at=when), want)
    frozen = snapshot_tensors(snap)
    # the whole catalogue as everybody's subset: the shared form
    whole = cat.unsqueeze(0).expand(9, -1)
    assert same(model.recommend_subset(src, ts, snap, 10, whole), model.recommend(src, ts, snap, 10))
    # k above what a row holds
    assert same(model.recommend_subset(src, ts, snap, 64, ids), model.recommend(src, ts, ids, 64))
    assert_same_state(before, state_of(model))
    after = snapshot_tensors(snap)
    assert frozen.keys() == after.keys() and all(torch.equal(frozen[n], after[n]) for n in frozen)


_BIN = {}


def bin_model():
    """one warmed 'bin' model for the read-only tests below (each asserts that it left the state as it was)"""
    if not _BIN:
        model, st = warmed('bin')
        src, ts, when = at_one_time(st, 9)
        _BIN.update(model=model, st=st, src=src, ts=ts, when=when, ids=walk_ids(model, src, ts),
                    items=t(every_other_item(st)), before=state_of(model))
    return _BIN


def test_ids_outside_the_catalogue_and_the_padding_id_are_left_out():
    """catalogue = every second destination node: a walk also ends in the others.  The lists equal the per-query form's on
    the ids with those entries replaced by the padding id 0"""
    b = bin_model()
    model, src, ts, ids, items = b['model'], b['src'], b['ts'], b['ids'], b['items']
    snap = model.embed_catalogue(items, b['when'])
    inside = torch.isin(ids, items)
    assert 0 < int(inside.sum()) < int((ids != 0).sum())           # some walked-to nodes are items, some are not
    want = model.recommend(src, ts, torch.where(inside, ids, 0), 5)
    got = model.recommend_subset(src, ts, snap, 5, ids)
    assert same(got, want) and int(got[2].sum()) == int(inside.sum())
    col = snap.col_of[ids]
    assert torch.equal(col >= 0, inside) and torch.equal(snap.ids[col.clamp(min=0).long()][inside], ids[inside])
    # an id 0 planted inside a row, and a subset that names an item twice
    twice = ids.clone()
    twice[:, 1] = twice[:, 0]
    twice[:, 2] = 0
    kept = torch.where(torch.isin(twice, items), twice, 0)
    assert same(model.recommend_subset(src, ts, snap, 5, twice), model.recommend(src, ts, kept, 5))
    # nothing of the subset in the catalogue; an empty subset; an empty catalogue
    for sub in (torch.where(inside, 0, ids), ids[:, :0]):
        i, s, n = model.recommend_subset(src, ts, snap, 3, sub)
        assert (i == 0).all() and torch.isneginf(s).all() and (n == 0).all()
    i, s, n = model.recommend_subset(src, ts, model.embed_catalogue(items[:0], b['when']), 3, ids)
    assert (i == 0).all() and torch.isneginf(s).all() and (n == 0).all()
    assert_same_state(b['before'], state_of(model))


def test_a_mask_is_honoured_and_the_chunking_does_not_show():
    b = bin_model()
    model, src, ts, ids, items = b['model'], b['src'], b['ts'], b['ids'], b['items']
    snap = model.embed_catalogue(items, b['when'])
    mask = t(np.random.RandomState(2).rand(*ids.shape) > 0.4, torch.bool)
    inside = torch.isin(ids, items)
    want = model.recommend(src, ts, torch.where(inside & mask, ids, 0), 5)
    got = model.recommend_subset(src, ts, snap, 5, ids, mask=mask)
    assert same(got, want) and int(got[2].sum()) == int((inside & mask).sum()) > 0
    assert not same(got, model.recommend_subset(src, ts, snap, 5, ids))
    Cq = ids.shape[1]
    for chunk_queries in (3 * (Cq + 1), Cq + 1, 1):   # three chunks of three queries; one query per chunk (twice)
        assert same(model.recommend_subset(src, ts, snap, 5, ids, mask=mask, chunk_queries=chunk_queries), got)
    assert_same_state(b['before'], state_of(model))


def test_recommend_walk_on_a_snapshot_is_the_walk_followed_by_the_subset_form():
    from www2023tiger_amd import hip_ops
    b = bin_model()
    model, src, ts, items = b['model'], b['src'], b['ts'], b['items']
    snap = model.embed_catalogue(items, b['when'])
    ids, scores, n_valid, cand = model.recommend_walk(src, ts, 5, C=12, snapshot=snap, exclude_seen=True, **WALK)
    two = hip_ops.walk_candidates(model.graph, src, ts, 12, exclude_seen=True, **WALK)
    assert all(torch.equal(cand[n], two[n]) for n in two)
    assert same((ids, scores, n_valid), model.recommend_subset(src, ts, snap, 5, two['ids']))
    assert same((ids, scores, n_valid), model.recommend(src, ts, torch.where(torch.isin(two['ids'], items), two['ids'], 0), 5))
    c_np, it = two['ids'].cpu().numpy(), set(items.cpu().numpy().tolist())
    count = np.array([sum(1 for x in row if x != 0 and x in it) for row in c_np], dtype=np.int32)
    assert cand['n_in_catalogue'].dtype == torch.int32
    np.testing.assert_array_equal(cand['n_in_catalogue'].cpu().numpy(), count)
    np.testing.assert_array_equal(n_valid.cpu().numpy(), count)
    assert 0 < count.sum() < int(two['n_valid'].sum())
    # without a snapshot the dict is what it was
    assert 'n_in_catalogue' not in model.recommend_walk(src, ts, 5, C=12, **WALK)[3]
    assert_same_state(b['before'], state_of(model))


def test_the_lazy_one_shot_form_equals_restart_embed_and_rank():
    """twin models at reset, empty bitmaps: recommend_subset(..., cat, ids, catalogue_at=t, uptodate=bm) against
    restart_involved over [src | cat], embed_catalogue and the subset form"""
    from www2023tiger_amd import hip_ops
    built = [build(D, D, K, 'bin', seed=D + K) for _ in range(2)]
    (A, B), st = [x[0] for x in built], built[0][2]
    src, ts, when = at_one_time(st, 9)
    items = t(every_other_item(st))
    ids = walk_ids(A, src, ts)
    bm_a, bm_b = (hip_ops.new_bitmap(st['n_nodes'], dev()) for _ in range(2))
    one = A.recommend_subset(src, ts, items, 5, ids, catalogue_at=when, uptodate=bm_a)
    at_t = torch.full((len(items),), when, dtype=torch.float64, device=dev())
    n = B.restart_involved(torch.cat([src, items]), torch.cat([ts, at_t]), bm_b)
    two = B.recommend_subset(src, ts, B.embed_catalogue(items, when), 5, ids)
    assert same(one, two) and int(one[2].sum()) > 0
    assert A.last_restarted == n > 0 and torch.equal(bm_a, bm_b) and int((bm_a != 0).sum()) > 0
    assert_same_state(state_of(A), state_of(B))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_anything_runs():
    from www2023tiger_amd import hip_ops
    b = bin_model()
    m, st, src, ts, ids, items, when = b['model'], b['st'], b['src'], b['ts'], b['ids'], b['items'], b['when']
    other, _ = warmed('bin')
    snap = m.embed_catalogue(items, when)
    bm = hip_ops.new_bitmap(st['n_nodes'], dev())
    bm0 = bm.clone()
    col_of = hip_ops.catalogue_index(items, st['n_nodes'])
    with pytest.raises(ValueError, match='subset.*snapshot'):
        m.recommend_subset(src, ts, items, 5, ids)
    with pytest.raises(ValueError, match='subset.*snapshot'):
        m.recommend_subset(src, ts, ids, 5, ids, uptodate=bm)
    for bad in (ids[:4], ids[0], ids.unsqueeze(0)):
        with pytest.raises(ValueError, match=r'subset.*\[B, Cq\]'):
            m.recommend_subset(src, ts, snap, 5, bad)
    for bad_id in (-1, st['n_nodes']):
        out = ids.clone()
        out[3, 2] = bad_id
        with pytest.raises(ValueError, match='node id outside'):
            m.recommend_subset(src, ts, snap, 5, out)
        with pytest.raises(ValueError, match='node id outside'):
            m.recommend_subset(src, ts, items, 5, out, catalogue_at=when, uptodate=bm)
    for kw in (dict(exclude_seen=True), dict(col_of=col_of)):   # the seen-item filter is the walk's: no such keywords
        with pytest.raises(TypeError, match='unexpected keyword'):
            m.recommend_subset(src, ts, snap, 5, ids, **kw)
    with pytest.raises(ValueError, match='subset'):
        m.recommend_subset(src, ts, snap, 5, None)
    with pytest.raises(ValueError, match='mask'):
        m.recommend_subset(src, ts, snap, 5, ids, mask=torch.ones(len(items), dtype=torch.bool))
    with pytest.raises(ValueError, match='mask'):
        m.recommend_subset(src, ts, snap, 5, ids, mask=torch.ones(9, len(items), dtype=torch.bool))
    # a catalogue that lists an id twice cannot be named by id: as a snapshot, and in the one-shot form before its restart
    dup = torch.cat([items, items[:1]])
    with pytest.raises(ValueError, match='recommend:.*duplicate'):
        m.recommend_subset(src, ts, m.embed_catalogue(dup, when), 5, ids)
    with pytest.raises(ValueError, match='recommend:.*duplicate'):
        m.recommend_subset(src, ts, dup, 5, ids, catalogue_at=when, uptodate=bm)
    # what recommend on a snapshot refuses already
    early = ts.clone()
    early[3] = when - 1.0
    with pytest.raises(ValueError, match='future'):
        m.recommend_subset(src, early, snap, 5, ids)
    with pytest.raises(ValueError, match='another model'):
        m.recommend_subset(src, ts, other.embed_catalogue(items, when), 5, ids)
    with pytest.raises(ValueError, match='another model'):
        m.recommend_walk(src, ts, 5, C=12, snapshot=other.embed_catalogue(items, when))
    with pytest.raises(ValueError, match='uptodate'):
        m.recommend_subset(src, ts, snap, 5, ids, uptodate=bm)
    with pytest.raises(ValueError, match='uptodate'):
        m.recommend_walk(src, ts, 5, C=12, snapshot=snap, uptodate=bm)
    with pytest.raises(ValueError, match='CatalogueSnapshot'):
        m.recommend_walk(src, ts, 5, C=12, snapshot=items)
    with pytest.raises(ValueError, match='k <='):
        m.recommend_subset(src, ts, snap, 65, ids)
    assert_same_state(b['before'], state_of(m))
    assert torch.equal(bm, bm0)
    vec, _, _ = build(8, 8, 5, 'vec')
    with pytest.raises(NotImplementedError, match='vec'):
        vec.recommend_subset(src, ts, items, 5, ids, catalogue_at=when)
    # a stale snapshot (RuntimeError) through either entry, unless recommend is told stale_ok; on a model of its own
    m2, st2 = warmed('bin')
    snap2 = m2.embed_catalogue(items, when)
    m2.stream_step(*batch(st2, WARM[-1], WARM[-1] + 5))
    late = ts + 1.0e6
    with pytest.raises(RuntimeError, match='stale'):
        m2.recommend_subset(src, late, snap2, 5, ids)
    with pytest.raises(RuntimeError, match='stale'):
        m2.recommend_walk(src, late, 5, C=12, snapshot=snap2)
    assert int(m2.recommend_subset(src, late, snap2, 5, ids, stale_ok=True)[2].sum()) > 0
    m2.train()
    with pytest.raises(RuntimeError, match='eval'):
        m2.recommend_subset(src, late, snap2, 5, ids, stale_ok=True)


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('lazy', [False, True], ids=['plain', 'lazy-restarts'])
def test_eval_recommendation_over_walk_candidates_on_one_snapshot_per_batch(lazy):
    """150 events at batch 50: eval_recommendation(walk=dict(C=..., catalogue=cat)) equals the loop written out from public
    pieces on a twin model - the walk at the events' own times, [ONE restart_involved over cat[src, dst, neg] at the event
    times and the catalogue at the batch's earliest time,] embed_catalogue there, recommend_subset, the batch - in
    positions, metrics, state and up-to-date set"""
    from www2023tiger_amd import hip_ops
    from www2023tiger_amd.eval_utils import eval_recommendation
    k, E, Cn = 5, 150, 8
    (A, _, st), (B, _, _) = (build(D, D, K, 'bin', seed=3, E=E) for _ in range(2))
    cat = every_other_item(st)
    upto = set() if lazy else None
    out = eval_recommendation(A, loader(A, st, K), dev(), walk=dict(WALK, C=Cn, catalogue=cat), k=k, exclude_seen=True,
                              return_positions=True, lazy_restarts=lazy, uptodate_nodes=upto)
    bm = hip_ops.new_bitmap(st['n_nodes'], dev())
    positions, covered, n_gen, n_in = [], [], 0, 0
    with torch.no_grad():
        for src, dst, neg, ts, eids, _, cg in loader(B, st, K):
            src, dst, neg, ts, eids = (x.to(dev()) for x in (src, dst, neg, ts, eids))
            cand = hip_ops.walk_candidates(B.graph, src, cg.ts64, Cn, exclude_seen=True, **WALK)['ids']
            t0 = float(cg.ts64.min())
            if lazy:
                at_t0 = torch.full((len(cat),), t0, dtype=torch.float64, device=dev())
                B.restart_involved(torch.cat([src, dst, neg, t(cat)]), torch.cat([cg.ts64.repeat(3), at_t0]), bm)
            snap = B.embed_catalogue(t(cat), t0)
            ids = B.recommend_subset(src, cg.ts64, snap, k, cand)[0]
            hit = (ids == dst[:, None]) & (ids != 0)
            positions.append(torch.where(hit.any(1), hit.float().argmax(1), -1).cpu().numpy())
            c_np = cand.cpu().numpy()
            covered.append(((c_np == dst.cpu().numpy()[:, None]) & (c_np != 0)).any(1))
            n_gen += int((c_np != 0).sum())
            n_in += int(np.isin(c_np, cat).sum())      # (the padding id 0 is no destination node)
            B.contrast_learning(src, dst, neg, ts, eids, cg)
    pos, covered = np.concatenate(positions), np.concatenate(covered)
    np.testing.assert_array_equal(out['positions'].cpu().numpy(), pos)
    hit = pos >= 0
    assert out['n_events'] == E and hit.any() and abs(out['hit_rate'] - hit.mean()) < 1e-12
    assert abs(out['ndcg'] - np.where(hit, 1.0 / np.log2(np.maximum(pos, 0) + 2.0), 0.0).mean()) < 1e-12
    assert abs(out['mrr_at_k'] - np.where(hit, 1.0 / (np.maximum(pos, 0) + 1.0), 0.0).mean()) < 1e-12
    assert abs(out['coverage'] - covered.mean()) < 1e-12 and (covered | ~hit).all()
    assert 0 < n_in < n_gen and abs(out['in_catalogue'] - n_in / n_gen) < 1e-12
    print(f"lazy={lazy}: recall@{Cn} {out['coverage']:.4f}, in_catalogue {out['in_catalogue']:.4f}, hit_rate {out['hit_rate']:.4f}")
    assert_same_state(state_of(A), state_of(B))
    if lazy:
        comp = hip_ops.unique_compact(bm, st['n_nodes'], st['n_nodes'])
        assert upto == set(comp['ids'][:int(comp['count'].item())].tolist()) and len(upto) > 0


def test_the_top_level_refusals_still_raise_and_a_bad_walk_catalogue_is_refused():
    from www2023tiger_amd.eval_utils import eval_recommendation
    b = bin_model()
    m, st = b['model'], b['st']
    cat = every_other_item(st)
    with pytest.raises(ValueError, match='walk'):
        eval_recommendation(m, None, dev(), cat, walk=dict(C=8))
    with pytest.raises(ValueError, match='walk'):
        eval_recommendation(m, None, dev(), cat, walk=dict(C=8, catalogue=cat))
    with pytest.raises(ValueError, match='walk'):
        eval_recommendation(m, None, dev(), walk=dict(C=8, catalogue=cat), catalogue_at='batch')
    with pytest.raises(ValueError, match='duplicate'):
        eval_recommendation(m, None, dev(), walk=dict(C=8, catalogue=np.r_[cat, cat[:1]]))
    with pytest.raises(ValueError, match=r'\[C\]'):
        eval_recommendation(m, None, dev(), walk=dict(C=8, catalogue=cat[None]))
    with pytest.raises(ValueError, match=r'\[C\]'):
        eval_recommendation(m, None, dev(), walk=dict(C=8, catalogue=cat[:0]))
    assert_same_state(b['before'], state_of(m))


def test_the_example_runs_with_walk_and_snapshot(tmp_path):
    """examples/recommend.run(walk=C, snapshot=True) on toy JODIE files: the lists it writes are those the metrics were
    folded from, and the dict carries in_catalogue"""
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
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, restart_prob=0.5, ckpt_path=ckpt, **kw)
    ids, scores, m = rc.run('toy', str(tmp_path), ckpt, k=5, walk=8, snapshot=True, out_dir=str(tmp_path), **kw)
    assert ids.shape == scores.shape == (m['n_events'], 5) and m['n_events'] > 0
    assert 0.0 < m['in_catalogue'] <= 1.0 and 0.0 <= m['hit_rate'] <= m['coverage'] <= 1.0
    assert np.array_equal(np.load(os.path.join(str(tmp_path), 'ids.npy')), ids)
    listed = ids != 0
    assert listed.any() and np.isfinite(scores[listed]).all() and np.isneginf(scores[~listed]).all()
    plain = rc.run('toy', str(tmp_path), ckpt, k=5, walk=8, out_dir=str(tmp_path), **kw)[2]
    assert 'in_catalogue' not in plain and plain['coverage'] == m['coverage']   # the generator does not depend on the ranking
