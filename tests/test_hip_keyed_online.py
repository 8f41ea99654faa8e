"""TIGE.observe_keys / recommend_keys on the GPU: serving behind external keys changes nothing but the names.  The stream of
tests/test_hip_grow_nodes.py numbers its ids in the order of their first appearance - the id map's own rule - so a keyed run
gets the stream's dense ids.  Model B observes the tail with observe(num_node='auto'); model C, with equal weights, sits
behind IdMap.from_keys(scramble(1 .. N0 - 1)) and observes the same batches with observe_keys on scrambled keys.  After every
batch embeddings, both memories, the mailbox, the four graph arrays and n_nodes are compared with torch.equal; recommend_keys
on C must be scramble(recommend on B)."""
import io

import numpy as np
import pytest
import torch

from test_hip_grow_nodes import BATCHES, E0, assert_same_state, batch, build, ids_upto, state_of, twins
from test_hip_rank import dev
from www2023tiger_amd.data.idmap import IdMap

pytestmark = pytest.mark.gpu

INT64_MIN = -(1 << 63)
MULT = np.uint64(0x9E3779B97F4A7C15)   # odd: a bijection of the 64-bit integers


def scramble(ids):
    """dense id -> key (int64, wrapping product); the padding id 0 -> INT64_MIN, as IdMap.keys_of gives it"""
    a = ids.cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    a = a.astype(np.int64)
    k = (a.astype(np.uint64) * MULT).astype(np.int64)
    return torch.from_numpy(np.where(a == 0, INT64_MIN, k))


def keyed_twins(**kw):
    """B: the dense model of test_hip_grow_nodes.twins; C: equal weights, the same E0 events streamed, behind a map seeded
    with the keys of the ids both were built on"""
    _, B, st, nf = twins(**kw)
    C = build(st, nf, B.n_nodes, E0, **kw)
    C.stream_step(*batch(st, 0, E0))
    assert_same_state(B, C)
    idmap = IdMap.from_keys(scramble(np.arange(1, B.n_nodes)), dev())
    assert idmap.size == B.n_nodes
    return B, C, idmap, st, nf


def same_models(B, C, what=''):
    assert B.n_nodes == C.n_nodes == C.graph.num_node, what
    for k, v in state_of(B).items():
        assert torch.equal(v, state_of(C)[k]), f'{what}: {k}'
    for a, b in zip(B.graph._tensors(), C.graph._tensors()):
        assert a.dtype == b.dtype and torch.equal(a, b), f'{what}: graph arrays'
    assert torch.equal(B.raw_feat_getter.nfeats, C.raw_feat_getter.nfeats), what


def feed(B, C, idmap, st, nf, lo, hi, observe_b=True):
    """one batch through both (B by dense ids unless it is a keyed model too: observe_b = its map) -> C's step"""
    src, dst, _, ts, eids = batch(st, lo, hi)
    n_old, n_new = C.n_nodes, max(C.n_nodes, ids_upto(st, hi))
    rows = nf[n_old:n_new]
    if observe_b is True:
        b = B.observe(src, dst, ts, eids, num_node='auto', nfeats=rows)
    else:
        b = B.observe_keys(observe_b, scramble(src), scramble(dst), ts, eids, nfeats=rows)
    c = C.observe_keys(idmap, scramble(src), scramble(dst), ts, eids, nfeats=rows)
    assert torch.equal(c.h[:3 * (hi - lo)], b.h[:3 * (hi - lo)]), f'h of batch [{lo}, {hi})'
    assert idmap.size == C.n_nodes == n_new
    same_models(B, C, f'batch [{lo}, {hi})')
    return c


def queries(st, hi, n=6):
    q = torch.from_numpy(st['src'][hi - n:hi].copy()).to(dev())
    t = torch.full((n,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    cand = torch.tensor(sorted(set(st['dst'][:hi].tolist())), device=dev())
    return q, t, cand


def same_lists(got, want, what=''):
    """recommend_keys on C against recommend on B: keys = scramble(ids), scores bit for bit, the same counts"""
    keys, scores, n_valid = got
    ids, s, nv = want
    assert keys.dtype == torch.int64 and torch.equal(keys.cpu(), scramble(ids)), what
    assert torch.equal(scores.view(torch.int32), s.view(torch.int32)) and torch.equal(n_valid, nv), what
    pad = torch.arange(ids.shape[1], device=ids.device)[None, :] >= nv[:, None].long()
    assert bool((keys[pad] == INT64_MIN).all()), what


def test_observe_keys_equals_observe_on_the_streams_own_ids():
    B, C, idmap, st, nf = keyed_twins()
    admitted = []
    for lo, hi in BATCHES:
        n0 = idmap.size
        feed(B, C, idmap, st, nf, lo, hi)
        admitted.append(idmap.size - n0)
    assert admitted[1] == admitted[2] == 0 and min(admitted[0], admitted[3], admitted[4]) > 0
    assert idmap.size == st['n_stream']
    every = np.arange(1, st['n_stream'])
    assert torch.equal(idmap.lookup(scramble(every).to(dev())).cpu(), torch.from_numpy(every.astype(np.int32)))


def test_nfeats_may_be_a_function_of_the_admitted_keys():
    B, C, idmap, st, nf = keyed_twins()
    lo, hi = BATCHES[0]
    src, dst, _, ts, eids = batch(st, lo, hi)
    n_old, n_new = C.n_nodes, ids_upto(st, hi)
    seen = []

    def rows(keys):
        seen.append(keys.clone())
        return nf[n_old:n_new]

    b = B.observe(src, dst, ts, eids, num_node='auto', nfeats=nf[n_old:n_new])
    c = C.observe_keys(idmap, scramble(src), scramble(dst), ts, eids, nfeats=rows)
    assert len(seen) == 1 and torch.equal(seen[0].cpu(), scramble(np.arange(n_old, n_new)))
    assert torch.equal(c.h[:3 * (hi - lo)], b.h[:3 * (hi - lo)])
    same_models(B, C)


def test_recommend_keys_equals_scrambled_recommend():
    B, C, idmap, st, nf = keyed_twins()
    for lo, hi in BATCHES[:4]:
        feed(B, C, idmap, st, nf, lo, hi)
    hi = BATCHES[3][1]
    q, t, cand = queries(st, hi)
    qk, k = scramble(q).to(dev()), len(cand)
    want = B.recommend(q, t, cand, k, exclude_seen=True)
    assert int(want[2].min()) < k                                    # someone has seen an item: padded columns exist
    same_lists(C.recommend_keys(idmap, qk, t, cand, k, exclude_seen=True), want, 'dense cand')
    same_lists(C.recommend_keys(idmap, qk, t, None, k, cand_keys=scramble(cand).to(dev()), exclude_seen=True), want, 'cand_keys')
    # a candidate key nobody has seen becomes the padding id: the list of the catalogue with a 0 in its place
    unknown = torch.cat([scramble(cand[:3]), torch.tensor([12345, 777]), scramble(cand[3:])]).to(dev())
    with_pad = torch.cat([cand[:3], torch.zeros(2, dtype=cand.dtype, device=dev()), cand[3:]])
    same_lists(C.recommend_keys(idmap, qk, t, None, k, cand_keys=unknown), B.recommend(q, t, with_pad, k), 'unknown candidates')
    per_query = cand[torch.arange(len(q) * 4, device=dev()).reshape(len(q), 4) % len(cand)]
    same_lists(C.recommend_keys(idmap, qk, t, None, 3, cand_keys=scramble(per_query).reshape(len(q), 4).to(dev())),
               B.recommend(q, t, per_query, 3), 'per-query cand_keys')
    t_snap = float(st['ts'][hi - 1]) + 0.5
    snap_b, snap_c = B.embed_catalogue(cand, t_snap), C.embed_catalogue(cand, t_snap)
    same_lists(C.recommend_keys(idmap, qk, t, snap_c, k, exclude_seen=True), B.recommend(q, t, snap_b, k, exclude_seen=True),
               'snapshot')
    with pytest.raises(ValueError, match='one of them'):
        C.recommend_keys(idmap, qk, t, cand, k, cand_keys=scramble(cand).to(dev()))
    with pytest.raises(ValueError, match='int64'):
        C.recommend_keys(idmap, qk.int(), t, cand, k)


def test_an_unknown_source_is_refused_or_admitted():
    B, C, idmap, st, nf = keyed_twins()
    for lo, hi in BATCHES:
        feed(B, C, idmap, st, nf, lo, hi)
    q, t, cand = queries(st, BATCHES[-1][1], n=2)
    newcomer = 424242
    qk = torch.tensor([int(scramble(q[:1])[0]), newcomer], device=dev())
    tables = [x.clone() for x in idmap.tables]
    n0, g0, size0 = C.n_nodes, C.graph, idmap.size
    s0 = {k: v.clone() for k, v in state_of(C).items()}
    with pytest.raises(ValueError, match='1 of the 2 sources'):
        C.recommend_keys(idmap, qk, t, cand, 5)
    assert idmap.size == size0 and all(torch.equal(a, b) for a, b in zip(idmap.tables, tables))
    assert C.n_nodes == n0 and C.graph is g0 and all(torch.equal(v, s0[k]) for k, v in state_of(C).items())
    keys, scores, n_valid = C.recommend_keys(idmap, qk, t, cand, 5, admit=True)
    assert idmap.size == size0 + 1 == C.n_nodes == C.graph.num_node
    assert int(idmap.lookup(qk)[1]) == size0                          # the next id
    assert n_valid.tolist() == [len(cand)] * 2 and len(cand) >= 5     # (n_valid counts the candidates left in, not k)
    assert keys.shape == (2, 5) and bool(torch.isfinite(scores).all())   # a full list for the newcomer, finite scores
    assert bool(torch.isin(keys.cpu(), scramble(cand)).all())
    same_lists((keys[:1], scores[:1], n_valid[:1]), B.recommend(q[:1], t[:1], cand, 5), 'the known source, after the growth')
    # the model still follows its twin once that one has admitted the id too
    B.grow_nodes(B.n_nodes + 1)
    same_models(B, C, 'after the admission')


def test_what_can_be_told_without_the_ids_is_refused_before_a_key_is_assigned(monkeypatch):
    from www2023tiger_amd.model.restarters import StaticRestarter
    B, C, idmap, st, nf = keyed_twins()
    lo, hi = BATCHES[0]
    src, dst, _, ts, eids = batch(st, lo, hi)
    rows = nf[C.n_nodes:ids_upto(st, hi)]
    tables = [x.clone() for x in idmap.tables]
    size0, n0 = idmap.size, C.n_nodes

    def refused(exc, match):
        with pytest.raises(exc, match=match):
            C.observe_keys(idmap, scramble(src), scramble(dst), ts, eids, nfeats=rows)
        assert idmap.size == size0 and all(torch.equal(a, b) for a, b in zip(idmap.tables, tables)) and C.n_nodes == n0

    C.train()
    refused(RuntimeError, 'eval')
    C.eval()
    C._row_of = torch.zeros(C.n_nodes, dtype=torch.int32, device=dev())
    refused(RuntimeError, 'partitioned')
    C._row_of = None
    seq = C.restarter_fn
    C.restarter_fn = StaticRestarter(raw_feat_getter=C.raw_feat_getter, graph=C.graph).to(dev())
    refused(NotImplementedError, 'static restarter')
    C.restarter_fn = seq
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)   # (the check alone, as in test_hip_grow_nodes)
    refused(RuntimeError, 'captured')
    monkeypatch.undo()
    with pytest.raises(ValueError, match='int64'):
        C.observe_keys(idmap, scramble(src).int(), scramble(dst), ts, eids)
    with pytest.raises(TypeError, match='num_node'):
        C.observe_keys(idmap, scramble(src), scramble(dst), ts, eids, num_node=5)
    with pytest.raises(ValueError, match='lives on'):
        C.observe_keys(IdMap('cpu'), scramble(src), scramble(dst), ts, eids)
    assert idmap.size == size0
    # what needs the ids comes after the assignment: the model is untouched, the keys stay assigned ...
    g0 = C.graph
    with pytest.raises(ValueError, match='before the latest event'):
        C.observe_keys(idmap, scramble(src), scramble(dst), ts - 1e6, eids, nfeats=rows)
    assert idmap.size == ids_upto(st, hi) > size0 and C.n_nodes == n0 and C.graph is g0
    # ... and the batch that brings their events admits them: the model follows its twin
    feed(B, C, idmap, st, nf, lo, hi)


def test_save_and_load_with_the_map_in_the_same_file():
    B, C, idmap, st, nf = keyed_twins()
    for lo, hi in BATCHES[:3]:
        feed(B, C, idmap, st, nf, lo, hi)
    f = io.BytesIO()
    torch.save({'online': C.online_state(), 'idmap': idmap.state_dict()}, f)
    f.seek(0)
    saved = torch.load(f, weights_only=True)
    D = build(st, nf, ids_upto(st, E0), E0)
    D.load_online(saved['online'])
    map_d = IdMap.from_state_dict(saved['idmap'], dev())
    assert map_d.size == idmap.size == D.n_nodes and torch.equal(map_d.key_of[:map_d.size], idmap.key_of[:idmap.size])
    same_models(C, D, 'loaded')
    for lo, hi in BATCHES[3:]:
        src, dst, _, ts, eids = batch(st, lo, hi)
        B.observe(src, dst, ts, eids, num_node='auto', nfeats=nf[B.n_nodes:max(B.n_nodes, ids_upto(st, hi))])
        feed(C, D, map_d, st, nf, lo, hi, observe_b=idmap)
    same_models(B, D, 'the dense model')
    assert torch.equal(map_d.key_of[:map_d.size], idmap.key_of[:idmap.size])
    q, t, cand = queries(st, BATCHES[-1][1])
    qk = scramble(q).to(dev())
    got, want = D.recommend_keys(map_d, qk, t, cand, 5, exclude_seen=True), C.recommend_keys(idmap, qk, t, cand, 5, exclude_seen=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    same_lists(got, B.recommend(q, t, cand, 5, exclude_seen=True), 'against the dense model')


def test_the_online_example_behind_keys(tmp_path, capsys):
    """examples/recommend.run_online(keyed=True) on the toy JODIE files of test_hip_grow_nodes: without grow the keyed
    lists are the scramble of the lists of the replay by ids, with its metrics; with grow the keys admitted per batch add up to
    the ids the test split brings, and a replay saved after two batches and one that loads the file - map included - write
    the lists of the uninterrupted replay"""
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
    late = np.arange(len(z['src']) - 250, len(z['src']))
    z['dst'][late[::10]] = top + 1 + np.arange(len(late[::10])) % 7
    z['src'][late[5::17]] = top + 8 + np.arange(len(late[5::17])) % 3
    z['labels'] = np.zeros(len(z['src']), dtype=np.int64)
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    plain, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, offline=False, save_after=1000, verbose=False, **kw)
    on, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, offline=False, keyed=True, verbose=False, **kw)
    assert on['ids'].dtype == np.int64 and sum(on['admitted']) == 0
    assert np.array_equal(on['ids'], np.where(plain['ids'] == 0, INT64_MIN, rc.scramble(plain['ids'])))
    assert all(on[k] == plain[k] for k in ('hit_rate', 'ndcg', 'mrr_at_k', 'n_events'))
    capsys.readouterr()
    whole, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, **kw)
    assert sum(whole['admitted']) == 10 and whole['ids'].shape == (whole['n_events'], 5)
    said = capsys.readouterr().out   # what a verbose replay prints: the keys admitted per batch, and nothing about a file
    assert said.count('keys admitted') == len(whole['admitted']) and 'loaded' not in said and 'saved' not in said
    state = str(tmp_path / 'served.pt')
    head, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, verbose=False, save_state=state,
                            save_after=2, **kw)
    tail, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, load_state=state, **kw)
    said = capsys.readouterr().out
    assert f'loaded {state}:' in said and 'continuing at event 200 of the split' in said
    assert np.array_equal(np.concatenate([head['ids'], tail['ids']]), whole['ids'])
    assert head['admitted'] + tail['admitted'] == whole['admitted']
    # the replay by ids says what it said before there were keys: its file is named when it loads one, and only then
    plain_state = str(tmp_path / 'plain.pt')
    rc.run_online('toy', str(tmp_path), ckpt, k=5, grow=True, save_state=plain_state, save_after=2, **kw)
    said = capsys.readouterr().out
    assert 'loaded' not in said and f'saved {plain_state}:' in said
    rc.run_online('toy', str(tmp_path), ckpt, k=5, grow=True, load_state=plain_state, **kw)
    assert f'loaded {plain_state}:' in capsys.readouterr().out
    with pytest.raises(ValueError, match='holds no id map'):
        rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, verbose=False, load_state=plain_state, **kw)
