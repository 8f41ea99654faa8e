"""TIGE.compact_nodes / TIGE.compact_keys on the GPU: small models (d = 8 and 16, sequence restarter, one and
two layers, batches of at most 64 events) against twins that never compact.  The remap is monotone, so every "ascending id"
tie-break survives the renumbering and every product is compared with torch.equal under `remap`.
  1. dense: C erases nodes and compacts, its twin D erases the same nodes and does not;
  2. keyed: the churn of tests/test_hip_erase_keys.py with compact_keys behind every erase, against a model that never
     removes a key - per live KEY;
  3. save_online + the map's state after a compaction, loaded into a freshly built model;
  4. a key that was assigned but never admitted, below and above a dropped id;
  5. every refusal leaves tables, graph and map unchanged;
  6. a snapshot of the old numbering is refused."""
import contextlib
import io

import numpy as np
import pytest
import torch

import test_hip_grow_nodes as G
from test_hip_erase_keys import Stream, born, dt, keyed_observe, lists_by_key
from test_hip_grow_nodes import BATCHES, E0, batch, build, state_of
from test_hip_keyed_online import same_models
from test_hip_rank import dev
from www2023tiger_amd import hip_ops
from www2023tiger_amd.data.idmap import IdMap, _capacity_for

pytestmark = pytest.mark.gpu
ROWS = ('left_vals', 'left_ts', 'left_active', 'right_vals', 'right_ts', 'right_active', 'msg_vals', 'msg_ts')


@contextlib.contextmanager
def width(d):
    """the stream and the model of test_hip_grow_nodes at another width"""
    old, G.D = G.D, d
    try:
        yield
    finally:
        G.D = old


def has_msg(m, ids):
    return (m.msg_store.has_msg_bits[ids >> 6] >> (ids & 63)) & 1


def same_under_remap(C, D, plan, what):
    """every per-node row, bit and graph array of C is D's under the plan"""
    old = plan.old_of[:C.n_nodes].long()
    assert C.n_nodes == plan.n_graph_new == C.graph.num_node == C.raw_feat_getter.n_nodes == C.restarter_fn.n_nodes, what
    sc, sd = state_of(C), state_of(D)
    for name in ROWS:
        assert sc[name].shape[0] == C.n_nodes and torch.equal(sc[name], sd[name][old]), f'{what}: {name}'
    assert torch.equal(has_msg(C, torch.arange(C.n_nodes, device=dev())), has_msg(D, old)), f'{what}: has_msg'
    assert sc['has_msg'].numel() == hip_ops.bitmap_words(C.n_nodes)
    spare = 64 * sc['has_msg'].numel() - C.n_nodes
    last = int(sc['has_msg'][-1]) & ((1 << 64) - 1)
    assert 0 <= spare < 64 and (spare == 0 or last >> (64 - spare) == 0), f'{what}: spare bits'
    assert torch.equal(C.raw_feat_getter.nfeats, D.raw_feat_getter.nfeats[old]), f'{what}: node table'
    c, d = C.graph._tensors(), D.graph._tensors()
    kept_bounds = torch.cat([d[0][old], d[0][-1:]])
    assert torch.equal(c[0], kept_bounds) and torch.equal(c[1], d[1]) and torch.equal(c[3], d[3]), f'{what}: indptr / ts / eid'
    assert torch.equal(c[2], plan.remap[d[2].long()]), f'{what}: nbr'


def same_products(C, D, plan, st, hi, what):
    """recommend, recommend_walk, trending and rank_scores: ids under remap, scores and counts bit for bit"""
    r = lambda ids: plan.remap[ids.long()].long()
    alive = lambda ids: ids[plan.remap[ids.long()] >= 0]
    q = alive(torch.from_numpy(st['src'][hi - 12:hi].copy()).to(dev()))
    t = torch.full((q.numel(),), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    cand = alive(torch.tensor(sorted(set(st['dst'][:hi].tolist())), device=dev()))
    assert q.numel() >= 4 and cand.numel() >= 6
    ic, sc, nc = C.recommend(r(q), t, r(cand), 5)
    id_, sd, nd = D.recommend(q, t, cand, 5)
    assert torch.equal(ic, r(id_)) and torch.equal(sc.view(torch.int32), sd.view(torch.int32)) and torch.equal(nc, nd), what
    wc, wd = C.recommend_walk(r(q), t, 4, C=32), D.recommend_walk(q, t, 4, C=32)
    assert torch.equal(wc[0], r(wd[0])) and torch.equal(wc[1].view(torch.int32), wd[1].view(torch.int32)), f'{what}: walk'
    assert torch.equal(wc[2], wd[2]) and torch.equal(wc[3]['ids'], r(wd[3]['ids'])), f'{what}: walk candidates'
    assert torch.equal(wc[3]['counts'], wd[3]['counts']), f'{what}: walk counts'
    tc, td = hip_ops.trending(C.graph, float(t[0]), 16), hip_ops.trending(D.graph, float(t[0]), 16)
    assert torch.equal(tc['ids'], r(td['ids'])) and all(torch.equal(tc[k], td[k]) for k in ('counts', 'n_valid', 'n_distinct')), \
        f'{what}: trending'
    dst = alive(torch.from_numpy(st['dst'][hi - 12:hi].copy()).to(dev()))[:q.numel()]
    n = min(q.numel(), dst.numel())
    rc = C.rank_scores(r(q[:n]), r(dst[:n]), t[:n], r(cand))
    rd = D.rank_scores(q[:n], dst[:n], t[:n], cand)
    assert torch.equal(rc.view(torch.int32), rd.view(torch.int32)), f'{what}: rank_scores'


def gone_for_good(st, hi, n=6):
    """ids met before `hi` that no later event names (so the twins can go on observing), and the one id nobody ever meets"""
    seen = np.union1d(st['src'][:hi], st['dst'][:hi])
    later = np.union1d(st['src'][hi:], st['dst'][hi:])
    gone = np.setdiff1d(seen, later)
    gone = gone[gone > 0]
    assert len(gone) >= n
    return np.concatenate([gone[:: max(1, len(gone) // n)][:n], [st['n_nodes'] - 1]]).astype(np.int64)


@pytest.mark.parametrize('d,L,forms', [(8, 1, ()), (16, 2, ()), (8, 1, ('fused', 'eager'))])
def test_dense_compaction_equals_the_uncompacted_twin_under_remap(d, L, forms):
    with width(d):
        st, nf = G.make_stream()
        C, D = (build(st, nf, st['n_nodes'], E0, L=L, forms=forms) for _ in range(2))
    for m in (C, D):
        m.stream_step(*batch(st, 0, E0))
        for lo, hi in BATCHES[:4]:
            src, dst, _, ts, eids = batch(st, lo, hi)
            for a in range(lo, hi, 64):
                b = min(hi, a + 64)
                m.observe(src[a - lo:b - lo], dst[a - lo:b - lo], ts[a - lo:b - lo], eids[a - lo:b - lo])
    hi = BATCHES[3][1]
    gone = gone_for_good(st, hi)
    C.erase(nodes=gone)
    D.erase(nodes=gone)
    same_models(C, D, 'erased')
    n_old, table = C.n_nodes, C.left_memory.vals
    plan = C.compact_nodes(gone)
    assert (plan.n_old, plan.n_new) == (n_old, n_old - len(gone)) and C.left_memory.vals is not table
    remap = np.full(n_old, -1, dtype=np.int32)
    remap[np.setdiff1d(np.arange(n_old), gone)] = np.arange(plan.n_new)
    assert torch.equal(plan.remap.cpu(), torch.from_numpy(remap)) and int(plan.remap[0]) == 0
    assert plan.translate(dt(gone)).eq(-1).all()
    same_under_remap(C, D, plan, 'compacted')
    same_products(C, D, plan, st, hi, 'before any further batch')
    # several further batches, C's ids translated; no new id is admitted
    lo, end = BATCHES[4]
    for a in range(lo, end, 20):
        b = min(end, a + 20)
        src, dst, _, ts, eids = batch(st, a, b)
        hc = C.observe(plan.translate(dt(src)), plan.translate(dt(dst)), ts, eids)
        hd = D.observe(src, dst, ts, eids)
        assert torch.equal(hc.h[:3 * (b - a)], hd.h[:3 * (b - a)]), f'h of batch [{a}, {b})'
        same_under_remap(C, D, plan, f'batch [{a}, {b})')
        same_products(C, D, plan, st, b, f'batch [{a}, {b})')
    # the tables still grow: a brand-new id is admitted into the head-room of the new stores
    ptrs = G.pointers(C)
    assert C.grow_nodes(C.n_nodes + 3) is False and G.pointers(C) == ptrs
    with pytest.raises(ValueError, match='rows are never released'):
        C.left_memory.grow(C.n_nodes - 1)
    # a checkpoint interchanges with a model born with n_new rows
    with width(d):
        fresh = build(st, nf, C.n_nodes, E0, L=L)
    fresh.load_state_dict(C.state_dict())


def test_an_empty_drop_is_the_identity_and_a_bitmap_is_a_drop_set():
    st, nf = G.make_stream()
    C = build(st, nf, st['n_nodes'], E0)
    C.stream_step(*batch(st, 0, E0))
    graph, table = C.graph, C.left_memory.vals
    for drop in ([], torch.zeros(0, dtype=torch.int64), np.zeros(0, dtype=np.int64)):
        plan = C.compact_nodes(drop)
        assert plan.identity and plan.n_new == C.n_nodes and C.graph is graph and C.left_memory.vals is table
        assert torch.equal(plan.remap, torch.arange(C.n_nodes, dtype=torch.int32, device=dev()))
    last = C.n_nodes - 1                                 # the id nobody meets: no entries, nothing to erase
    bits = hip_ops.new_bitmap(C.n_nodes, dev())
    hip_ops.bitmap_mark(dt([last]), bits, C.n_nodes)
    plan = C.compact_nodes(bits, bitmap=True)
    assert plan.n_new == last == C.n_nodes and C.graph is not graph and int(plan.remap[last]) == -1


def run_compacting(S, every=1, upto=len(BATCHES)):
    """the churn of test_hip_erase_keys.run_recycling with compact_keys behind every erase_keys"""
    C = born(S)
    idmap = IdMap.from_keys(torch.from_numpy(S.key[1:S.N0].copy()), dev())
    live, peak, plans = set(S.key[1:S.N0].tolist()), S.N0 - 1, []
    for b, (lo, hi) in enumerate(BATCHES[:upto]):
        keyed_observe(S, C, idmap, lo, hi)
        ks, kd, _, _ = S.keys_of_batch(lo, hi)
        live |= set(ks.tolist()) | set(kd.tolist())
        peak = max(peak, len(live))
        if b in S.leave:
            C.erase_keys(idmap, dt(S.leaving(b)))
            live -= set(S.leaving(b).tolist())
            n_free, size, n_nodes = idmap.n_free, idmap.size, C.n_nodes
            plans.append(C.compact_keys(idmap))
            assert n_free > 0 and (idmap.size, idmap.n_free, idmap.slots_used) == (size - n_free, 0, size - n_free)
            assert C.n_nodes == n_nodes - n_free == idmap.size == len(live) + 1
            assert idmap.capacity == _capacity_for(idmap.size) and not bool(idmap.free_bits.any())
    return C, idmap, live, peak, plans


def test_keyed_churn_with_compaction_against_a_model_that_never_compacts(S):
    """Per live KEY: memory rows, mailbox row, feature row and the keys and scores of recommend_keys(cand_keys=).  Left out
    after the first post-compaction admission: the products with an id tie-break (walk, trending) - the two models number
    the keys admitted later differently, so equal counts are ordered differently."""
    C, cmap, live, peak, plans = run_compacting(S)
    N = born(S)
    nmap = IdMap.from_keys(torch.from_numpy(S.key[1:S.N0].copy()), dev())
    for b, (lo, hi) in enumerate(BATCHES):
        keyed_observe(S, N, nmap, lo, hi)
        if b in S.leave:
            ids = nmap.lookup(dt(S.leaving(b)))
            N.erase(nodes=ids[ids > 0].long())
    # The run ends with a round of its own: one more account closes and the map is compacted behind it.  (Between two
    # compactions `assign` keeps room for a whole batch of new keys - the growth rule of DESIGN 7.18, which this feature does
    # not touch -, so the map's capacity is held against the live peak where a compaction has just run.)
    last = dt([sorted(live)[len(live) // 2]])
    C.erase_keys(cmap, last)
    plans.append(C.compact_keys(cmap))
    N.erase(nodes=nmap.lookup(last).long())
    live -= set(last.tolist())
    assert len(plans) == 3 and all(not p.identity for p in plans)
    # at most the live peak + 1; without compaction the high-water mark
    assert C.n_nodes <= peak + 1 and cmap.capacity <= _capacity_for(peak + 1)
    assert nmap.capacity >= _capacity_for(S.st['n_stream']) >= cmap.capacity
    assert C.n_nodes == cmap.size == len(live) + 1 < N.n_nodes == nmap.size == S.st['n_stream']
    keys = dt(sorted(live))
    ci, ni = cmap.lookup(keys).long(), nmap.lookup(keys).long()
    assert bool((ci > 0).all()) and bool((ni > 0).all()) and not torch.equal(ci, ni)
    assert sorted(ci.tolist()) == list(range(1, C.n_nodes)), 'the live keys fill the id space'
    sc, sn = state_of(C), state_of(N)
    for name in ROWS:
        assert torch.equal(sc[name][ci], sn[name][ni]), name
    assert torch.equal(has_msg(C, ci), has_msg(N, ni)), 'has_msg'
    assert torch.equal(C.raw_feat_getter.nfeats[ci], N.raw_feat_getter.nfeats[ni])
    hi = BATCHES[-1][1]
    q, t, cand, got = lists_by_key(S, C, cmap, hi)
    want = N.recommend_keys(nmap, q, t, None, 4, cand_keys=cand)
    assert torch.equal(got[2], want[2]) and int(got[2].min()) >= 4
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), 'scores'
    assert torch.equal(got[0], want[0]), 'keys'


@pytest.fixture(scope='module')
def S():
    return Stream()


def test_save_and_load_after_a_compaction(S):
    C, idmap, _, _, _ = run_compacting(S, upto=4)       # saved right behind the second compaction
    f = io.BytesIO()
    torch.save({'online': C.online_state(), 'idmap': idmap.state_dict()}, f)
    f.seek(0)
    saved = torch.load(f, weights_only=True)
    assert saved['idmap']['format'] == 'tiger-idmap' and saved['idmap']['version'] == 1      # no holes: version 1 again
    assert saved['online']['n_nodes'] == C.n_nodes >= S.N0
    D = build(S.st, S.nf, S.N0, E0)                      # a stub: fewer rows, another graph
    D.load_online(saved['online'])
    dmap = IdMap.from_state_dict(saved['idmap'], dev())
    assert (dmap.size, dmap.n_free, dmap.capacity) == (idmap.size, 0, idmap.capacity)
    same_models(C, D, 'loaded')
    lo, hi = BATCHES[4]
    c, d = keyed_observe(S, C, idmap, lo, hi), keyed_observe(S, D, dmap, lo, hi)
    assert torch.equal(c.h[:3 * (hi - lo)], d.h[:3 * (hi - lo)])
    assert dmap.size == idmap.size and torch.equal(dmap.key_of[:dmap.size], idmap.key_of[:idmap.size])
    same_models(C, D, 'one batch on')
    got, want = lists_by_key(S, D, dmap, hi)[3], lists_by_key(S, C, idmap, hi)[3]
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_a_key_that_was_assigned_but_never_admitted(S):
    """two keys are assigned by a batch the model refuses; a free id between them and one below both leave"""
    C, idmap, _, _, _ = run_compacting(S, upto=1)
    lo, hi = BATCHES[1]
    ks, kd, ts, eids = S.keys_of_batch(lo, hi)
    kd = kd.copy()
    kd[:3] = [777001, 777002, 777003]                    # (event order: their ids ascend)
    n0, size0 = C.n_nodes, idmap.size
    k = int((idmap.lookup(torch.unique(dt(np.concatenate([ks, kd])))) < 0).sum())   # the three, and whoever comes back
    with pytest.raises(ValueError):                      # the batch goes back in time: refused AFTER the assignment
        C.observe_keys(idmap, dt(ks), dt(kd), ts - 1e9, eids)
    assert k >= 3 and C.n_nodes == n0 == size0 and idmap.size == size0 + k
    old = {key: int(idmap.lookup(dt([key]))[0]) for key in (777001, 777002, 777003)}
    assert n0 <= old[777001] < old[777002] < old[777003]
    known = dt(S.key[S.st['src'][60:100]])
    admitted = known[idmap.lookup(known) > 0][:1]        # an admitted key leaves: a free id BELOW the three
    assert 0 < int(idmap.lookup(admitted)[0]) < n0
    C.erase_keys(idmap, torch.cat([admitted, dt([777002])]))   # and the middle one of the three: a free id between them
    assert idmap.n_free == 2
    state = {name: v.clone() for name, v in state_of(C).items()}
    plan = C.compact_keys(idmap)
    assert (plan.n_old, plan.n_new, plan.n_graph_old, plan.n_graph_new) == (size0 + k, size0 + k - 2, n0, n0 - 1)
    assert C.n_nodes == n0 - 1 and idmap.size == size0 + k - 2 > C.n_nodes and idmap.n_free == 0
    new = {key: int(idmap.lookup(dt([key]))[0]) for key in old}
    assert new[777001] == old[777001] - 1 and new[777003] == old[777003] - 2 and new[777002] == -1
    assert int(idmap.lookup(admitted)[0]) == -1 and new[777001] >= C.n_nodes, 'assigned, still not admitted'
    keep = plan.old_of[:C.n_nodes].long()
    for name in ROWS:
        assert torch.equal(state_of(C)[name], state[name][keep]), name
    # the batch arrives again, in time: the two keys are admitted under their new ids, 777002 is a new key
    C.observe_keys(idmap, dt(ks), dt(kd), ts, eids)
    assert C.n_nodes == idmap.size == size0 + k - 1
    assert int(idmap.lookup(dt([777001]))[0]) == new[777001] and int(idmap.lookup(dt([777002]))[0]) == size0 + k - 2


def snapshot_of(C, idmap=None):
    tabs = {k: (v, v.clone()) for k, v in state_of(C).items()}
    tabs['nfeats'] = (C.raw_feat_getter.nfeats, C.raw_feat_getter.nfeats.clone())
    m = None if idmap is None else ([x.clone() for x in idmap.tables] + [idmap.free_bits.clone()], idmap.tables,
                                   (idmap.size, idmap.n_free, idmap.slots_used))
    return tabs, C.graph, (C.n_nodes, C.raw_feat_getter.n_nodes, C.restarter_fn.n_nodes), m


def unchanged(C, idmap, before, what):
    tabs, graph, counts, m = snapshot_of(C, idmap)
    assert graph is before[1] and counts == before[2], what
    for k, (t, _) in tabs.items():
        assert t is before[0][k][0] and torch.equal(t, before[0][k][1]), f'{what}: {k}'
    if m is not None:
        assert all(a is b for a, b in zip(m[1], before[3][1])) and m[2] == before[3][2], what
        assert all(torch.equal(a, b) for a, b in zip(m[0], before[3][0])), what


def test_every_refusal_leaves_tables_graph_and_map_unchanged(S, monkeypatch):
    C, idmap, _, _, _ = run_compacting(S, upto=1)
    known = dt(S.key[S.st['src'][60:100]])
    leaver = known[idmap.lookup(known) > 0][:1]
    node = int(idmap.lookup(leaver)[0])
    assert 0 < node < C.n_nodes
    C.erase_keys(idmap, leaver)
    assert idmap.n_free == 1
    before = snapshot_of(C, idmap)
    calls = (lambda: C.compact_nodes([node]), lambda: C.compact_keys(idmap))
    C.train()
    for call in calls:
        with pytest.raises(RuntimeError, match='eval'):
            call()
    C.eval()
    C._row_of = torch.zeros(C.n_nodes, dtype=torch.int32, device=dev())
    for call in calls:
        with pytest.raises(RuntimeError, match='partitioned'):
            call()
    C._row_of = None
    fg = C.raw_feat_getter
    fg.pin_mem = False
    for call in calls:
        with pytest.raises(NotImplementedError, match='pinned host memory'):
            call()
    fg.pin_mem = True
    nfeats, fg.nfeats = fg.nfeats, None
    for call in calls:
        with pytest.raises(NotImplementedError, match='no node table'):
            call()
    fg.nfeats = nfeats
    C.left_memory.n += 1
    for call in calls:
        with pytest.raises(RuntimeError, match='do not all hold n_nodes'):
            call()
    C.left_memory.n -= 1
    from www2023tiger_amd.model.restarters import StaticRestarter
    seq = C.restarter_fn
    C.restarter_fn = StaticRestarter(raw_feat_getter=C.raw_feat_getter, graph=C.graph).to(dev())
    for call in calls:
        with pytest.raises(NotImplementedError, match='static restarter'):
            call()
    C.restarter_fn = seq
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)   # (the check alone, as in test_hip_grow_nodes)
    for call in calls:
        with pytest.raises(RuntimeError, match='captured'):
            call()
    monkeypatch.undo()
    unchanged(C, idmap, before, 'refusals before the plan')
    # ids: the padding id, an id outside [0, n_nodes), floats; a bitmap of the wrong size
    for drop, pattern in (([0], 'padding id'), ([C.n_nodes], r'\[0, n_nodes\)'), ([-1], r'\[0, n_nodes\)'),
                          (torch.tensor([1.5]), 'integer node ids')):
        with pytest.raises(ValueError, match=pattern):
            C.compact_nodes(drop)
    with pytest.raises(ValueError, match='a bitmap over'):
        C.compact_nodes(torch.zeros(1, dtype=torch.int32, device=dev()), bitmap=True)
    bits = hip_ops.new_bitmap(C.n_nodes, dev())
    bits[0] = 1
    with pytest.raises(ValueError, match='ID0'):
        C.compact_nodes(bits, bitmap=True)
    # the plan's ROW / NBR classes: the id is named, with the advice to erase first
    deg = torch.diff(C.graph._tensors()[0])
    owner = int(torch.nonzero(deg[1:] > 0)[0]) + 1
    with pytest.raises(ValueError, match=f'node {owner} is dropped but still owns entries of the graph: `erase` it first'):
        C.compact_nodes([owner])
    d = C.graph._tensors()
    lone = [t.clone() for t in d]                        # the owner's row emptied by hand: its id is still a neighbour
    row = torch.repeat_interleave(torch.arange(C.n_nodes, device=dev()), deg)
    keep = row != owner
    ind = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev()), torch.cumsum(torch.bincount(row[keep], minlength=C.n_nodes), 0)])
    from www2023tiger_amd.data.graph import Graph
    broken = Graph._from_device_arrays((ind, lone[1][keep], lone[2][keep], lone[3][keep]), C.graph._t_last, True,
                                       strategy=C.graph.strategy, seed=0)
    good = C.graph
    C.graph = broken
    with pytest.raises(ValueError, match=f'node {owner} is dropped but is still the neighbour of entry'):
        C.compact_nodes([owner])
    C.graph = good
    with pytest.raises(ValueError, match='lives on'):
        C.compact_keys(IdMap('cpu'))
    small = IdMap(dev())
    with pytest.raises(ValueError, match='the model has admitted'):
        C.compact_keys(small)
    # a map whose count of free ids is not what its bitmap holds: refused before the model changes
    idmap.n_free = 2
    with pytest.raises(ValueError, match='free ids'):
        C.compact_keys(idmap)
    idmap.n_free = 1
    unchanged(C, idmap, before, 'refusals')
    # a row width the row kernel does not move is refused while the tables are being BUILT: nothing has changed
    odd = torch.zeros(C.n_nodes, 7, device=dev())
    fg.nfeats = odd
    with pytest.raises(ValueError, match='rows of 28 bytes'):
        C.compact_keys(idmap)
    fg.nfeats = nfeats
    unchanged(C, idmap, before, 'a failure while building')
    plan = C.compact_keys(idmap)                         # and now it goes through
    assert plan.n_new == plan.n_old - 1 and C.n_nodes == before[2][0] - 1 and idmap.n_free == 0


def test_a_snapshot_of_the_old_numbering_is_refused():
    st, nf = G.make_stream()
    C = build(st, nf, st['n_nodes'], E0)
    C.stream_step(*batch(st, 0, E0))
    hi = E0
    cand = torch.tensor(sorted(set(st['dst'][:hi].tolist())), device=dev())
    q = torch.from_numpy(st['src'][hi - 4:hi].copy()).to(dev())
    t = torch.full((4,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    snap = C.embed_catalogue(cand, float(t[0]))
    C.recommend(q, t, snap, 3)
    bits = hip_ops.new_bitmap(C.n_nodes, dev())
    hip_ops.bitmap_mark(q, bits, C.n_nodes)
    never = np.setdiff1d(np.arange(1, st['n_nodes']), np.union1d(st['src'][:hi], st['dst'][:hi]))[:5]
    plan = C.compact_nodes(never)
    for stale_ok in (False, True):                       # refused through the stamp and the count, never remapped
        with pytest.raises((RuntimeError, ValueError), match='catalogue snapshot'):
            C.recommend(plan.translate(q), t, snap, 3, stale_ok=stale_ok)
    fresh = C.embed_catalogue(plan.translate(cand), float(t[0]))
    C.recommend(plan.translate(q), t, fresh, 3)
    # a held uptodate bitmap goes through plan.bitmap
    new_bits = plan.bitmap(bits)
    assert new_bits.numel() == hip_ops.bitmap_words(C.n_nodes)
    marked = torch.nonzero(((new_bits[:, None] >> torch.arange(64, device=dev())) & 1).reshape(-1)).reshape(-1)
    assert torch.equal(marked, torch.unique(plan.translate(q)))


def test_the_online_example_with_compact_at(tmp_path, capsys):
    """examples/recommend.run_online(keyed=True, grow=True, churn=FILE, compact_at=F) on the toy files of
    test_hip_erase_keys: behind the erase of batch 0 the free ids leave the id space, rows before -> after are printed, the
    replay goes on behind the renumbered map and ends smaller than the replay that only recycles; without the flag the
    example does what it did"""
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
    z['labels'] = np.zeros(len(z['src']), dtype=np.int64)
    write_files(str(tmp_path), 'toy', z, with_feats=False)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    cut = int(len(z['src']) * 0.8)
    users = np.setdiff1d(z['src'][:cut], np.concatenate([z['src'][cut:], z['dst']]))[:6]   # they never come back
    assert len(users) == 6
    churn = tmp_path / 'churn.txt'
    churn.write_text('# batch key\n' + ''.join(f'0 {int(rc.scramble(np.array([u]))[0])}\n' for u in users))
    plain, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, churn=str(churn), verbose=False, **kw)
    assert 'compacted' not in plain
    capsys.readouterr()
    out, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, churn=str(churn), compact_at=0.0, **kw)
    said = capsys.readouterr().out
    assert len(out['compacted']) == 1 and said.count('compacted:') == 1 and ' rows -> ' in said
    b, before, after = out['compacted'][0]
    assert b == 0 and after == before - 6 and out['released'] == plain['released']
    assert sum(out['recycled']) == 0 < sum(plain['recycled'])          # nothing is left to recycle: the ids are gone
    assert out['n_nodes'] <= plain['n_nodes'] and out['ids'].shape == plain['ids'].shape
    assert np.array_equal(out['ids'][:100], plain['ids'][:100])         # the lists in front of the compaction
    none, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, churn=str(churn), compact_at=0.9,
                            verbose=False, **kw)
    assert none['compacted'] == [] and np.array_equal(none['ids'], plain['ids'])
    with pytest.raises(ValueError, match='--churn'):
        rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, compact_at=0.5, verbose=False, **kw)
