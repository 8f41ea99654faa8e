"""TIGE.observe_events / retract_events on the GPU: at-least-once delivery changes nothing.  Twin models with equal weights
(tests/test_hip_grow_nodes.py::build: d = 8, K = 5, one layer, `recent_edges`, a sequence restarter) start from the first
E0 events; C is fed the clean stream through `observe`, D gets every batch with copies inside it, copies of the previous
batch and once more as a whole through `observe_events`.  Everything is compared with torch.equal: embeddings, memories,
mailbox, graph arrays, edge table, `recommend` lists - also under forget(release_edge_rows=True) after every batch, through
a retraction, through a state round trip and behind an IdMap."""
import numpy as np
import pytest
import torch

from test_hip_grow_nodes import D, K, build, ids_upto, state_of
from test_hip_keyed_online import scramble
from test_hip_rank import dev
from www2023tiger_amd.data.events import EventKeys
from www2023tiger_amd.data.idmap import IdMap

pytestmark = pytest.mark.gpu

E0, B, NB = 40, 32, 10
E = E0 + NB * B
BATCHES = [(E0 + i * B, E0 + (i + 1) * B) for i in range(NB)]
M = 64   # forget(keep_last=M): two batches of B events fit into every node's last M entries


def KEY(idx):
    """the external key of event number idx (0-based position in the stream)"""
    return torch.from_numpy((np.asarray(idx, dtype=np.int64) + 1) * 1_000_003 + 17)


_STREAM = {}


def stream(small=False):
    """bench.make_stream, the ids in the order of their first appearance (the id map's own rule) -> (stream, nfeats).
    small: 8 users and 3 items, so that nodes pass M entries and forget(keep_last=M) has something to drop"""
    if small not in _STREAM:
        import bench
        st = bench.make_stream(*((8, 3) if small else (60, 15)), E, 5000.0, seed=0, d_e=D, with_efeats=True)
        both = np.stack([st['src'], st['dst']], 1).reshape(-1)
        _, first = np.unique(both, return_index=True)
        order = both[np.sort(first)]
        new_id = np.zeros(st['n_nodes'], dtype=np.int64)
        new_id[order] = np.arange(1, len(order) + 1)
        st = dict(st, src=new_id[st['src']], dst=new_id[st['dst']], n_nodes=len(order) + 1)
        nf = (np.random.RandomState(1).standard_normal((st['n_nodes'], D)) * 0.3).astype(np.float32)
        nf[0] = 0
        assert st['efeats'].shape[0] == E + 1 and np.array_equal(st['eids'], np.arange(1, E + 1))
        _STREAM[small] = (st, nf)
    return _STREAM[small]


def model(n_nodes=None, small=False):
    """a model on the first E0 events and the first E0 + 1 rows of the edge table, which has streamed them"""
    st, nf = stream(small)
    m = build(st, nf, n_nodes or st['n_nodes'], E0)
    m.raw_feat_getter.efeats = m.raw_feat_getter.efeats[:E0 + 1].clone()
    m.invalidate_struct()
    m.stream_step(*[st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')])
    return m


def tracked(small=False):
    m = model(small=small)
    ev = m.track_events(KEY(np.arange(E0)))
    assert ev is m.events and ev.size == E0 + 1
    return m


def same_models(C, Dm, what=''):
    a, b = state_of(C), state_of(Dm)
    for k in a:
        assert torch.equal(a[k], b[k]), f'{what}: {k}'
    for x, y in zip(C.graph._tensors(), Dm.graph._tensors()):
        assert x.dtype == y.dtype and torch.equal(x, y), f'{what}: graph arrays'
    assert torch.equal(C.raw_feat_getter.efeats, Dm.raw_feat_getter.efeats), f'{what}: edge table'
    assert Dm.events is None or Dm.events.size == Dm.raw_feat_getter.efeats.shape[0], what


def same_lists(C, Dm, hi, what='', small=False):
    st, _ = stream(small)
    q = torch.from_numpy(st['src'][hi - 6:hi].copy()).to(dev())
    t = torch.full((6,), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    cand = torch.tensor(sorted(set(st['dst'][:hi].tolist())), device=dev())
    for x, y in zip(C.recommend(q, t, cand, 5, exclude_seen=True), Dm.recommend(q, t, cand, 5, exclude_seen=True)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), what


def clean(C, lo, hi, small=False):
    st, _ = stream(small)
    rows = C.raw_feat_getter.efeats.shape[0]
    return C.observe(st['src'][lo:hi], st['dst'][lo:hi], st['ts'][lo:hi], np.arange(rows, rows + hi - lo),
                     efeats=st['efeats'][lo + 1:hi + 1])


def delivery(lo, hi, prev):
    """event numbers as a bus delivers them: copies of the previous batch, the batch with copies inside it, more copies"""
    cur = np.arange(lo, hi)
    old = np.arange(*prev)[::3] if prev else np.arange(0)
    return np.concatenate([old, cur[:10], cur[:5], cur[10:], cur[::4], old[:2]])


def deliver(Dm, idx, small=False, **kw):
    st, _ = stream(small)
    return Dm.observe_events(st['src'][idx], st['dst'][idx], st['ts'][idx], KEY(idx), efeats=st['efeats'][idx + 1], **kw)


def redelivered(C, Dm, lo, hi, prev, what, small=False):
    """one batch through both -> the admission; the whole delivery a second time changes nothing"""
    n = hi - lo
    c = clean(C, lo, hi, small)
    idx = delivery(lo, hi, prev)
    rows = Dm.events.size
    step, adm = deliver(Dm, idx, small)
    uniq, pos = np.unique(idx, return_index=True)
    first = np.sort(pos[uniq >= lo])   # the first copies of this batch's events: everything else is a duplicate
    assert adm.n_kept == n and adm.keep.cpu().numpy().tolist() == first.tolist(), what
    assert torch.equal(step.h[:3 * n], c.h[:3 * n]), f'{what}: h'
    assert Dm.events.size == rows + n
    assert torch.equal(adm.eids.cpu(), Dm.events.lookup(KEY(idx).to(dev())).cpu()) and int(adm.eids.min()) >= 1, what
    again, adm2 = deliver(Dm, idx, small)
    assert again is None and adm2.n_kept == 0 and adm2.keep.numel() == 0 and torch.equal(adm2.eids, adm.eids), what
    same_models(C, Dm, what)
    return adm


def test_a_redelivered_stream_leaves_the_model_of_the_clean_stream():
    C, Dm = model(), tracked()
    same_models(C, Dm, 'start')
    prev = None
    for lo, hi in BATCHES:
        redelivered(C, Dm, lo, hi, prev, f'batch [{lo}, {hi})')
        prev = (lo, hi)
    assert Dm.events.size == E + 1
    assert torch.equal(Dm.events.lookup(KEY(np.arange(E)).to(dev())).cpu(), torch.arange(1, E + 1, dtype=torch.int32))
    same_lists(C, Dm, E, 'recommend')


def test_the_same_while_forgetting_and_releasing_rows_after_every_batch():
    C, Dm = model(small=True), tracked(small=True)
    prev, released = None, 0
    for lo, hi in BATCHES:
        redelivered(C, Dm, lo, hi, prev, f'batch [{lo}, {hi})', small=True)
        for m in (C, Dm):
            m.forget(keep_last=M, release_edge_rows=True)
        released += C.last_release.shift
        same_models(C, Dm, f'forget after [{lo}, {hi})')
        # THE PRECONDITION the dedupe horizon asks for, on the clean model: every event of this batch still owns its row
        # (both of its entries are among their endpoints' last M), so the tracker still holds its key when copies of it
        # arrive with the next batch
        named = torch.unique(C.graph._tensors()[3].long() & 0x7FFFFFFF)
        n_rows = C.raw_feat_getter.efeats.shape[0]
        assert bool(torch.isin(torch.arange(n_rows - (hi - lo), n_rows, device=dev()), named).all())
        rows_now = Dm.events.lookup(KEY(np.arange(lo, hi)).to(dev()))
        assert torch.equal(rows_now.cpu(), torch.arange(n_rows - (hi - lo), n_rows, dtype=torch.int32))
        prev = (lo, hi)
    assert released > 0 and Dm.events.size == E + 1 - released
    gone = Dm.events.lookup(KEY(np.arange(E)).to(dev())) < 0
    assert int(gone.sum()) == released   # the keys left with their rows
    same_lists(C, Dm, E, 'recommend', small=True)


def test_a_batch_that_goes_back_in_time_raises_and_changes_nothing():
    Dm = tracked()
    lo, hi = BATCHES[0]
    deliver(Dm, np.arange(lo, hi))
    s0, g0, rows = {k: v.clone() for k, v in state_of(Dm).items()}, Dm.graph, Dm.events.size
    table = Dm.raw_feat_getter.efeats.clone()
    before = [t.clone() for t in Dm.events.tables]
    st, _ = stream()
    idx = np.arange(hi, hi + 8)
    late_keys = KEY(idx)
    with pytest.raises(ValueError):
        Dm.observe_events(st['src'][idx], st['dst'][idx], st['ts'][idx - 70], late_keys, efeats=st['efeats'][idx + 1])
    assert Dm.events.size == rows and Dm.graph is g0 and torch.equal(Dm.raw_feat_getter.efeats, table)
    assert bool((Dm.events.lookup(late_keys.to(dev())) == -1).all())
    for k, v in state_of(Dm).items():
        assert torch.equal(v, s0[k]), k
    for a, b in zip(before, Dm.events.tables):   # (key_of may have gained spare rows; the mapping has not changed)
        assert torch.equal(a[:rows], b[:rows]) if a is before[2] else torch.equal(a, b)
    # late=True admits it: the graph takes the events, nothing is streamed, the keys are held
    g, adm = Dm.observe_events(st['src'][idx], st['dst'][idx], st['ts'][idx - 70], late_keys, efeats=st['efeats'][idx + 1],
                               late=True)
    assert g is Dm.graph and g is not g0 and adm.n_kept == 8 and Dm.events.size == rows + 8
    assert Dm.events.lookup(late_keys.to(dev())).tolist() == list(range(rows, rows + 8))
    for k, v in state_of(Dm).items():
        assert torch.equal(v, s0[k]), k


def test_retract_events_equals_erase_by_row_and_leaves_a_tombstone():
    C, Dm = model(), tracked()
    for lo, hi in BATCHES[:3]:
        clean(C, lo, hi)
        deliver(Dm, np.arange(lo, hi))
    same_models(C, Dm, 'before')
    hi = BATCHES[2][1]
    gone = np.array([E0 + 3, E0 + 40, 7, E0 + 3])   # two observed events, one the model was built with, a duplicate
    keys = torch.cat([KEY(gone), torch.tensor([123456789, -(1 << 63)])])   # ... an unknown key and INT64_MIN: ignored
    rows = Dm.events.lookup(KEY(gone).to(dev())).long()
    assert rows.tolist() == (gone + 1).tolist()
    g, eids = Dm.retract_events(keys)
    assert g is Dm.graph and torch.equal(eids, rows)
    C.erase(eids=rows)
    same_models(C, Dm, 'retracted')
    assert Dm.graph.tcsr.num_entry == 2 * (hi - 3)
    assert torch.equal(Dm.events.lookup(KEY(gone).to(dev())).long(), rows)   # the key stays: a tombstone
    step, adm = deliver(Dm, gone[:2])   # the bus redelivers the retracted events: dropped
    assert step is None and adm.n_kept == 0
    same_models(C, Dm, 'redelivered after the retraction')
    size = Dm.events.size
    g, eids = Dm.retract_events(KEY([E0 + 50, E0 + 51]), release_edge_rows=True)
    C.erase(eids=eids, release_edge_rows=True)
    same_models(C, Dm, 'retracted and released')
    shift = Dm.last_release.shift
    assert shift == 5 and Dm.events.size == size - shift   # the rows of all five retracted events left the table
    assert bool((Dm.events.lookup(KEY([E0 + 50, E0 + 51, E0 + 3, E0 + 40, 7]).to(dev())) == -1).all())
    g0 = Dm.graph
    g, eids = Dm.retract_events(torch.tensor([5, 6]))   # nothing known: nothing changes
    assert g is g0 and eids.numel() == 0
    lo, hi = BATCHES[3]
    clean(C, lo, hi)
    deliver(Dm, delivery(lo, hi, BATCHES[2]))
    same_models(C, Dm, 'the next batch')


def test_a_saved_model_and_its_tracker_continue_bit_for_bit():
    Dm = tracked()
    for i, (lo, hi) in enumerate(BATCHES[:4]):
        deliver(Dm, delivery(lo, hi, BATCHES[i - 1] if i else None))
    Dm.forget(keep_last=M, release_edge_rows=True)
    online, keys = Dm.online_state(), Dm.events.state_dict()
    F = model()
    F.load_online(online)
    ev = F.attach_events(EventKeys.from_state_dict(keys, dev()))
    assert ev is F.events and ev.size == Dm.events.size
    same_models(Dm, F, 'loaded')
    for i in (4, 5):
        lo, hi = BATCHES[i]
        idx = delivery(lo, hi, BATCHES[i - 1])
        (a, adm_a), (b, adm_b) = deliver(Dm, idx), deliver(F, idx)
        assert torch.equal(a.h[:3 * B], b.h[:3 * B]) and torch.equal(adm_a.eids, adm_b.eids) and torch.equal(adm_a.keep, adm_b.keep)
        same_models(Dm, F, f'batch {i}')
    same_lists(Dm, F, BATCHES[5][1], 'recommend')


def test_the_guards_refuse_before_anything_changes():
    import bench
    st, _ = stream()
    Dm = tracked()
    lo, hi = BATCHES[0]
    s0, g0, rows = {k: v.clone() for k, v in state_of(Dm).items()}, Dm.graph, Dm.events.size
    args = (st['src'][lo:hi], st['dst'][lo:hi], st['ts'][lo:hi], np.arange(rows, rows + B))
    with pytest.raises(RuntimeError, match='tracker is attached'):
        Dm.observe(*args, efeats=st['efeats'][lo + 1:hi + 1])
    with pytest.raises(RuntimeError, match='tracker is attached'):
        Dm.observe_late(*args, efeats=st['efeats'][lo + 1:hi + 1])
    idmap = IdMap.from_keys(scramble(np.arange(1, Dm.n_nodes)), dev())
    with pytest.raises(RuntimeError, match='tracker is attached'):
        Dm.observe_keys(idmap, scramble(args[0]), scramble(args[1]), *args[2:], efeats=st['efeats'][lo + 1:hi + 1])
    with pytest.raises(RuntimeError, match='tracker is attached'):
        Dm.load_online({})
    with pytest.raises(TypeError, match='eids follow'):
        Dm.observe_events(*args[:3], KEY(np.arange(lo, hi)), efeats=st['efeats'][lo + 1:hi + 1], eids=args[3])
    with pytest.raises(ValueError, match='efeats'):
        Dm.observe_events(*args[:3], KEY(np.arange(lo, hi)), efeats=st['efeats'][lo + 1:hi])
    ev = Dm.detach_events()
    assert Dm.events is None and ev.size == rows
    with pytest.raises(RuntimeError, match='no event-key tracker'):
        Dm.observe_events(*args[:3], KEY(np.arange(lo, hi)), efeats=st['efeats'][lo + 1:hi + 1])
    with pytest.raises(RuntimeError, match='no event-key tracker'):
        Dm.retract_events(KEY([3]))
    with pytest.raises(ValueError, match='covers 9 rows'):
        Dm.attach_events(EventKeys(dev(), 9))
    with pytest.raises(ValueError, match='lives on cpu'):
        Dm.attach_events(EventKeys('cpu', rows))
    Dm.train()
    with pytest.raises(RuntimeError, match='eval'):
        Dm.attach_events(ev)
    Dm.eval()
    Dm._row_of = torch.zeros(Dm.n_nodes, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError, match='partitioned'):
        Dm.track_events()
    Dm._row_of = None
    assert Dm.events is None and Dm.graph is g0 and Dm.raw_feat_getter.efeats.shape[0] == rows
    for k, v in state_of(Dm).items():
        assert torch.equal(v, s0[k]), k
    assert Dm.attach_events(ev) is ev
    bare = bench.make_stream(60, 15, 200, 5000.0, seed=0, with_efeats=False)   # a model without an edge table
    N, _ = bench.build_models(bare, 8, 5, 'left', 'right')
    assert N.raw_feat_getter.efeats is None
    with pytest.raises(NotImplementedError, match='no edge table'):
        N.track_events()
    with pytest.raises(NotImplementedError, match='no edge table'):
        N.attach_events(ev)
    assert N.events is None


def test_behind_an_id_map_a_dropped_duplicate_assigns_no_node_id():
    st, nf = stream()
    N0 = ids_upto(st, E0)
    assert N0 < st['n_nodes']
    C, Dm = model(N0), model(N0)
    Dm.track_events(KEY(np.arange(E0)))
    map_c, map_d = (IdMap.from_keys(scramble(np.arange(1, N0)), dev()) for _ in range(2))
    admitted, prev = 0, None
    for lo, hi in BATCHES[:5]:
        rows = C.raw_feat_getter.efeats.shape[0]
        n_before = map_c.size
        c = C.observe_keys(map_c, scramble(st['src'][lo:hi]), scramble(st['dst'][lo:hi]), st['ts'][lo:hi],
                           np.arange(rows, rows + hi - lo), efeats=st['efeats'][lo + 1:hi + 1], nfeats=nf[n_before:ids_upto(st, hi)])
        idx = delivery(lo, hi, prev)
        # a copy of a PREVIOUS event under node keys nobody has seen: were it not dropped first, it would assign two ids
        src_k, dst_k = scramble(st['src'][idx]), scramble(st['dst'][idx])
        if prev:
            src_k[0], dst_k[0] = 999_000 + lo, 999_500 + lo
        d, adm = Dm.observe_events(src_k, dst_k, st['ts'][idx], KEY(idx), efeats=st['efeats'][idx + 1], idmap=map_d,
                                   nfeats=nf[n_before:ids_upto(st, hi)])
        assert adm.n_kept == hi - lo and torch.equal(d.h[:3 * (hi - lo)], c.h[:3 * (hi - lo)])
        assert map_d.size == map_c.size == C.n_nodes == Dm.n_nodes == ids_upto(st, hi)
        admitted += map_c.size - n_before
        same_models(C, Dm, f'batch [{lo}, {hi})')
        assert torch.equal(C.raw_feat_getter.nfeats, Dm.raw_feat_getter.nfeats)
        prev = (lo, hi)
    assert admitted > 0
    assert torch.equal(map_c.key_of[:map_c.size], map_d.key_of[:map_d.size])


def test_the_online_example_fed_at_least_once_writes_the_lists_of_the_plain_replay(tmp_path):
    """examples/recommend.run_online(event_keys=True, redeliver=0.5) on toy JODIE files with an 8-wide edge table: every batch
    arrives with half of itself and half of the previous batch a second time, and the lists and metrics are those of the
    plain online replay (which is saved at its end only to make run_online return its lists)"""
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
    n, rs = len(z['src']), np.random.RandomState(0)
    z['labels'] = np.zeros(n, dtype=np.int64)
    z['efeats'] = rs.standard_normal((n + 1, 8)).astype(np.float32)
    z['efeats'][0] = 0
    z['nfeats'] = np.zeros((int(max(z['src'].max(), z['dst'].max())) + 1, 8), dtype=np.float32)
    write_files(str(tmp_path), 'toy', z)
    ckpt = str(tmp_path / 'model.pt')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    plain, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, verbose=False, offline=False, save_state=str(tmp_path / 's.pt'), **kw)
    keyed, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, verbose=False, offline=False, event_keys=True, redeliver=0.5, **kw)
    kept, dropped = keyed.pop('kept'), keyed.pop('dropped')
    assert np.array_equal(keyed.pop('ids'), plain.pop('ids')) and keyed == plain and plain['n_events'] > 0
    assert sum(kept) == plain['n_events'] and min(dropped) > 0
    with pytest.raises(ValueError, match='plain online replay only'):
        rc.run_online('toy', str(tmp_path), ckpt, k=5, verbose=False, event_keys=True, keep_last=6, **kw)
