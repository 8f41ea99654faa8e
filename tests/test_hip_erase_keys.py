"""TIGE.erase_keys and the admission of recycled ids (observe_keys / recommend_keys on a map with free ids) on the GPU; the
model and the stream are those of tests/test_hip_keyed_online.py (d = 8; the ids of the stream scrambled into keys).
  a. the keyed model against a DENSE twin that is driven by the ids the Python reference (tests/_idmap_free_ref.py) computes:
     erase(nodes=), set_node_rows, observe(num_node=) - the numbering is the same, so every tensor is compared with torch.equal;
  b. recycling against not recycling: the same keyed stream through a model that erases by id and never removes a key,
     compared per KEY through each map's own lookup;
  c. save_online and the holed map in one file, loaded by a freshly built model that continues bit for bit;
  d. refusals leave model and map unchanged;
  e. the example with --churn."""
import io

import numpy as np
import pytest
import torch

from _idmap_free_ref import RefFreeMap
from test_hip_grow_nodes import BATCHES, E0, batch, build, ids_upto, make_stream, state_of
from test_hip_keyed_online import INT64_MIN, same_models, scramble
from test_hip_rank import dev
from www2023tiger_amd.data.idmap import IdMap

pytestmark = pytest.mark.gpu


def dt(a, dtype=torch.int64):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


class Stream:
    """the stream, the key of every id of it, and who leaves when: after the batches 0 and 3, ids that come back later and
    ids that never do"""

    def __init__(self):
        self.st, self.nf = make_stream()
        st = self.st
        self.N0 = ids_upto(st, E0)
        self.key = scramble(np.arange(st['n_nodes'])).numpy()
        self.orig = {int(k): i for i, k in enumerate(self.key)}
        both = lambda lo, hi: set(st['src'][lo:hi].tolist()) | set(st['dst'][lo:hi].tolist())
        users = lambda lo, hi: sorted(set(st['src'][lo:hi].tolist()))
        self.leave = {}
        for b, n_back, n_gone in ((0, 2, 3), (3, 2, 2)):
            hi = BATCHES[b][1]
            seen, later = users(0, hi), both(hi, len(st['src']))
            seen = [x for x in seen if not any(x in v for v in self.leave.values())]
            back, gone = [x for x in seen if x in later][:n_back], [x for x in seen if x not in later][:n_gone]
            assert len(back) == n_back and len(gone) == n_gone, 'the stream no longer has who the tests need'
            self.leave[b] = back + gone
        # an item leaves too (an id with many entries), and the key of a user nobody has met: unknown, ignored
        self.leave[3].append(int(np.bincount(st['dst'][:BATCHES[3][1]]).argmax()))
        self.unknown = 987654321

    def rows(self, keys):
        """the feature rows of keys: those of the ids the stream knows them by"""
        return torch.from_numpy(self.nf[[self.orig[int(k)] for k in torch.as_tensor(keys).cpu().tolist()]]).to(dev())

    def keys_of_batch(self, lo, hi):
        src, dst, _, ts, eids = batch(self.st, lo, hi)
        return self.key[src], self.key[dst], ts, eids

    def leaving(self, b):
        return np.array([self.key[i] for i in self.leave[b]] + [self.unknown, INT64_MIN], dtype=np.int64)


@pytest.fixture(scope='module')
def S():
    return Stream()


def born(S):
    m = build(S.st, S.nf, S.N0, E0)
    m.stream_step(*batch(S.st, 0, E0))
    return m


def seeded_ref(S):
    ref = RefFreeMap()
    ref.d = {int(S.key[i]): i for i in range(1, S.N0)}
    ref.size = S.N0
    return ref


def keyed_observe(S, C, idmap, lo, hi):
    ks, kd, ts, eids = S.keys_of_batch(lo, hi)
    return C.observe_keys(idmap, dt(ks), dt(kd), ts, eids, nfeats=S.rows)


def dense_observe(S, B, ref, lo, hi):
    """what observe_keys does, by the reference's ids: grow with zero rows, write the rows of the ids given out, observe"""
    ks, kd, ts, eids = S.keys_of_batch(lo, hi)
    n0 = B.n_nodes
    ids, new = ref.assign(np.stack([ks, kd], 1).reshape(-1), return_new=True)
    admit = [int(i) for i in new if i < n0] + list(range(n0, ref.size))
    if ref.size > n0:
        B.grow_nodes(ref.size)
    if admit:
        B.set_node_rows(dt(admit), S.rows(ref.key_of()[admit]))
    step = B.observe(ids[0::2].astype(np.int64), ids[1::2].astype(np.int64), ts, eids, num_node=max(ref.size, n0))
    return step, sum(i < n0 for i in admit)


def dense_erase(B, ref, keys, eids=None):
    _, gone = ref.remove(keys)
    nodes = [int(i) for i in gone if i < B.n_nodes]
    B.erase(nodes=nodes or None, eids=eids)
    if nodes:
        B.set_node_rows(dt(nodes), 0)
    return gone


def lists_by_key(S, model, idmap, hi, k=4):
    """recommend_keys for the sources of the last events before hi that the map still holds, over the items it still holds"""
    st = S.st
    q = dt(S.key[st['src'][hi - 8:hi]])
    q = q[idmap.lookup(q) > 0]
    cand = dt(np.unique(S.key[st['dst'][:hi]]))
    cand = cand[idmap.lookup(cand) > 0]
    t = torch.full((q.numel(),), float(st['ts'][hi - 1]) + 1.0, dtype=torch.float64, device=dev())
    assert q.numel() >= 2 and cand.numel() >= k
    return q, t, cand, model.recommend_keys(idmap, q, t, None, k, cand_keys=cand)


def test_the_stream_has_keys_that_leave_arrive_and_come_back(S):
    st = S.st
    assert len(set(S.leave[0]) | set(S.leave[3])) == len(S.leave[0]) + len(S.leave[3])
    for b, hi in ((0, 100), (3, 180)):
        later = set(st['src'][hi:].tolist()) | set(st['dst'][hi:].tolist())
        assert sum(x in later for x in S.leave[b]) >= 2 and sum(x not in later for x in S.leave[b]) >= 2
    assert ids_upto(st, 240) > ids_upto(st, 180) > ids_upto(st, 100) > S.N0      # never-seen keys arrive


def test_a_keyed_model_against_a_dense_twin_driven_by_the_reference(S):
    B, C, ref = born(S), born(S), seeded_ref(S)
    idmap = IdMap.from_keys(torch.from_numpy(S.key[1:S.N0].copy()), dev())
    same_models(B, C, 'born')
    recycled = 0
    for b, (lo, hi) in enumerate(BATCHES):
        c = keyed_observe(S, C, idmap, lo, hi)
        bb, n_recycled = dense_observe(S, B, ref, lo, hi)
        recycled += n_recycled
        assert torch.equal(c.h[:3 * (hi - lo)], bb.h[:3 * (hi - lo)]), f'h of batch {b}'
        assert idmap.size == ref.size == C.n_nodes and idmap.n_free == ref.n_free
        assert torch.equal(idmap.key_of[:idmap.size].cpu(), torch.from_numpy(ref.key_of()))
        same_models(B, C, f'batch {b}')
        if b in S.leave:
            keys = S.leaving(b)
            eids = S.st['eids'][50:52] if b == 3 else None
            graph, removed = C.erase_keys(idmap, dt(keys), eids=eids)
            gone = dense_erase(B, ref, keys, eids)
            assert graph is C.graph and removed.dtype == torch.int32 and torch.equal(removed.cpu(), torch.from_numpy(gone))
            assert len(gone) == len(S.leave[b]) and idmap.n_free == ref.n_free >= len(gone)
            assert bool(idmap.is_free(removed).all()) and bool((idmap.lookup(dt(keys)) <= 0).all())
            assert not bool(C.raw_feat_getter.nfeats[removed.long()].any())
            same_models(B, C, f'after the erase behind batch {b}')
        # lists: recommend_keys on C against recommend on B by the reference's ids
        q, t, cand, got = lists_by_key(S, C, idmap, hi)
        ids, scores, n_valid = B.recommend(dt(ref.lookup(q.cpu().numpy())), t, dt(ref.lookup(cand.cpu().numpy())), 4)
        assert torch.equal(got[0].cpu(), torch.from_numpy(ref.key_of())[ids.cpu().long()]), f'lists after batch {b}'
        assert torch.equal(got[1].view(torch.int32), scores.view(torch.int32)) and torch.equal(got[2], n_valid)
    assert recycled >= 4 and idmap.size < S.st['n_stream']   # ids were handed out twice: fewer rows than the stream has ids


def run_recycling(S, upto=len(BATCHES)):
    C = born(S)
    idmap = IdMap.from_keys(torch.from_numpy(S.key[1:S.N0].copy()), dev())
    live, peak = set(S.key[1:S.N0].tolist()), S.N0 - 1
    for b, (lo, hi) in enumerate(BATCHES[:upto]):
        keyed_observe(S, C, idmap, lo, hi)
        ks, kd, _, _ = S.keys_of_batch(lo, hi)
        live |= set(ks.tolist()) | set(kd.tolist())
        peak = max(peak, len(live))
        if b in S.leave:
            C.erase_keys(idmap, dt(S.leaving(b)))
            live -= set(S.leaving(b).tolist())
    return C, idmap, live, peak


def test_recycling_against_not_recycling_per_key(S):
    """Every output element is one fixed-order accumulation over the row's own inputs, so a node's rows do not depend on
    the row's number: the two models agree bit for bit on every live key."""
    C, cmap, live, peak = run_recycling(S)
    N = born(S)
    nmap = IdMap.from_keys(torch.from_numpy(S.key[1:S.N0].copy()), dev())
    for b, (lo, hi) in enumerate(BATCHES):
        keyed_observe(S, N, nmap, lo, hi)
        if b in S.leave:
            ids = nmap.lookup(dt(S.leaving(b)))
            N.erase(nodes=ids[ids > 0].long())           # by id; the keys stay mapped to their emptied rows
    assert C.n_nodes <= peak + 1 and C.n_nodes < N.n_nodes == S.st['n_stream']   # the peak of live keys / every key ever seen
    keys = dt(sorted(live))
    ci, ni = cmap.lookup(keys).long(), nmap.lookup(keys).long()
    assert bool((ci > 0).all()) and bool((ni > 0).all()) and not torch.equal(ci, ni)      # other rows, the same nodes
    sc, sn = state_of(C), state_of(N)
    for name in ('left_vals', 'left_ts', 'left_active', 'right_vals', 'right_ts', 'right_active', 'msg_vals', 'msg_ts'):
        assert torch.equal(sc[name][ci], sn[name][ni]), name
    bit = lambda s, i: (s['has_msg'][i >> 6] >> (i & 63)) & 1
    assert torch.equal(bit(sc, ci), bit(sn, ni)), 'has_msg'
    assert torch.equal(C.raw_feat_getter.nfeats[ci], N.raw_feat_getter.nfeats[ni])
    hi = BATCHES[-1][1]
    q, t, cand, got = lists_by_key(S, C, cmap, hi)
    want = N.recommend_keys(nmap, q, t, None, 4, cand_keys=cand)
    assert torch.equal(got[2], want[2]) and int(got[2].min()) >= 4       # full lists: no padded positions to order
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), 'scores'
    assert torch.equal(got[0], want[0]), 'keys'


def test_save_and_load_with_the_holed_map_in_the_same_file(S):
    C, idmap, _, _ = run_recycling(S, upto=4)            # saved right after the second erase: the map has holes
    assert idmap.n_free > 0
    f = io.BytesIO()
    torch.save({'online': C.online_state(), 'idmap': idmap.state_dict()}, f)
    f.seek(0)
    saved = torch.load(f, weights_only=True)
    assert saved['idmap']['format'] == 'tiger-idmap-free'
    D = build(S.st, S.nf, S.N0, E0)
    D.load_online(saved['online'])
    dmap = IdMap.from_state_dict(saved['idmap'], dev())
    assert (dmap.size, dmap.n_free) == (idmap.size, idmap.n_free) and torch.equal(dmap.free_ids(), idmap.free_ids())
    same_models(C, D, 'loaded')
    lo, hi = BATCHES[4]
    c, d = keyed_observe(S, C, idmap, lo, hi), keyed_observe(S, D, dmap, lo, hi)
    assert torch.equal(c.h[:3 * (hi - lo)], d.h[:3 * (hi - lo)])
    assert dmap.size == idmap.size and torch.equal(dmap.key_of[:dmap.size], idmap.key_of[:idmap.size])
    same_models(C, D, 'one batch on')
    got, want = lists_by_key(S, D, dmap, hi)[3], lists_by_key(S, C, idmap, hi)[3]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # a key leaves on both, and a newcomer asks for a list: the same recycled id on both
    leaver = dt(S.key[S.st['src'][hi - 3:hi - 2]])
    assert torch.equal(C.erase_keys(idmap, leaver)[1], D.erase_keys(dmap, leaver)[1])
    same_models(C, D, 'after the erase')
    newcomer = dt([424242, int(S.key[S.st['src'][hi - 1]])])
    t = torch.full((2,), float(S.st['ts'][hi - 1]) + 2.0, dtype=torch.float64, device=dev())
    cand = dt(np.unique(S.key[S.st['dst'][:hi]]))
    n_free, n_nodes = idmap.n_free, C.n_nodes
    assert n_free > 0
    got = D.recommend_keys(dmap, newcomer, t, None, 3, cand_keys=cand, admit=True)
    want = C.recommend_keys(idmap, newcomer, t, None, 3, cand_keys=cand, admit=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert idmap.n_free == dmap.n_free == n_free - 1 and C.n_nodes == D.n_nodes == n_nodes
    assert int(idmap.lookup(newcomer)[0]) == int(dmap.lookup(newcomer)[0]) < n_nodes
    same_models(C, D, 'after the admission')


def test_refusals_leave_model_and_map_unchanged(S):
    C, idmap, _, _ = run_recycling(S, upto=1)
    keys = dt(S.key[S.st['src'][60:64]])

    def snapshot():
        return ([x.clone() for x in idmap.tables] + [idmap.free_bits.clone()], (idmap.size, idmap.n_free, idmap.slots_used),
                {k: v.clone() for k, v in state_of(C).items()}, C.graph, C.n_nodes, C.raw_feat_getter.nfeats.clone())

    def unchanged(before, what):
        now = snapshot()
        assert all(torch.equal(a, b) for a, b in zip(now[0], before[0])) and now[1] == before[1], what
        assert all(torch.equal(v, before[2][k]) for k, v in now[2].items()), what
        assert now[3] is before[3] and now[4] == before[4] and torch.equal(now[5], before[5]), what

    before = snapshot()
    C.train()
    with pytest.raises(RuntimeError, match='eval'):
        C.erase_keys(idmap, keys)
    C.eval()
    C._row_of = torch.zeros(C.n_nodes, dtype=torch.int32, device=dev())
    with pytest.raises(RuntimeError, match='partitioned'):
        C.erase_keys(idmap, keys)
    C._row_of = None
    with pytest.raises(ValueError, match='int64'):
        C.erase_keys(idmap, keys.int())
    with pytest.raises(ValueError, match='lives on'):
        C.erase_keys(IdMap('cpu'), keys)
    with pytest.raises(ValueError):                       # what erase refuses: a negative eid
        C.erase_keys(idmap, keys, eids=[-1])
    unchanged(before, 'erase_keys')
    # unknown keys and the padding key alone: nothing to erase, nothing removed
    graph, removed = C.erase_keys(idmap, dt([S.unknown, INT64_MIN]))
    assert graph is before[3] and removed.numel() == 0
    unchanged(before, 'unknown keys')
    # feature rows of another shape are refused before the model grows; the keys stay assigned, as without free ids
    assert idmap.n_free > 0
    lo, hi = BATCHES[1]
    ks, kd, ts, eids = S.keys_of_batch(lo, hi)
    kd = kd.copy()
    kd[0] = 31337                                         # a never-seen key: it takes a free id
    with pytest.raises(ValueError, match='admitted node ids'):
        C.observe_keys(idmap, dt(ks), dt(kd), ts, eids, nfeats=torch.zeros(7, 8))
    assert int(idmap.lookup(dt([31337]))[0]) > 0 and idmap.n_free < before[1][1]
    now = snapshot()
    assert all(torch.equal(v, before[2][k]) for k, v in now[2].items()) and now[3] is before[3] and now[4] == before[4]
    # set_node_rows: the refusals of append_node_rows, and its own
    fg = C.raw_feat_getter
    for ids, rows, exc, pattern in ((dt([1, 2]), torch.zeros(2, 7), ValueError, 'width'), (dt([1, 2]), torch.zeros(3, 8), ValueError, 'rows'),
                                    (dt([1, 2]), 5, ValueError, '0 for zero rows'), (dt([1, C.n_nodes]), 0, ValueError, 'outside'),
                                    (dt([-1]), 0, ValueError, 'outside'), (dt([[1]]), 0, ValueError, '1-d'),
                                    (torch.tensor([1.0]), 0, ValueError, '1-d')):
        with pytest.raises(exc, match=pattern):
            fg.set_node_rows(ids, rows)
    assert torch.equal(fg.nfeats, before[5])
    fg.set_node_rows(dt([3, 1], torch.int32), torch.ones(2, 8))
    assert bool((fg.nfeats[[1, 3]] == 1).all()) and torch.equal(fg.nfeats[2], before[5][2])
    fg.set_node_rows(dt([3]), 0)
    assert not bool(fg.nfeats[3].any())


def test_the_online_example_with_churn(tmp_path, capsys):
    """examples/recommend.run_online(keyed=True, grow=True, churn=FILE) on the toy files of test_hip_keyed_online: the keys
    the file names leave behind their batch, the replay prints released / recycled / n_nodes per batch, and the model ends
    smaller than the replay without churn although it met the same keys"""
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
    whole, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, verbose=False, **kw)
    n_batches = len(whole['admitted'])
    # behind batch 0 three users of the training set leave who never come back, and two keys the split brings later (unknown
    # by then, or admitted: both are fine); behind batch 1 a key nobody knows
    cut = int(len(z['src']) * 0.8)                       # (the test split is the last 15 %)
    users = np.setdiff1d(z['src'][:cut], np.concatenate([z['src'][cut:], z['dst']]))[:3]   # they never come back
    assert len(users) == 3
    churn = tmp_path / 'churn.txt'
    churn.write_text('# batch key\n' + ''.join(f'0 {int(rc.scramble(np.array([u]))[0])}\n' for u in list(users) + [top + 1, top + 2])
                     + '1 123456789\n')
    capsys.readouterr()
    out, _ = rc.run_online('toy', str(tmp_path), ckpt, k=5, keyed=True, grow=True, churn=str(churn), **kw)
    said = capsys.readouterr().out
    assert said.count('released') == n_batches and said.count('recycled') == n_batches and said.count('n_nodes') >= n_batches
    assert len(out['released']) == len(out['recycled']) == n_batches
    assert out['released'][0] >= 3 and out['released'][1] == 0 and sum(out['released'][2:]) == 0
    assert sum(out['recycled']) >= 1 and sum(out['recycled']) <= sum(out['released'])
    assert out['n_nodes'] < whole['n_nodes'] and out['ids'].shape == whole['ids'].shape
    with pytest.raises(ValueError, match='--keyed'):
        rc.run_online('toy', str(tmp_path), ckpt, k=5, grow=True, churn=str(churn), verbose=False, **kw)
