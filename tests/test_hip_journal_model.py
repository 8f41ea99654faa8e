"""TIGE.journal / OnlineJournal.save / TIGE.apply_online_delta on the GPU.  Model B journals a base and then a delta after
every step of: observe, observe with growth and feature rows, forget(keep_last), erase, observe_late, restart_involved, a
one-event batch, release_edge_rows (forces a base) and one more batch.  Model C - freshly built on a three-event stub graph
and stub tables, with OTHER parameters - loads the base and applies the deltas.  After EVERY file B and C are compared with
torch.equal (every buffer, both tables, the four graph arrays, recommendations), and from every file on both continue equal
for two more batches.  The builders are those of tests/test_hip_online_state.py (d = 8 and 16, 77 node ids, ragged batches)."""
import io

import numpy as np
import pytest
import torch

from test_hip_online_state import (E0, KEYS, assert_same, assert_twins, bits, build, copy_of, everything, ids_upto, observe, stream)
from test_hip_rank import dev
from www2023tiger_amd import hip_ops

pytestmark = pytest.mark.gpu

VARIANTS = {
    'one-layer': dict(d=8),
    'fused+eager': dict(d=16, K=10, forms=('fused', 'eager')),
    'two-layers-recent-nodes': dict(d=8, L=2, strategy='recent_nodes'),
}
STEPS = ('observe', 'grow', 'forget', 'erase', 'late', 'restart', 'one', 'release', 'after-release')
KINDS = dict.fromkeys(STEPS, 'delta')
KINDS['release'] = 'base'


def feed(m, st, nf, lo, hi):
    """observe events [lo, hi) with their rows appended to m's edge table, admitting the ids they bring -> h"""
    rows = m.raw_feat_getter.efeats.shape[0]
    n_now = max(m.n_nodes, ids_upto(st, hi))
    return observe(m, st, lo, hi, eids=np.arange(rows, rows + hi - lo), num_node='auto',
                   nfeats=torch.from_numpy(nf[m.n_nodes:n_now]))


def step(m, st, nf, name, pos):
    """one step of the sequence on model m -> the stream position afterwards"""
    if name == 'observe':
        assert m.n_nodes == ids_upto(st, 80)
        rows = m.raw_feat_getter.efeats.shape[0]
        observe(m, st, 40, 80, eids=np.arange(rows, rows + 40))
        return 80
    if name == 'grow':
        n0 = m.n_nodes
        feed(m, st, nf, 80, 118)
        assert m.n_nodes > n0, 'the batch brings new ids'
        return 118
    if name == 'forget':
        m.forget(keep_last=4)
    elif name == 'erase':
        live = m.graph._tensors()[3] & 0x7FFFFFFF
        m.erase(nodes=torch.tensor([int(st['src'][50]), int(st['dst'][60])]), eids=live[live > 0][:2].cpu())
    elif name == 'late':
        rows = m.raw_feat_getter.efeats.shape[0]
        d_e = m.raw_feat_getter.efeats.shape[1]
        m.observe_late(np.array([int(st['src'][45]), int(st['src'][100])]), np.array([int(st['dst'][70]), int(st['dst'][30])]),
                       np.array([float(st['ts'][50]), float(st['ts'][20])]), np.array([rows, rows + 1]),
                       efeats=torch.full((2, d_e), 0.25))
    elif name == 'restart':
        nodes = torch.unique(torch.from_numpy(np.concatenate([st['src'][80:118], st['dst'][80:118]]))).to(dev())
        t = torch.full((nodes.numel(),), float(st['ts'][117]) + 1.0, dtype=torch.float64, device=dev())
        assert m.restart_involved(nodes, t, hip_ops.new_bitmap(m.n_nodes, dev())) > 0
    elif name == 'one':
        feed(m, st, nf, 118, 119)
        return 119
    elif name == 'release':
        assert m.release_edge_rows().shift > 0
    elif name == 'after-release':
        feed(m, st, nf, 119, 140)
        return 140
    return pos


def start(kw, **build_kw):
    """B: a model on the ids of the first 80 events over the first 40, streamed once; -> st, nf, B"""
    st, nf = stream(kw['d'])
    B = build(st, nf, ids_upto(st, 80), E0, **kw, **build_kw)
    B.stream_step(*(st[k][:E0] for k in ('src', 'dst', 'dst', 'ts', 'eids')))
    return st, nf, B


def fresh(st, nf, kw):
    C = build(st, nf, ids_upto(st, 80), 3, seed=99, stub=True, **kw)
    return C


def saved(J):
    f = io.BytesIO()
    kind = J.save(f)
    f.seek(0)
    return kind, f


def take(C, kind, f):
    g0 = C.graph
    g = C.load_online(f) if kind == 'base' else C.apply_online_delta(f)
    assert g is C.graph and g is not g0


@pytest.mark.parametrize('stop', range(len(STEPS) + 1))
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_a_fresh_model_follows_the_files_and_continues(variant, stop):
    """files 0 .. stop, compared after every one; then two more batches on both"""
    kw = VARIANTS[variant]
    st, nf, B = start(kw)
    C = fresh(st, nf, kw)
    assert not torch.equal(C.score_fn.fc1.weight, B.score_fn.fc1.weight)
    J = B.journal()
    assert B.journal() is J and J.whole
    kind, f = saved(J)
    assert kind == 'base' and (J.seq, J.whole) == (0, False)
    take(C, kind, f)
    assert C._journal is not None and (C._journal.chain, C._journal.seq) == (J.chain, 0)
    pos = E0
    assert_twins(B, C, st, pos, 'after the base')
    seq = 0
    for name in STEPS[:stop]:
        pos = step(B, st, nf, name, pos)
        kind, f = saved(J)
        assert kind == KINDS[name], f'{name}: {kind} ({J.reason})'
        seq = 0 if kind == 'base' else seq + 1
        assert J.seq == seq and not J.whole and not bool(J.state_bits.any()) and not bool(J.graph_bits.any())
        take(C, kind, f)
        assert (C._journal.chain, C._journal.seq) == (J.chain, seq)
        assert_twins(B, C, st, pos, f'after the file of {name!r}')
    for lo, hi in ((pos, pos + 13), (pos + 13, pos + 30)):
        hb, hc = feed(B, st, nf, lo, hi), feed(C, st, nf, lo, hi)
        assert torch.equal(bits(hb), bits(hc)), f'h of batch [{lo}, {hi}) after {stop} steps'
        assert_twins(B, C, st, hi, f'after batch [{lo}, {hi}) after {stop} steps')


def run_files(kw, steps, hook=None):
    """B through `steps`, a file after each -> st, nf, B, [(kind, loaded dict)]"""
    st, nf, B = start(kw)
    J = B.journal()
    files, pos = [], E0
    for name in (None,) + tuple(steps):
        if name is not None:
            pos = step(B, st, nf, name, pos)
        if hook is not None:
            hook(B, name)
        kind, f = saved(J)
        files.append((kind, torch.load(f, map_location='cpu', weights_only=True)))
    return st, nf, B, files


def same_value(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    return type(a) is type(b) and a == b


def test_a_cleared_tracker_changes_no_file_and_a_saved_journal_clears_no_tracker():
    kw, steps = VARIANTS['one-layer'], STEPS[:6]
    plain = run_files(kw, steps)[3]
    seen = {}

    def hook(B, name):
        tr = B.track_changes()
        if name == 'observe':
            assert bool(tr.bits.any())
            seen['before'] = tr.bits.clone()
        if name == 'grow':   # the journal saved (and cleared its own bitmaps) in between: the tracker kept its bits
            assert bool((tr.bits[:seen['before'].numel()] & seen['before']).eq(seen['before']).all())
            tr.clear()
        if name == 'forget':
            assert not tr.whole and bool(tr.bits.any())
    tracked = run_files(kw, steps, hook)[3]
    assert [k for k, _ in plain] == [k for k, _ in tracked] == ['base'] + ['delta'] * 6
    for (_, a), (_, b), name in zip(plain, tracked, ('base',) + steps):
        a, b = dict(a, chain=0), dict(b, chain=0)   # (the chain id is drawn at random)
        assert same_value(a, b), name


def tensor_bytes(v):
    if torch.is_tensor(v):
        return v.numel() * v.element_size()
    return sum(tensor_bytes(x) for x in v.values()) if isinstance(v, dict) else 0


def test_the_payload_of_a_delta_is_the_dirty_rows_and_nothing_else():
    kw = VARIANTS['one-layer']
    st, nf, B, files = run_files(kw, STEPS[:7])
    d = kw['d']
    per_node = 2 * (4 * d + 4 + 1) + 4 * (3 * d + d) + 4 + 1 + 4 * d   # two memories, mailbox row + time + has-message byte, node row
    full = tensor_bytes(B.online_state())
    for (kind, f), name in zip(files[1:], STEPS[:7]):
        assert kind == 'delta' and f['format'] == 'tiger-online-delta' and f['version'] == 1
        D, Dg, P = f['ids'].numel(), f['rows'].numel(), f['ts'].numel()
        tail = f['efeat_rows_after'] - f['efeat_rows_before']
        fixed = 624 * 8 + (625 * 4 if f['graph_state']['mt_state'] is not None else 0)
        # (a packed entry is ts float64 + nbr int32 + eid int32: 16 bytes)
        want = D * (per_node + 4) + Dg * 4 + (Dg + 1) * 8 + P * 16 + tail * d * 4 + fixed
        got = tensor_bytes(f)
        print(f'{name}: D_state={D} D_graph={Dg} packed={P} tail={tail} bytes={got} (full state {full})')
        assert got == want, name
        assert f['n_nodes_after'] > max(D, Dg), 'the case would not tell a whole table from the dirty rows'
        for k, t in f['rows_of'].items():
            assert t.shape[0] == D, f'{name}: rows_of[{k}] carries {t.shape[0]} rows for {D} dirty ids'
        assert f['has_msg'].shape == (D,) and f['off'].shape == (Dg + 1,) and f['efeats_tail'].shape == (tail, d)
        assert f['nbr'].numel() == f['eid'].numel() == P == int(f['off'][-1])
        assert not any(k in f for k in ('state_dict', 'mailbox', 'nfeats', 'efeats', 'graph')), 'a delta carries no table whole'
    by = dict(zip(STEPS[:7], (f for _, f in files[1:])))
    assert by['restart']['rows'].numel() == 0 and by['restart']['ts'].numel() == 0 and by['restart']['ids'].numel() > 0, \
        'a restart does not drag T-CSR rows into the file'
    assert by['forget']['ids'].numel() == 0 and by['forget']['rows'].numel() > 0, 'a trim dirties T-CSR rows only'
    assert 1 <= by['one']['ids'].numel() <= 2 and 1 <= by['one']['rows'].numel() <= 2   # one event: at most two nodes
    assert by['grow']['n_nodes_after'] > by['grow']['n_nodes_before']
    assert by['late']['efeat_rows_after'] == by['late']['efeat_rows_before'] + 2


def refused(C, state, exc, pattern):
    before, g0, J = everything(C), C.graph, C._journal
    t0 = (C.raw_feat_getter.nfeats, C.raw_feat_getter.efeats)
    at = (J.chain, J.seq)
    with pytest.raises(exc, match=pattern):
        C.apply_online_delta(state)
    assert C.graph is g0 and C.raw_feat_getter.nfeats is t0[0] and C.raw_feat_getter.efeats is t0[1]
    assert C._journal is J and (J.chain, J.seq) == at
    assert_same(everything(C), before, 'after a refusal')


def test_refusals_leave_the_model_as_it_was():
    kw = VARIANTS['one-layer']
    st, nf, B, files = run_files(kw, STEPS[:2])
    (_, base), (_, d1), (_, d2) = files
    assert d2['ids'].numel() > 2 and d2['rows'].numel() > 2 and d2['nbr'].numel() > 0 and d2['n_nodes_after'] > d2['n_nodes_before']
    C = fresh(st, nf, kw)
    with pytest.raises(ValueError, match='chain'):
        C.apply_online_delta(copy_of(d1))                         # no base was loaded: the model follows no chain
    C.load_online(copy_of(base))
    refused(C, copy_of(d2), ValueError, 'seq 2 is not the successor')          # out of order
    refused(C, dict(copy_of(d1), chain=d1['chain'] ^ 1), ValueError, 'chain')  # another chain
    C.apply_online_delta(copy_of(d1))
    refused(C, copy_of(d1), ValueError, 'seq 1 is not the successor')          # applied twice
    n1 = d2['n_nodes_after']

    def corrupt(**kv):
        s = copy_of(d2)
        for k, fn in kv.items():
            s[k] = fn(s[k])
        return s

    def put(index, value):
        def fn(t):
            t = t.clone()
            t[index] = value
            return t
        return fn
    swap = lambda t: torch.cat([t[1:2], t[0:1], t[2:]])
    cases = [(corrupt(off=lambda t: t[:-1].clone()), 'off is'),                  # a truncated off
             (corrupt(off=put(1, -1)), 'off must start at 0'),
             (corrupt(ids=swap), 'ids must ascend'),                              # unsorted ids
             (corrupt(ids=put(-1, n1)), 'ids must ascend strictly inside'),      # an id beyond n_nodes_after
             (corrupt(rows=put(-1, n1)), 'rows must ascend'),
             (corrupt(nbr=put(0, n1)), 'NBR_RANGE.*entry'),                       # caught by tg_tcsr_verify
             (corrupt(ts=put(0, float('nan'))), 'TS_NAN'),
             (corrupt(eid=put(0, d2['efeat_rows_after'])), 'EID_RANGE'),
             (corrupt(has_msg=lambda t: t[:-1].clone()), 'has_msg'),
             (corrupt(efeats_tail=lambda t: t[:-1].clone()), 'efeats_tail'),
             (corrupt(n_nodes_before=lambda v: v + 1), 'n_nodes_before'),
             (corrupt(num_entry_before=lambda v: v + 2), 'num_entry_before'),
             (corrupt(num_entry_after=lambda v: v + 2), 'num_entry_after'),
             (corrupt(efeat_rows_before=lambda v: v - 1), 'efeat_rows_before'),
             (corrupt(n_nodes_after=lambda v: d2['n_nodes_before'] - 1), 'n_nodes_after'),
             (corrupt(version=lambda v: 2), 'version 2'),
             (corrupt(format=lambda v: 'tiger-online-state'), 'format'),
             (corrupt(fingerprint=lambda v: dict(v, dim=16)), r"fingerprint.*'dim': \(16, 8\)")]
    s = copy_of(d2)
    s['rows_of']['left.vals'] = s['rows_of']['left.vals'][:, :-1].clone()
    cases.append((s, r"rows_of\['left.vals'\]"))
    s = copy_of(d2)
    s['graph_state']['t_last'] = float(d2['ts'].max()) - 1.0
    cases.append((s, 't_last'))
    for state, pattern in cases:
        refused(C, state, ValueError, pattern)
    refused(C, base, ValueError, 'format')                                      # a base is no delta
    C3 = fresh(st, nf, kw)
    C3.load_online(copy_of(base))
    C3.train()                                      # training mode (and train() says that parameters are about to change:
    refused(C3, copy_of(d1), RuntimeError, 'eval')  # the model has left the chain and wants a base)
    C3.eval()
    refused(C3, copy_of(d1), ValueError, 'left the chain')
    C._row_of = torch.zeros(1, dtype=torch.int32)   # what partition_state leaves behind
    refused(C, copy_of(d2), RuntimeError, 'partitioned')
    del C._row_of
    C.observe_late(np.array([3]), np.array([4]), np.array([1.0]), np.array([1]))   # the model moves on by itself:
    with pytest.raises(ValueError, match='num_entry_before'):                      # it is no longer the delta's predecessor
        C.apply_online_delta(copy_of(d2))
    C2 = fresh(st, nf, kw)
    C2.load_online(copy_of(base))
    C2.apply_online_delta(copy_of(d1))
    C2.apply_online_delta(copy_of(d2))                                             # and the uncorrupted delta applies
    assert_twins(B, C2, st, 118, 'after the uncorrupted files')


def test_the_online_example_journals_and_a_replay_from_the_files_writes_the_same_lists(tmp_path):
    """examples/recommend.run_online on toy JODIE files, forgetting on the way: a replay that journals (a base, then a delta per
    batch) and stops after two batches, and one that loads the base, applies the deltas and goes on, give between them the
    lists of the replay that was never interrupted"""
    import json
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
    ckpt, jdir = str(tmp_path / 'model.pt'), str(tmp_path / 'journal')
    kw = dict(seed=0, bs=100, dim=8, n_neighbors=4, hist_len=6, restarter_type='seq')
    lp.run('toy', str(tmp_path), n_epochs=1, lr=1e-3, ckpt_path=ckpt, **kw)
    on = dict(k=5, keep_last=6, verbose=False, offline=False, **kw)
    whole, _ = rc.run_online('toy', str(tmp_path), ckpt, journal=str(tmp_path / 'all'), journal_every=2, **on)
    assert whole['journal'][0] == 'base' and set(whole['journal'][1:]) == {'delta'} and len(whole['journal']) >= 2
    head, _ = rc.run_online('toy', str(tmp_path), ckpt, journal=jdir, save_after=2, **on)
    assert head['journal'] == ['base', 'delta', 'delta'] and head['n_events'] == 200
    with open(os.path.join(jdir, 'index.json')) as f:
        index = json.load(f)
    assert [x['next_event'] for x in index] == [0, 100, 200]
    sizes = [os.path.getsize(os.path.join(jdir, x['file'])) for x in index]
    assert max(sizes[1:]) < sizes[0]
    tail, _ = rc.run_online('toy', str(tmp_path), ckpt, load_state=os.path.join(jdir, index[0]['file']), apply_deltas=jdir, **on)
    assert tail['n_events'] == whole['n_events'] - 200 > 0
    np.testing.assert_array_equal(np.concatenate([head['ids'], tail['ids']]), whole['ids'])
    with pytest.raises(ValueError, match='no base file'):
        rc.run_online('toy', str(tmp_path), ckpt, load_state=os.path.join(jdir, index[1]['file']), apply_deltas=jdir, **on)


def test_what_the_journal_itself_refuses_and_what_forces_a_base(tmp_path):
    kw = VARIANTS['one-layer']
    st, nf, B = start(kw)
    J = B.journal()
    B.train()
    with pytest.raises(RuntimeError, match='eval'):
        J.save(tmp_path / 'x.pt')
    B.eval()           # (train() told the sinks that parameters are about to change)
    assert J.whole and J.chain is None and J.seq == -1
    assert J.save(tmp_path / 'base.pt') == 'base'
    chain = J.chain
    step(B, st, nf, 'observe', E0)
    state = (J.seq, J.state_bits.clone(), J.graph_bits.clone())
    with pytest.raises(Exception):
        J.save(tmp_path / 'no-such-directory' / 'd.pt')      # the save raises: the journal is unchanged
    assert (J.seq, J.chain, J.whole) == (state[0], chain, False)
    assert torch.equal(J.state_bits, state[1]) and torch.equal(J.graph_bits, state[2]) and bool(state[1].any())
    assert J.save(tmp_path / 'd1.pt') == 'delta' and J.seq == 1
    for why, act in (('flush_msg', lambda: B.flush_msg()), ('reset', lambda: B.reset()),
                     ('load_state_dict', lambda: B.load_state_dict(B.state_dict()))):
        act()
        assert J.whole, why
        assert J.save(tmp_path / 'b.pt') == 'base' and J.chain != chain and J.seq == 0, why
        chain = J.chain
    # a file written by save_online (no chain, no seq) loads as before and installs no journal
    C = fresh(st, nf, kw)
    B.save_online(tmp_path / 'plain.pt')
    C.load_online(tmp_path / 'plain.pt')
    assert C._journal is None
    with pytest.raises(ValueError, match='chain'):
        C.load_online(dict(B.online_state(), chain=-3, seq=0))
