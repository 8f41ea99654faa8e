"""tests/_state_ref.py (the NumPy state machine the state-kernel tests compare with) against the oracle:
store_events, consume, _mem_set, restart and whole stream steps on random small streams with a hub, self-loops and
float32 time ties, both message sources, with and without feature tables.  CPU only.

Tables must match bit for bit after every batch, except the mailbox's time segment: the oracle takes torch's float32
cosine, the reference rounds a float64 cosine of the same float32 argument, and both are within one unit in the last
place of values below 1 of the exact cosine, so they differ by at most 2^-23."""
import numpy as np
import pytest
import torch

import _state_ref as S
from _util import fixture_params, load, parse_cfg
from oracle import tiger_oracle as O
from www2023tiger_amd import _lib

FIXTURE = 'seq_lr_d8'      # d = d_e = 8, 56 nodes, 600 edge rows: its parameters serve every variant below
TE_TOL = 2.0 ** -23
BIT_OF_TEXT = {text: bit for bit, text in _lib.ERR_TEXT.items()}


def bit_of(exc):
    msg = str(exc)
    if 'has unused messages' in msg:   # the oracle names the node, the table of texts does not
        return _lib.ERR_UNUSED_MESSAGE
    return BIT_OF_TEXT[msg]


def make_stream(n_nodes, E, seed, times):
    rs = np.random.RandomState(seed)
    src = rs.randint(1, n_nodes, E).astype(np.int64)
    dst = rs.randint(1, n_nodes, E).astype(np.int64)
    src[rs.uniform(size=E) < 0.3] = 7                      # a hub
    loops = rs.uniform(size=E) < 0.1
    dst[loops] = src[loops]                                # self-loops
    if times == 'floor':                                   # equal float64 (and float32) times
        ts = np.floor(np.sort(rs.uniform(0, E / 4.0, E)))
    else:                                                  # float64 times that differ and collapse in float32
        ts = 2.5e6 + 0.05 * np.arange(E)
    return src, dst, ts, np.arange(1, E + 1, dtype=np.int64), rs.randint(1, n_nodes, E).astype(np.int64)


def build(msg_src, with_nf, with_ef, times, seed):
    z = load(FIXTURE)
    cfg = parse_cfg(z)
    n_nodes, d = int(z['n_nodes']), cfg['d']
    src, dst, ts, eids, neg = make_stream(n_nodes, 240, seed, times)
    rs = np.random.RandomState(seed + 100)
    nf = rs.standard_normal((n_nodes, d)).astype(np.float32) if with_nf else None
    ef = rs.standard_normal((len(src) + 1, d)).astype(np.float32) if with_ef else None
    g = O.OracleGraph(src, dst, ts, eids, max_node_id=n_nodes - 1)
    orc = O.OracleTIGER(fixture_params(z, cfg), g, n_nodes=n_nodes, dim=d, nfeats=nf, efeats=ef, n_neighbors=cfg['K'],
                        msg_src=msg_src, upd_src=cfg['upd_src'], restarter=cfg['restarter'], hist_len=cfg['H'])
    st = S.State(n_nodes, d, d, msg_src, orc.p['time_encoder.basis_freq'].numpy(), orc.p['time_encoder.phase'].numpy(),
                 nf, ef)
    return orc, st, (src, dst, ts, eids, neg), cfg


ORACLE_TABLES = ('left_vals', 'left_ts', 'right_vals', 'right_ts', 'msg_vals', 'msg_ts')


def push(st, orc):
    """reference state -> oracle"""
    for k in ORACLE_TABLES:
        setattr(orc, k, torch.from_numpy(getattr(st, k).copy()))
    orc.has_msg = st.has_msg.copy()


def assert_same(st, orc, what):
    d, d_e = st.d, st.d_e
    for k in ORACLE_TABLES:
        a, b = getattr(st, k), getattr(orc, k).numpy()
        if k == 'msg_vals':
            np.testing.assert_array_equal(a[:, :2 * d + d_e].view(np.uint32), b[:, :2 * d + d_e].view(np.uint32),
                                          err_msg=f'{what}: {k}')
            assert np.abs(a[:, 2 * d + d_e:].astype(np.float64) - b[:, 2 * d + d_e:]).max() <= TE_TOL, what
        else:
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f'{what}: {k}')
    np.testing.assert_array_equal(st.has_msg, orc.has_msg, err_msg=f'{what}: has_msg')


def up(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(np.inf))
    return x


def corrupt(st, rs, batch, involved, kind):
    """one time moved one float32 step to the wrong side (or, kind 0, to equality: no violation)"""
    src, dst, ts32 = batch['src'], batch['dst'], batch['ts32']
    pos = np.concatenate([src, dst])
    i = rs.randint(len(pos))
    v, t = pos[i], np.tile(ts32, 2)[i]
    pend = [u for u in np.unique(involved) if st.has_msg[u]]
    if kind == 0:
        st.mem()[1][v] = min(st.mem()[1][v], t)
    elif kind == 1:      # event before the message-source memory
        st.mem()[1][v] = up(np.tile(ts32, 2)[pos == v].min())
        if st.msg_src == 'right' and st.has_msg[v]:   # STEP 4 moves the right memory to the message's time first
            st.msg_ts[v] = st.right_ts[v]
    elif kind == 2:     # left memory after the event
        st.left_ts[v] = up(t)
    elif kind == 3 and pend:   # message before memory, on any involved node
        u = pend[rs.randint(len(pend))]
        st.msg_ts[u] = np.nextafter(st.mem()[1][u], np.float32(-np.inf))
    elif kind == 4 and pend:   # right memory after the message
        u = pend[rs.randint(len(pend))]
        st.right_ts[u] = up(st.msg_ts[u])
    elif kind == 5 and pend:   # message time above the memory's (a mismatch with msg_src = left, nothing otherwise)
        u = pend[rs.randint(len(pend))]
        st.msg_ts[u] = up(st.msg_ts[u])


def oracle_step(orc, batch, cg):
    """-> (None, rows, new_row, left_row) or (exception, ...): the oracle's batch, and the rows STEP 4 / STEP 6 wrote"""
    src, dst, B = batch['src'], batch['dst'], len(batch['src'])
    d = orc.d
    rows, new_row = np.zeros((2 * B, d), np.float32), np.zeros(2 * B, np.int64)
    try:
        with torch.no_grad():
            outdated, h_new, _ = orc.consume(cg['involved'])
            if len(outdated):
                where = np.minimum(np.searchsorted(outdated, np.concatenate([src, dst])), len(outdated) - 1)
                rows = np.concatenate([rows, h_new.numpy()])
                new_row = 2 * B + where   # (read only for nodes with a pending message: those are in `outdated`)
            h = orc.stream_step(src, dst, batch['neg'], batch['ts'], batch['eids'], cg).numpy()
        rows[:2 * B] = h
        return None, rows, new_row, np.arange(2 * B)
    except ValueError as e:
        return e, rows, new_row, np.arange(2 * B)


@pytest.mark.parametrize('times', ['floor', 'collapse'])
@pytest.mark.parametrize('with_ef', [False, True])
@pytest.mark.parametrize('with_nf', [False, True])
@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_stream_steps_match_oracle(msg_src, with_nf, with_ef, times):
    orc, st, (src, dst, ts, eids, neg), cfg = build(msg_src, with_nf, with_ef, times, seed=5)
    rs = np.random.RandomState(9)
    B, raised, clean = 24, set(), 0
    for b in range(len(src) // B):
        sl = slice(b * B, (b + 1) * B)
        batch = dict(src=src[sl], dst=dst[sl], neg=neg[sl], ts=ts[sl], ts32=ts[sl].astype(np.float32), eids=eids[sl])
        cg = O.collate(orc.graph, batch['src'], batch['dst'], batch['neg'], batch['ts'], cfg['K'], cfg['restarter'],
                       cfg['H'])
        for kind in ([None] if b < 2 else [None, 0, 1, 2, 3, 4, 5]):
            trial = st.copy()
            if kind is not None:
                corrupt(trial, rs, batch, cg['involved'], kind)
            push(trial, orc)
            exc, rows, new_row, left_row = oracle_step(orc, batch, cg)
            word = S.step_invariants(trial, batch, cg['involved'])
            word |= S.writeback(trial, batch, rows, new_row, left_row)
            assert (word == 0) == (exc is None), (b, kind, word, exc)
            if exc is not None:
                assert word & bit_of(exc), (b, kind, word, exc)
                raised.update(b_ for b_ in _lib.ERR_TEXT if word & b_)
            else:
                assert_same(trial, orc, f'batch {b} kind {kind}')
                clean += 1
            if kind is None:
                assert exc is None
                keep = trial
        st = keep
    assert clean >= len(src) // B
    want = {_lib.ERR_PAST_MEMORY, _lib.ERR_MSG_BEFORE_MEM, _lib.ERR_EVENT_BEFORE_MEM}
    if msg_src == 'left':
        want.add(_lib.ERR_MSG_TS_MISMATCH)
    assert want <= raised, raised   # (every check fired at least once, in the oracle or behind its first raise)


def test_winners_match_select_latest():
    rs = np.random.RandomState(0)
    for B in (1, 3, 40, 200):   # 200: the oracle's vectorised branch
        src, dst = rs.randint(0, 9, B), rs.randint(0, 9, B)
        for ts in (np.floor(rs.uniform(0, 5, B)), np.full(B, 3.0), 2.5e6 + 0.05 * np.arange(B)):
            ts32 = ts.astype(np.float32)
            u, idx = S.winners(src, dst, ts32)
            ru, ridx = O.select_latest_nids(np.concatenate([src, dst]), np.tile(ts32, 2))
            np.testing.assert_array_equal(u, ru)
            np.testing.assert_array_equal(idx, ridx)


@pytest.mark.parametrize('with_feats', [False, True])
@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_store_events_matches_oracle(msg_src, with_feats):
    orc, st, (src, dst, ts, eids, _), _ = build(msg_src, with_feats, with_feats, 'floor', seed=11)
    rs = np.random.RandomState(1)
    for k in ('left_vals', 'right_vals', 'msg_vals'):
        getattr(st, k)[:] = rs.standard_normal(getattr(st, k).shape)
    B = 40
    s, dd, t32, e = src[:B], dst[:B], (ts[:B] + 50).astype(np.float32), eids[:B]
    st.left_ts[:] = rs.randint(0, 50, st.n_nodes)
    st.right_ts[:] = rs.randint(0, 50, st.n_nodes)
    pos = np.concatenate([s, dd])
    for case in ('clean', 'equal', 'before', 'unused'):
        trial = st.copy()
        v = pos[B + 3]
        first = np.tile(t32, 2)[pos == v].min()
        if case == 'equal':
            trial.mem()[1][v] = first
        elif case == 'before':
            trial.mem()[1][v] = up(first)
        elif case == 'unused':
            trial.has_msg[v] = True
        push(trial, orc)
        exc = None
        try:
            orc.store_events(s, dd, torch.from_numpy(t32), e)
        except ValueError as err:
            exc = err
        word = S.store_events(trial, s, dd, t32, e)
        expect = {'clean': 0, 'equal': 0, 'before': S.ERR_EVENT_BEFORE_MEM, 'unused': S.ERR_UNUSED_MESSAGE}[case]
        assert word == expect, case
        assert (exc is None) == (word == 0)
        if exc is None:
            assert_same(trial, orc, case)
        else:
            assert word == bit_of(exc)


def test_consume_update_right_matches_mem_set():
    orc, st, _, _ = build('left', False, False, 'floor', seed=2)
    rs = np.random.RandomState(3)
    st.right_vals[:] = rs.standard_normal(st.right_vals.shape)
    st.right_ts[:] = rs.randint(0, 50, st.n_nodes)
    st.msg_ts[:] = st.right_ts + rs.randint(0, 3, st.n_nodes)   # equal times among them
    st.has_msg[:] = rs.uniform(size=st.n_nodes) < 0.5
    involved = np.unique(rs.randint(0, st.n_nodes, 40))
    upos = rs.permutation(involved)[:17]
    rows = rs.standard_normal((len(involved), st.d)).astype(np.float32)
    for bad in (False, True):
        for form in ('rank', 'rows'):
            trial = st.copy()
            if bad:
                v = upos[trial.has_msg[upos]][0]
                trial.right_ts[v] = up(trial.msg_ts[v])
            push(trial, orc)
            ids = upos[trial.has_msg[upos]]
            exc = None
            try:
                orc._mem_set(orc.right_vals, orc.right_ts, torch.from_numpy(ids),
                             torch.from_numpy(rows[np.searchsorted(involved, ids)]), orc.msg_ts[torch.from_numpy(ids)])
                orc.has_msg[ids] = False
            except ValueError as err:
                exc = err
            if form == 'rank':
                word = S.consume_update_right(trial, upos, rows, involved=involved)
            else:
                word = S.consume_update_right(trial, upos, rows, row_index=np.searchsorted(involved, upos))
            assert word == (S.ERR_PAST_MEMORY if bad else 0)
            if bad:
                assert bit_of(exc) == word
            else:
                assert exc is None
                assert_same(trial, orc, form)
                assert trial.right_active[ids].all() and trial.right_active.sum() == len(ids)
    g = S.mailbox_consume_gather(st, involved)
    np.testing.assert_array_equal(g, st.right_vals[involved])


@pytest.mark.parametrize('msg_src', ['left', 'right'])
def test_restart_matches_oracle(msg_src):
    orc, st, (src, dst, ts, _, _), _ = build(msg_src, True, True, 'floor', seed=4)
    rs = np.random.RandomState(5)
    for k in ('left_vals', 'right_vals'):
        getattr(st, k)[:] = rs.standard_normal(getattr(st, k).shape)
    st.left_ts[:] = st.right_ts[:] = 1000.0      # a restart may move times back: no check
    st.has_msg[:] = rs.uniform(size=st.n_nodes) < 0.5
    nids = np.unique(np.concatenate([src[-30:], dst[-30:]]))
    t = np.full(len(nids), ts[-1] + 1)
    push(st, orc)
    with torch.no_grad():
        hl, hr, pt = orc.restarter_forward(nids, t)
        orc.restart(nids, t)
    assert S.restart_apply(st, nids, hl.numpy(), hr.numpy(), pt.numpy()) == 0
    assert_same(st, orc, 'restart')
    assert st.left_active[nids].all() and st.right_active[nids].all() and st.left_active.sum() == len(nids)


def test_effective_rows_serve_adopt_round_trip():
    """gather_eff_rows is the row STEP 4 would leave; serve then adopt moves the named rows and times and nothing else"""
    for msg_src in ('left', 'right'):
        _, st, _, _ = build(msg_src, False, False, 'floor', seed=6)
        rs = np.random.RandomState(7)
        for k in ('left_vals', 'right_vals', 'pending_vals'):
            getattr(st, k)[:] = rs.standard_normal(getattr(st, k).shape)
        for k in ('left_ts', 'right_ts', 'msg_ts'):
            getattr(st, k)[:] = rs.uniform(0, 100, st.n_nodes)
        st.has_msg[:] = rs.uniform(size=st.n_nodes) < 0.5
        ids = rs.permutation(st.n_nodes)[:20]
        rows, ts = S.gather_eff_rows(st, ids)
        after = st.copy()
        S.consume_update_right(after, ids, st.pending_vals, row_index=ids)
        np.testing.assert_array_equal(rows, after.right_vals[ids])
        np.testing.assert_array_equal(ts, after.right_ts[ids])
        eff, msg = ids[:12], ids[8:]
        pos = rs.permutation(40)
        out = np.full((40, st.d + 1), -7.0, np.float32)
        S.serve_rows(st, eff, pos[:12], msg, pos[12:24], out)
        assert (out[pos[24:]] == -7.0).all()
        other = st.copy()
        for k in ('left_vals', 'right_vals', 'left_ts', 'right_ts'):
            getattr(other, k)[:] = 0
        S.adopt_rows(other, eff, pos[:12], msg, pos[12:24], out)
        np.testing.assert_array_equal(other.right_vals[eff[:8]], rows[:8])
        np.testing.assert_array_equal(other.right_ts[eff[:8]], ts[:8])
        mv, mt = other.mem()
        if msg_src == 'left':
            np.testing.assert_array_equal(mv[msg], st.left_vals[msg])
            np.testing.assert_array_equal(mt[msg], st.left_ts[msg])
        else:
            np.testing.assert_array_equal(mv[msg], rows[8:])
            np.testing.assert_array_equal(mt[msg], ts[8:])
        untouched = np.setdiff1d(np.arange(st.n_nodes), ids)
        assert not other.right_vals[untouched].any() and not other.left_vals[untouched].any()
