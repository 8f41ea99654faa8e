"""Releasing edge-feature rows without a GPU: tg_edge_rows_host against the numpy reference (remap, packed table and
renumbered eids, bit for bit), what it refuses, and the Python layers on host-only objects: Graph.renumbered,
NumericalFeature.compact_edge_rows / append_edge_rows after it, and a chain of extended / trimmed / release."""
import numpy as np
import pytest
import torch

from _append_ref import assert_same, host_append, host_build
from _edge_rows_ref import GUARD32, host_release, patterns, release_numpy, row_stream, table_of, tiny_eids
from _trim_ref import trim_numpy

N_ROWS = 41


def check(eid, n_rows, d_e, keep_from=None, pin=None, what=''):
    table = table_of(n_rows, d_e, seed=n_rows + d_e, special=True)
    before = table.copy()
    rc, remap, t_out, eid_out, n_live = host_release(eid, table, n_rows, keep_from, pin)
    assert rc == 0, what
    w_remap, w_table, w_eid = release_numpy(eid, table, n_rows, keep_from, pin)
    np.testing.assert_array_equal(remap, w_remap, err_msg=what)
    np.testing.assert_array_equal(eid_out, w_eid, err_msg=what)
    np.testing.assert_array_equal(t_out.view(np.int32), w_table.view(np.int32), err_msg=what)
    assert n_live == len(w_table) == int((remap >= 0).sum()) and remap[0] == 0
    np.testing.assert_array_equal(table.view(np.int32), before.view(np.int32))   # the input is only read
    kf = n_rows if keep_from is None else keep_from
    shift = n_rows - n_live
    np.testing.assert_array_equal(remap[kf:], np.arange(kf, n_rows) - shift)   # the tail moves as one block
    live = remap[remap >= 0]
    assert np.all(np.diff(live) == 1)   # monotone, dense
    return remap, n_live


def test_only_the_padding_row_and_an_empty_graph():
    remap, n_live = check(np.zeros(0, dtype=np.int32), 1, 4)
    assert remap.tolist() == [0] and n_live == 1


@pytest.mark.parametrize('d_e', [4, 8, 172])
def test_the_tiny_stream(d_e):
    eid, n_rows = tiny_eids()
    remap, n_live = check(eid, n_rows, d_e)
    assert n_live == n_rows and remap.tolist() == list(range(n_rows))   # every event is in the graph: the identity


@pytest.mark.parametrize('d_e', [4, 8, 172])
@pytest.mark.parametrize('name', list(patterns(N_ROWS)))
def test_live_patterns(name, d_e):
    eid = patterns(N_ROWS)[name]
    remap, n_live = check(eid, N_ROWS, d_e, what=name)
    if name == 'all-live':
        assert n_live == N_ROWS and remap.tolist() == list(range(N_ROWS))   # identity, shift 0
    if name == 'none-but-0':
        assert n_live == 1 and remap[1:].tolist() == [-1] * (N_ROWS - 1)
    if name == 'last-only':
        assert n_live == 2 and remap[-1] == 1
    if name == 'alternating':
        assert remap[1::2].tolist() == list(range(1, 1 + N_ROWS // 2)) and (remap[2::2] == -1).all()
    if name == 'self-loop':
        _, _, _, eid_out, _ = host_release(eid, None, N_ROWS)
        assert eid_out.view(np.uint32).tolist() == [1, 1 | 0x80000000]   # one row, both flag values kept


@pytest.mark.parametrize('keep_from', [0, N_ROWS // 2, N_ROWS])
@pytest.mark.parametrize('name', ['none-but-0', 'alternating', 'random-third'])
def test_keep_from(name, keep_from):
    remap, n_live = check(patterns(N_ROWS)[name], N_ROWS, 8, keep_from=keep_from, what=f'{name} keep_from={keep_from}')
    if keep_from == 0:
        assert n_live == N_ROWS   # everything is pending: nothing can go


@pytest.mark.parametrize('pin', [[2, 4], [1, 3], [0], [6, 6, 6], [2, 1, 0, 2, N_ROWS - 1], []], ids=str)
def test_pins_of_dead_rows_live_rows_row_0_and_duplicates(pin):
    eid = patterns(N_ROWS)['alternating']   # rows 1, 3, 5, .. are live
    remap, _ = check(eid, N_ROWS, 8, pin=pin, what=f'pin={pin}')
    assert all(remap[p] >= 0 for p in pin)
    check(eid, N_ROWS, 4, keep_from=30, pin=pin)


def test_an_entry_or_a_pin_that_names_no_row_is_refused_and_nothing_is_written():
    from www2023tiger_amd._lib import TG_EINVAL
    table = table_of(N_ROWS, 8)
    eid = patterns(N_ROWS)['random-third'].copy()
    eid[len(eid) // 2] = N_ROWS   # the first id past the table
    for e, pin in ((eid, None), (eid | np.int32(-0x80000000), None), (patterns(N_ROWS)['alternating'], [3, N_ROWS]),
                   (patterns(N_ROWS)['alternating'], [-1])):
        rc, remap, t_out, eid_out, n_live = host_release(e, table, N_ROWS, None, pin)
        assert rc == TG_EINVAL and n_live == -7
        assert (remap == GUARD32).all() and (eid_out == GUARD32).all() and (t_out.view(np.int32) == GUARD32).all()


def test_bad_arguments():
    import ctypes as C
    from www2023tiger_amd._lib import TG_EINVAL, TgTcsr, lib, ptr
    eid = patterns(N_ROWS)['alternating']
    table = table_of(N_ROWS, 8)
    for kf in (-1, N_ROWS + 1):
        assert host_release(eid, table, N_ROWS, kf)[0] == TG_EINVAL
    assert host_release(eid, table.reshape(-1, 2)[:N_ROWS].copy(), N_ROWS)[0] == TG_EINVAL   # d_e % 4 != 0
    out = np.empty(N_ROWS, dtype=np.int32)
    n = C.c_int64(0)
    for n_rows, ne, n_pin in ((0, 3, 0), (2 ** 31, 3, 0), (N_ROWS, -1, 0), (N_ROWS, 2 ** 32, 0), (N_ROWS, 3, -1)):
        g = TgTcsr(1, ne, None, None, None, ptr(eid))
        assert lib.tg_edge_rows_host(C.byref(g), None, n_rows, 0, min(n_rows, N_ROWS), None, n_pin, ptr(out), None, ptr(out),
                                     C.byref(n)) == TG_EINVAL
    assert lib.tg_edge_rows_workspace_bytes(0, 3) == 0 and lib.tg_edge_rows_workspace_bytes(N_ROWS, -1) == 0
    assert lib.tg_edge_rows_workspace_bytes(N_ROWS, 3) >= 5 * N_ROWS   # a mark byte and an int32 of the inverse list per row


def test_the_device_entries_check_their_arguments_before_any_launch():
    """callable here: every refusal comes before the first launch"""
    import ctypes as C
    from www2023tiger_amd._lib import TG_EINVAL, TG_EWORKSPACE, TgTcsr, lib
    fake = 1 << 20   # (never dereferenced)
    g = TgTcsr(1, 4, None, None, None, fake)
    need = lib.tg_edge_rows_workspace_bytes(N_ROWS, 4)
    plan = lambda n_rows=N_ROWS, kf=N_ROWS, pin=None, n_pin=0, ws=fake, nb=need: lib.tg_edge_rows_plan(
        C.byref(g), n_rows, kf, pin, n_pin, fake, fake, ws, nb, None)
    assert plan(nb=need - 1) == TG_EWORKSPACE and plan(ws=None) == TG_EWORKSPACE
    assert plan(kf=-1) == plan(kf=N_ROWS + 1) == plan(n_pin=-1) == plan(n_pin=2) == plan(n_rows=0) == TG_EINVAL
    apply = lambda n_live=5, d_e=8, nb=need, table=fake: lib.tg_edge_rows_apply(
        C.byref(g), table, N_ROWS, d_e, fake, n_live, fake, fake, fake, nb, None)
    assert apply(nb=need - 1) == TG_EWORKSPACE
    assert apply(n_live=0) == apply(n_live=N_ROWS + 1) == apply(d_e=6) == apply(d_e=0) == apply(d_e=-4) == TG_EINVAL


# ------------------------------------------------------------------------- Graph.renumbered, compact_edge_rows: host only
def graph_of(N, ev, **kw):
    from www2023tiger_amd.data.graph import Graph
    return Graph.from_arrays(*ev, max_node_id=N - 1, **kw)


def feats(table, **kw):
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    return NumericalFeature(None, torch.from_numpy(table.copy()), table.shape[1], **kw)


def test_renumbered_on_a_host_only_parent_shares_what_it_does_not_change():
    from www2023tiger_amd import hip_ops
    N, E = 30, 200
    ev = row_stream(N, E, seed=3)
    g0 = graph_of(N, ev, strategy='recent_edges', seed=3).trimmed(keep_last=3)
    g0.alpha = 0.25
    h0 = [a.copy() for a in g0._host_tcsr()]
    table = table_of(E + 1, 8, special=True)
    remap, t_out, eid_out = hip_ops.edge_rows_host(g0, table, E + 1, keep_from=E - 10, pin=[1, 2])
    w_remap, w_table, w_eid = release_numpy(h0[3], table, E + 1, E - 10, [1, 2])
    np.testing.assert_array_equal(remap, w_remap)
    np.testing.assert_array_equal(t_out.view(np.int32), w_table.view(np.int32))
    np.testing.assert_array_equal(eid_out, w_eid)
    assert 1 < len(t_out) < E + 1
    g1 = g0.renumbered(remap, eid_out)
    assert g1 is not g0 and g1.serial != g0.serial and g1._root is not g0._root and g1.num_node == N
    for i in range(3):
        assert g1._host_tcsr()[i] is g0._host_tcsr()[i]   # indptr, ts and nbr are shared, not copied
    np.testing.assert_array_equal(g1._host_tcsr()[3], w_eid)
    assert_same(g0._host_tcsr(), h0, 'the parent is unchanged')
    assert (g1.strategy, g1.seed, g1.alpha, g1._device) == (g0.strategy, g0.seed, g0.alpha, g0._device)
    assert g1.rng is g0.rng and g1._time_ordered == g0._time_ordered and g1._t_last == g0._t_last
    assert g1._events is None   # a capped trim is no event list, renumbered or not
    with pytest.raises(ValueError, match='int32'):
        g0.renumbered(remap, eid_out[:-1])
    with pytest.raises(ValueError, match='int32'):
        g0.renumbered(remap, eid_out.astype(np.int64))
    with pytest.raises(ValueError, match='before the latest event'):
        g1.extended(ev[0][:1], ev[1][:1], ev[2][-1:] - 1, ev[3][:1])


def test_renumbered_pushes_an_event_list_through_the_remap():
    from www2023tiger_amd import hip_ops
    N, E = 30, 200
    ev = row_stream(N, E, seed=4)
    t_cut = float(ev[2][120])
    g0 = graph_of(N, ev).trimmed(before=t_cut)   # a horizon alone: still an event list
    remap, _, eid_out = hip_ops.edge_rows_host(g0, None, E + 1)
    g1 = g0.renumbered(remap, eid_out)
    m = ev[2] >= t_cut
    np.testing.assert_array_equal(g1._events[3], np.arange(1, 1 + int(m.sum())))
    assert_same(g1._host_tcsr(), host_build(N, ev[0][m], ev[1][m], ev[2][m], g1._events[3]), 'the build over the new ids')


def test_edge_rows_host_refuses_what_the_twin_refuses():
    from www2023tiger_amd import hip_ops
    g = graph_of(30, row_stream(30, 200, seed=5))
    with pytest.raises(ValueError, match='names no row'):
        hip_ops.edge_rows_host(g, None, 200)   # eid 200 is row 200: the table is one row short
    with pytest.raises(ValueError, match='names no row'):
        hip_ops.edge_rows_host(g, None, 201, pin=[201])
    for kf in (-1, 202):
        with pytest.raises(ValueError, match='keep_from'):
            hip_ops.edge_rows_host(g, None, 201, keep_from=kf)


def test_compact_edge_rows_on_a_host_table_and_append_after_it():
    N, E = 30, 200
    ev = row_stream(N, E, seed=6)
    table = table_of(E + 1, 8, special=True)
    g = graph_of(N, ev).trimmed(keep_last=2)
    fg = feats(table)
    res = fg.compact_edge_rows(g, keep_from=E - 4)
    w_remap, w_table, w_eid = release_numpy(g._host_tcsr()[3], table, E + 1, E - 4)
    n_live = len(w_table)
    assert (res.rows_before, res.rows, res.shift) == (E + 1, n_live, E + 1 - n_live) and n_live < E + 1
    np.testing.assert_array_equal(res.remap.numpy(), w_remap)
    np.testing.assert_array_equal(np.asarray(res.eid_out), w_eid)
    assert fg.n_edges == n_live and tuple(fg.efeats.shape) == (n_live, 8)
    np.testing.assert_array_equal(fg.efeats.numpy().view(np.int32), w_table.view(np.int32))
    # head-room: n_live + max(16, n_live // 4) rows, efeats the leading view
    assert fg._ef_store.shape[0] == n_live + max(16, n_live // 4) and fg._ef_store.data_ptr() == fg.efeats.data_ptr()
    new = table_of(10, 8, seed=9)
    assert fg.append_edge_rows(torch.from_numpy(new)) is False   # lands at row n_live, the table does not move
    assert fg.n_edges == n_live + 10
    np.testing.assert_array_equal(fg.efeats[n_live:].numpy().view(np.int32), new.view(np.int32))
    np.testing.assert_array_equal(fg.efeats[:n_live].numpy().view(np.int32), w_table.view(np.int32))
    # slack=: that many spare rows; one more row than the slack moves the table
    fg = feats(table)
    res = fg.compact_edge_rows(g, slack=3)
    assert fg._ef_store.shape[0] == res.rows + 3
    assert fg.append_edge_rows(torch.from_numpy(table_of(3, 8))) is False
    assert fg.append_edge_rows(torch.from_numpy(table_of(1, 8))) is True
    # swap=False changes nothing until it is adopted
    fg = feats(table)
    res = fg.compact_edge_rows(g, swap=False)
    assert fg.n_edges == E + 1 and fg.efeats.shape[0] == E + 1
    fg.adopt_edge_rows(res)
    assert fg.n_edges == res.rows == fg.efeats.shape[0]


def test_compact_edge_rows_refusals_and_the_model_without_a_table():
    from www2023tiger_amd.model.feature_getter import NumericalFeature
    N, E = 30, 200
    g = graph_of(N, row_stream(N, E, seed=6)).trimmed(keep_last=2)
    table = table_of(E + 1, 8)
    assert NumericalFeature(None, None, 8).compact_edge_rows(g) is None   # no edge table: nothing to do
    fg = feats(table, register_buffer=False)
    with pytest.raises(NotImplementedError, match='pinned host memory'):
        fg.compact_edge_rows(g)
    fg = feats(table)
    for bad in (dict(keep_from=-1), dict(keep_from=E + 2), dict(pin=[E + 1]), dict(slack=-1)):
        with pytest.raises(ValueError):
            fg.compact_edge_rows(g, **bad)
    short = feats(table[:E])   # the graph names row E
    with pytest.raises(ValueError, match='names no row'):
        short.compact_edge_rows(g.extended(*(a[-1:] + (1 if i == 2 else 0) for i, a in enumerate(row_stream(N, E, seed=6)))))
    assert fg.n_edges == E + 1 and fg.efeats.shape[0] == E + 1 and getattr(fg, '_ef_store', None) is None
    np.testing.assert_array_equal(fg.efeats.numpy().view(np.int32), table.view(np.int32))


def test_extended_trimmed_release_extended_release_equals_the_references_in_the_same_order():
    N, E = 60, 600
    s = row_stream(N, E, seed=31)
    part = lambda lo, hi, sh=0: tuple(np.ascontiguousarray(a[lo:hi]) - (sh if i == 3 else 0) for i, a in enumerate(s))
    table = table_of(E + 1, 8, special=True)
    fg = feats(table[:401])   # rows of the events observed so far
    # the library: extended -> trimmed -> release -> extended -> release
    g = graph_of(N, part(0, 200)).extended(*part(200, 400)).trimmed(keep_last=3)
    r1 = fg.compact_edge_rows(g)
    g = g.renumbered(r1.remap, r1.eid_out)
    assert r1.shift > 0
    fg.append_edge_rows(torch.from_numpy(table[401:]))   # the rows of the pending events, behind the packed ones
    g = g.extended(*part(400, 500, r1.shift))   # the caller's pending eids go through `- shift`
    r2 = fg.compact_edge_rows(g, keep_from=501 - r1.shift)   # events 500 .. 599 are not observed yet
    g = g.renumbered(r2.remap, r2.eid_out)
    # the references in the same order
    h = trim_numpy(host_append(N, host_build(N, *part(0, 200)), part(200, 400))[1], -np.inf, 3)
    m1, t1, e1 = release_numpy(h[3], table[:401], 401)
    h = host_append(N, (h[0], h[1], h[2], e1), part(400, 500, 401 - len(t1)))[1]
    t1 = np.concatenate([t1, table[401:]])
    m2, t2, e2 = release_numpy(h[3], t1, len(t1), 501 - r1.shift)
    assert_same(g._host_tcsr(), (h[0], h[1], h[2], e2), 'the chain')
    np.testing.assert_array_equal(fg.efeats.numpy().view(np.int32), t2.view(np.int32))
    np.testing.assert_array_equal(r2.remap.numpy(), m2)
    assert r2.shift == 0 or (r2.remap[501 - r1.shift:].numpy() == np.arange(501 - r1.shift, len(t1)) - r2.shift).all()
    # every entry of the final graph names the row its event had in the full table
    e = g._host_tcsr()[3].view(np.uint32) & np.uint32(0x7FFFFFFF)
    old = np.flatnonzero(m1 >= 0)   # first release: new row -> old row
    back = np.concatenate([old, np.arange(401, E + 1)])[np.flatnonzero(m2 >= 0)]
    np.testing.assert_array_equal(fg.efeats.numpy().view(np.int32), table[back].view(np.int32))
    assert len(np.unique(back[e])) > 10
